// diffmat.cpp -- Chebyshev collocation differentiation matrix on the Gauss-Lobatto nodes
// x_i = cos(i pi/n), split by parity and laid out as f64 MFMA operand fragments.
//
// The reference never forms this matrix: chebyshev.c:142-199 applies it as
// DCT-I -> (times k) -> DST-I -> /(2n sin) plus two endpoint sums.  In exact arithmetic
// that chain IS multiplication by D below (the derivative of the degree-n interpolant at
// the nodes), so y = D x reproduces ChebMult to rounding.  P = 256 and 128 make the
// logical FFT length 2(P-1) = 510 = 2*3*5*17 and 254 = 2*127, hostile to butterflies; a
// dense product on the matrix cores, halved by the centro-antisymmetry of D, is both
// faster on gfx950 and more accurate (see DESIGN.md "Why dense").
//
// Parity split (n = P-1, H = ceil(P/2)); for j < H with 2j != n:
//     e_j = x_j + x_{n-j},  o_j = x_j - x_{n-j};   self-paired middle (2j == n): e_j = x_j, o_j = 0
//     ME[i][j] = (D[i][j] + D[i][n-j]) / 2   (middle column: D[i][j])
//     MO[i][j] = (D[i][j] - D[i][n-j]) / 2   (middle column: 0)
// and because D[n-i][n-j] = -D[i][j]:
//     y_i = (ME e)_i + (MO o)_i,      y_{n-i} = (MO o)_i - (ME e)_i,     i < H.
#include "sweep.h"
#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <limits>
#include <vector>

namespace chebhip {

static const long double PI_L = 3.14159265358979323846264338327950288L;

// sin(k pi / 2n) for |k| <= 2n with the argument folded into [0, pi/2] (sin(pi - t) = sin t): PI_L carries a rounding error of
// 2^-65 pi, and near t = pi that absolute error is relative to a SMALL sine -- unfolded, the entries of D next to the far
// corner were off by up to 4e-17 of their size, and D D, which cancels by four orders of magnitude at P = 256, turned that into
// 5e-14 of an entry of the second-derivative matrix.
static long double sin_half(int k, int n) {
  int a = k < 0 ? -k : k;
  if (a > n) a = 2 * n - a;
  const long double s = sinl(PI_L * a / (2.0L * n));
  return k < 0 ? -s : s;
}

// D[i][j] in long double.  Off-diagonal: (c_i/c_j) (-1)^(i+j) / (x_i - x_j) with
// x_i - x_j = -2 sin((i+j) pi/2n) sin((i-j) pi/2n) (no cancellation); diagonal from the
// closed forms  D00 = (2n^2+1)/6 = -Dnn,  Dii = -x_i / (2 sin^2(i pi/n)),  x_i = sin((n-2i) pi/2n).
static long double dentry(int i, int j, int n) {
  if (i == j) {
    if (i == 0) return (2.0L * n * n + 1.0L) / 6.0L;
    if (i == n) return -(2.0L * n * n + 1.0L) / 6.0L;
    if (2 * i == n) return 0.0L;                 // x_i = 0 exactly
    long double s = sin_half(2 * i, n);
    return -sin_half(n - 2 * i, n) / (2.0L * s * s);
  }
  long double ci = (i == 0 || i == n) ? 2.0L : 1.0L;
  long double cj = (j == 0 || j == n) ? 2.0L : 1.0L;
  long double sgn = ((i + j) & 1) ? -1.0L : 1.0L;
  long double dx = -2.0L * sin_half(i + j, n) * sin_half(i - j, n);
  return (ci / cj) * sgn / dx;
}

void diffmat_dense_host(int P, double *D) {
  const int n = P - 1;
  for (int i = 0; i < P; i++)
    for (int j = 0; j < P; j++) D[(size_t)i * P + j] = (double)dentry(i, j, n);
}

// [m-tile][k-step][lane] -> [m-tile][k-step pair][lane][2]: a lane fetches two fragments with one 16-byte load
static hipError_t upload_paired(const std::vector<double> &f, int MTP, int KS, double *dev) {
  std::vector<double> g(f.size());
  for (int mt = 0; mt < MTP; mt++)
    for (int s = 0; s < KS; s++)
      for (int l = 0; l < 64; l++)
        g[(((size_t)mt * (KS / 2) + s / 2) * 64 + l) * 2 + (s & 1)] = f[((size_t)mt * KS + s) * 64 + l];
  return hipMemcpy(dev, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice);
}

// P > 256: the matrix does not fit the register file of a workgroup; cheb_sweep_long_kernel streams the dense
// transpose from L2 instead (a correctness path for any extent the reference accepts, not a tuned one).
static hipError_t diffmat_create_long(int P, DiffMat *out) {
  std::vector<double> DT((size_t)P * P), D((size_t)P * P);
  const int n = P - 1;
  for (int i = 0; i < P; i++) for (int j = 0; j < P; j++) { const double v = (double)dentry(i, j, n); DT[(size_t)j * P + i] = v; D[(size_t)i * P + j] = v; }
  DiffMat m;
  m.P = P; m.H = (P + 1) / 2; m.KS = 0; m.MTP = 0;
  // Lines of up to 1024 points: the even / odd halves in MFMA-operand order for cheb_sweep_xl_kernel (sweep_xl.hip):
  // [m-tile][k-step][64 lanes], m-tiles padded by a workgroup's worth (16), k-steps to a multiple of 8; zero padded.
  std::vector<double> fe, fo;
  size_t cnt = 0;
  if (P <= 1024) {
    const int H = m.H;
    m.MTP = (H + 15) / 16 + 16;                  // (a workgroup covers up to 16 m-tiles: its last one starts below ceil(H/16))
    m.xl_ks = ((H + 3) / 4 + 7) / 8 * 8;
    cnt = (size_t)m.MTP * m.xl_ks * 64;
    fe.assign(cnt, 0.0); fo.assign(cnt, 0.0);
    for (int mt = 0; mt < m.MTP; mt++)
      for (int s = 0; s < m.xl_ks; s++)
        for (int l = 0; l < 64; l++) {
          const int i = mt * 16 + (l & 15), j = 4 * s + (l >> 4);
          if (i >= H || j >= H) continue;
          long double me, mo;
          if (2 * j == n) { me = dentry(i, j, n); mo = 0.0L; }
          else { const long double a = dentry(i, j, n), b = dentry(i, n - j, n); me = 0.5L * (a + b); mo = 0.5L * (a - b); }
          fe[((size_t)mt * m.xl_ks + s) * 64 + l] = (double)me;
          fo[((size_t)mt * m.xl_ks + s) * 64 + l] = (double)mo;
        }
  }
  hipError_t e = hipMalloc((void **)&m.fragE, (cnt + 8 + 1024) * sizeof(double));
  if (e != hipSuccess) return e;
  m.zero = m.fragE + cnt; m.sink = m.zero + 8;
  e = hipMemset(m.zero, 0, 8 * sizeof(double));
  if (e == hipSuccess && cnt) e = hipMemcpy(m.fragE, fe.data(), cnt * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess && cnt) e = hipMalloc((void **)&m.fragO, cnt * sizeof(double));
  if (e == hipSuccess && cnt) e = hipMemcpy(m.fragO, fo.data(), cnt * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void **)&m.longDT, DT.size() * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(m.longDT, DT.data(), DT.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void **)&m.longD, D.size() * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(m.longD, D.data(), D.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(m.fragE); if (m.fragO) (void)hipFree(m.fragO); if (m.longDT) (void)hipFree(m.longDT); if (m.longD) (void)hipFree(m.longD); return e; }
  *out = m;
  return hipSuccess;
}

hipError_t diffmat_create(int P, DiffMat *out) {
  // option "force_gemm" (A/B measurements only): every extent takes the long-line route, i.e. a library DGEMM
  const int force = opt(OPT_FORCE_GEMM);
  if (P > 256 || (force && P >= 4)) return diffmat_create_long(P, out);
  const int n = P - 1;
  const int H = (P + 1) / 2;
  int KS = 4;
  while (4 * KS < H) KS *= 2;
  const int MTP = KS / 4;
  const size_t cnt = (size_t)MTP * KS * 64;
  std::vector<double> fe(cnt, 0.0), fo(cnt, 0.0);
  for (int mt = 0; mt < MTP; mt++)
    for (int s = 0; s < KS; s++)
      for (int l = 0; l < 64; l++) {
        const int i = mt * 16 + (l & 15);  // output row held by this lane
        const int j = 4 * s + (l >> 4);    // reduction index
        if (i >= H || j >= H) continue;
        long double me, mo;
        if (2 * j == n) { me = dentry(i, j, n); mo = 0.0L; }
        else {
          const long double a = dentry(i, j, n), b = dentry(i, n - j, n);
          me = 0.5L * (a + b); mo = 0.5L * (a - b);
        }
        fe[((size_t)mt * KS + s) * 64 + l] = (double)me;
        fo[((size_t)mt * KS + s) * 64 + l] = (double)mo;
      }
  DiffMat m;
  m.P = P; m.H = H; m.KS = KS; m.MTP = MTP;
  hipError_t e = hipMalloc((void **)&m.fragE, (cnt + 8 + 1024) * sizeof(double));
  if (e != hipSuccess) return e;
  e = hipMalloc((void **)&m.fragO, 3 * cnt * sizeof(double));
  if (e != hipSuccess) { (void)hipFree(m.fragE); return e; }
  m.fragE2 = m.fragO + cnt; m.fragO2 = m.fragO + 2 * cnt;
  m.zero = m.fragE + cnt;
  m.sink = m.zero + 8;
  e = hipMemset(m.zero, 0, 8 * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(m.fragE, fe.data(), cnt * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m.fragO, fo.data(), cnt * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = upload_paired(fe, MTP, KS, m.fragE2);
  if (e == hipSuccess) e = upload_paired(fo, MTP, KS, m.fragO2);
  if (e != hipSuccess) { (void)hipFree(m.fragE); (void)hipFree(m.fragO); return e; }
  *out = m;
  return hipSuccess;
}

// Fragments of a dense M x M matrix A (row-major, long double) that is centro-symmetric (sym = 1:
// A[m-i][m-j] = A[i][j], m = M-1) or centro-antisymmetric (sym = 0).  With e, o as above
//     y_i = (ME e)_i + (MO o)_i,   y_{m-i} = (ME e)_i - (MO o)_i   (sym = 1; sym = 0: (MO o)_i - (ME e)_i).
hipError_t diffmat_from_dense(int M, const long double *A, int sym, DiffMat *out) {
  if (M < 1 || M > 256) return hipErrorInvalidValue;
  const int m = M - 1, H = (M + 1) / 2;
  std::vector<long double> ME((size_t)H * H), MO((size_t)H * H);
  for (int i = 0; i < H; i++)
    for (int j = 0; j < H; j++) {
      long double me, mo;
      if (2 * j == m) { me = A[(size_t)i * M + j]; mo = 0.0L; }
      else {
        const long double a = A[(size_t)i * M + j], b = A[(size_t)i * M + (m - j)];
        me = 0.5L * (a + b); mo = 0.5L * (a - b);
      }
      ME[(size_t)i * H + j] = me; MO[(size_t)i * H + j] = mo;
    }
  return diffmat_from_blocks(M, ME.data(), MO.data(), sym, out);
}

hipError_t diffmat_from_blocks(int M, const long double *ME, const long double *MO, int sym, DiffMat *out) {
  if (M < 1 || M > 256) return hipErrorInvalidValue;
  const int H = (M + 1) / 2;
  int KS = 4;
  while (4 * KS < H) KS *= 2;
  const int MTP = KS / 4;
  const size_t cnt = (size_t)MTP * KS * 64;
  std::vector<double> fe(cnt, 0.0), fo(cnt, 0.0);
  for (int mt = 0; mt < MTP; mt++)
    for (int s = 0; s < KS; s++)
      for (int l = 0; l < 64; l++) {
        const int i = mt * 16 + (l & 15), j = 4 * s + (l >> 4);
        if (i >= H || j >= H) continue;
        fe[((size_t)mt * KS + s) * 64 + l] = (double)ME[(size_t)i * H + j];
        fo[((size_t)mt * KS + s) * 64 + l] = (double)MO[(size_t)i * H + j];
      }
  DiffMat r;
  r.P = M; r.H = H; r.KS = KS; r.MTP = MTP; r.sym = sym;
  hipError_t e = hipMalloc((void **)&r.fragE, (cnt + 8 + 1024) * sizeof(double));
  if (e != hipSuccess) return e;
  e = hipMalloc((void **)&r.fragO, 3 * cnt * sizeof(double));
  if (e != hipSuccess) { (void)hipFree(r.fragE); return e; }
  r.fragE2 = r.fragO + cnt; r.fragO2 = r.fragO + 2 * cnt;
  r.zero = r.fragE + cnt;
  r.sink = r.zero + 8;
  e = hipMemset(r.zero, 0, 8 * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(r.fragE, fe.data(), cnt * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(r.fragO, fo.data(), cnt * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = upload_paired(fe, MTP, KS, r.fragE2);
  if (e == hipSuccess) e = upload_paired(fo, MTP, KS, r.fragO2);
  if (e != hipSuccess) { (void)hipFree(r.fragE); (void)hipFree(r.fragO); return e; }
  *out = r;
  return hipSuccess;
}

// Second-derivative operator of a zero-Dirichlet line, restricted to its interior:
//   L = (D D)[1..n-1, 1..n-1],  M = P-2 points.
// For constant coefficients the two sweeps of a direction, D_k (1 * D_k w0) with w0 = 0 at both ends
// (elliptic.C:305-334 with eta = 1, deta = 0), collapse into y = L x on the interior values.  L is
// centro-SYMMETRIC.  The product is formed in long double and rounded once.
hipError_t diffmat_create_lap(int P, DiffMat *out) {
  const int n = P - 1, M = P - 2;
  std::vector<long double> D((size_t)P * P), L((size_t)M * M);
  for (int i = 0; i < P; i++) for (int j = 0; j < P; j++) D[(size_t)i * P + j] = dentry(i, j, n);
  for (int i = 0; i < M; i++)
    for (int j = 0; j < M; j++) {
      long double s = 0.0L;
      for (int q = 0; q < P; q++) s += D[(size_t)(i + 1) * P + q] * D[(size_t)q * P + (j + 1)];
      L[(size_t)i * M + j] = s;
    }
  return diffmat_from_dense(M, L.data(), 1, out);
}

// D with the end values of a line replaced by their extrapolation from the interior (StokesPressureReduceOrder,
// stokes.C:1029-1080: the degree-(P-3) polynomial through the interior values, evaluated at both ends):
//     x_0 = sum_j w0_j x_j,  x_n = sum_j w1_j x_j   (j = 1 .. n-1, Lagrange weights)
//     D (x_0, x_1 .. x_{n-1}, x_n)^T = Dext x,   Dext[i][j] = D[i][j] + D[i][0] w0_j + D[i][n] w1_j,  Dext[i][0] = Dext[i][n] = 0.
// w1_j = w0_{n-j} (mirror nodes), so Dext is centro-antisymmetric like D and runs on the same kernels.  Formed in long
// double, rounded once.  The interior values of a pressure-gradient line never depend on the extrapolations along the
// OTHER directions, so a Stokes callback needs no extrapolation pass at all (stokes.hip).
hipError_t diffmat_create_pext(int P, DiffMat *out) {
  if (P < 3 || P > 256) return hipErrorInvalidValue;
  const int n = P - 1, m = P - 2;
  std::vector<long double> x(P), w0(P, 0.0L), w1(P, 0.0L), A((size_t)P * P, 0.0L);
  for (int i = 0; i < P; i++) x[i] = cosl(PI_L * i / n);
  for (int j = 1; j <= m; j++) {
    long double l0 = 1.0L, l1 = 1.0L;
    for (int q = 1; q <= m; q++) if (q != j) { l0 *= (x[0] - x[q]) / (x[j] - x[q]); l1 *= (x[n] - x[q]) / (x[j] - x[q]); }
    w0[j] = l0; w1[j] = l1;
  }
  for (int i = 0; i < P; i++)
    for (int j = 1; j <= m; j++) A[(size_t)i * P + j] = dentry(i, j, n) + dentry(i, 0, n) * w0[j] + dentry(i, n, n) * w1[j];
  return diffmat_from_dense(P, A.data(), 0, out);
}

// D D on all P points (rows and columns 0 .. n): formed in long double, rounded once.  D is centro-antisymmetric, so the
// product is centro-symmetric.
hipError_t diffmat_create_dd(int P, DiffMat *out) {
  if (P < 3 || P > 256) return hipErrorInvalidValue;
  const int n = P - 1;
  std::vector<long double> D((size_t)P * P), A((size_t)P * P);
  for (int i = 0; i < P; i++) for (int j = 0; j < P; j++) D[(size_t)i * P + j] = dentry(i, j, n);
  for (int i = 0; i < P; i++)
    for (int j = 0; j < P; j++) {
      long double s = 0.0L;
      for (int q = 0; q < P; q++) s += D[(size_t)i * P + q] * D[(size_t)q * P + j];
      A[(size_t)i * P + j] = s;
    }
  return diffmat_from_dense(P, A.data(), 1, out);
}

// ---------------------------------------------------------------------------------------------
// Fast diagonalisation of the finite-difference preconditioner (elliptic.C:556-579 with eta = 1, deta = 0;
// stokes.C:1181-1226 per velocity component): on the tensor grid that matrix is  sum_k I x .. x T_k x .. x I  with
// the 1-D three-point operator T on the interior Gauss-Lobatto nodes,
//     (T u)_i = -idx (idxM u_{i-1} + idxP u_{i+1}) + idx (idxP + idxM) u_i,
//     idxM = 1/(x_i - x_{i-1}), idxP = 1/(x_{i+1} - x_i), idx = 1/(xP - xM), xM, xP the midpoints.
// T = H^-1 K with H = diag(-(xP - xM)) > 0 and K symmetric positive definite, so T = S Lambda S^-1 with
// S = H^-1/2 W, S^-1 = W^T H^1/2, W the orthonormal eigenvectors of H^-1/2 K H^-1/2 (implicit QL, long double).
// ---------------------------------------------------------------------------------------------
// EISPACK tql2: eigenvalues d[] and eigenvectors z (row-major n x n, identity on entry) of the symmetric
// tridiagonal matrix with diagonal d[] and sub-diagonal e[1..n-1] (e[0] unused)
static bool tql2(int n, std::vector<long double> &d, std::vector<long double> &e, std::vector<long double> &z) {
  for (int i = 1; i < n; i++) e[i - 1] = e[i];
  e[n - 1] = 0.0L;
  long double f = 0.0L, tst1 = 0.0L;
  for (int l = 0; l < n; l++) {
    const long double h0 = fabsl(d[l]) + fabsl(e[l]);
    if (tst1 < h0) tst1 = h0;
    int m = l;
    while (m < n - 1) { if (tst1 + fabsl(e[m]) == tst1) break; m++; }
    if (m != l) {
      int iter = 0;
      do {
        if (++iter > 200) return false;
        const long double g0 = d[l];
        long double p = (d[l + 1] - g0) / (2.0L * e[l]);
        long double r = hypotl(p, 1.0L);
        d[l] = e[l] / (p + (p < 0 ? -r : r));
        d[l + 1] = e[l] * (p + (p < 0 ? -r : r));
        const long double dl1 = d[l + 1];
        long double h = g0 - d[l];
        for (int i = l + 2; i < n; i++) d[i] -= h;
        f += h;
        p = d[m];
        long double c = 1.0L, c2 = c, c3 = c, s = 0.0L, s2 = 0.0L;
        const long double el1 = e[l + 1];
        for (int i = m - 1; i >= l; i--) {
          c3 = c2; c2 = c; s2 = s;
          const long double g = c * e[i];
          h = c * p;
          r = hypotl(p, e[i]);
          e[i + 1] = s * r;
          s = e[i] / r; c = p / r;
          p = c * d[i] - s * g;
          d[i + 1] = h + s * (c * g + s * d[i]);
          for (int k = 0; k < n; k++) {
            h = z[(size_t)k * n + i + 1];
            z[(size_t)k * n + i + 1] = s * z[(size_t)k * n + i] + c * h;
            z[(size_t)k * n + i] = c * z[(size_t)k * n + i] - s * h;
          }
        }
        p = -s * s2 * c3 * el1 * e[l] / dl1;
        e[l] = s * p;
        d[l] = c * p;
      } while (tst1 + fabsl(e[l]) > tst1);
    }
    d[l] += f;
  }
  return true;
}

// S (nodal <- modal), S^-1 and the eigenvalues of the 1-D operator T on the M = P-2 interior nodes of a line
bool fdm_line(int P, std::vector<long double> &S, std::vector<long double> &Sinv, std::vector<long double> &lam) {
  const int n = P - 1, M = P - 2;
  if (M < 1) return false;
  std::vector<long double> x(P), h(M), kd(M), ke(M, 0.0L);
  for (int i = 0; i < P; i++) x[i] = cosl(PI_L * i / n);
  for (int q = 0; q < M; q++) {
    const int i = q + 1;
    const long double idxM = 1.0L / (x[i] - x[i - 1]), idxP = 1.0L / (x[i + 1] - x[i]);
    h[q] = -0.5L * (x[i + 1] - x[i - 1]);              // -(xP - xM) > 0
    kd[q] = -(idxP + idxM);                            // K = -(reference's bracket): positive diagonal
    if (q > 0) ke[q] = idxM;                           // K[q][q-1] = idxM < 0
  }
  // A = H^-1/2 K H^-1/2: symmetric tridiagonal, diagonal d, sub-diagonal e[q] = A[q][q-1]
  std::vector<long double> d(M), e(M, 0.0L);
  for (int q = 0; q < M; q++) { d[q] = kd[q] / h[q]; if (q > 0) e[q] = ke[q] / sqrtl(h[q] * h[q - 1]); }
  // The nodes are symmetric about 0, so A is centro-symmetric and every eigenvector is even or odd under i -> M-1-i.
  // The modes localised at the two ends of the line come in even / odd pairs whose eigenvalues agree to far below
  // rounding, so a solver for the whole matrix returns arbitrary mixtures of each pair.  The two parity classes are
  // therefore diagonalised SEPARATELY: restricted to even (odd) vectors A is again tridiagonal, of half the size, with
  // simple well-separated eigenvalues.  Modes are laid out by parity -- position p < ceil(M/2): the p-th even mode,
  // position M-1-q: the q-th odd mode, both by ascending eigenvalue -- which is the layout the raw modes of the sweep
  // kernels read and write (sweep.h: SweepParams::raw).
  const int m = M - 1, He = (M + 1) / 2, Ho = M / 2;
  const bool has_mid = (M & 1) != 0;
  const long double r2 = sqrtl(2.0L);
  std::vector<long double> W((size_t)M * M, 0.0L);       // W[i][position]
  lam.assign(M, 0.0L);
  for (int parity = 0; parity < 2; parity++) {           // 0: even, 1: odd
    const int n = parity == 0 ? He : Ho;
    if (n == 0) continue;
    std::vector<long double> dd(n), ee(n, 0.0L), Z((size_t)n * n, 0.0L);
    for (int i = 0; i < n; i++) { dd[i] = d[i]; if (i > 0) ee[i] = e[i]; Z[(size_t)i * n + i] = 1.0L; }
    if (!has_mid) dd[n - 1] += (parity == 0 ? e[n] : -e[n]);        // the two middle points couple to each other
    else if (parity == 0 && n > 1) ee[n - 1] = r2 * e[n - 1];       // the middle point is its own mirror
    if (!tql2(n, dd, ee, Z)) return false;
    std::vector<int> ord(n);
    for (int j = 0; j < n; j++) ord[j] = j;
    std::sort(ord.begin(), ord.end(), [&](int a, int b) { return dd[a] < dd[b]; });
    for (int q = 0; q < n; q++) {
      const int j = ord[q], pos = parity == 0 ? q : m - q;
      lam[pos] = dd[j];
      for (int i = 0; i < n; i++) {
        const long double v = Z[(size_t)i * n + j];
        if (has_mid && parity == 0 && i == n - 1) W[(size_t)i * M + pos] = v;
        else { W[(size_t)i * M + pos] = v / r2; W[(size_t)(m - i) * M + pos] = (parity == 0 ? v : -v) / r2; }
      }
    }
  }
  S.assign((size_t)M * M, 0.0L); Sinv.assign((size_t)M * M, 0.0L);
  for (int i = 0; i < M; i++)
    for (int pos = 0; pos < M; pos++) {
      S[(size_t)i * M + pos] = W[(size_t)i * M + pos] / sqrtl(h[i]);
      Sinv[(size_t)pos * M + i] = W[(size_t)i * M + pos] * sqrtl(h[i]);
    }
  return true;
}

// ---------------------------------------------------------------------------------------------
// Fast diagonalisation of the SPECTRAL line operator (Haidvogel-Zang): A_1 = -(D D)[1..n-1, 1..n-1] on the M = P-2 interior
// nodes, the operator MatMult_Elliptic applies along one direction at eta == 1 (elliptic.C:305-334).  A_1 is not symmetric and
// no diagonal scaling makes it so; its eigenvalues are real, positive and simple (pi^2/4 .. ~0.05 n^4).  A_1 is centro-symmetric,
// so, as in fdm_line, the even and the odd vectors are diagonalised separately:
//     even half  Ae[i][j] = A[i][j] + A[i][m-j]   (odd M: the middle column j = m/2 once),   x_{m-i} = x_i
//     odd half   Ao[i][j] = A[i][j] - A[i][m-j],                                            x_{m-i} = -x_i (middle 0)
// Each half: balancing (exact powers of two), Householder reduction to Hessenberg form, Francis double-shift QR for the
// eigenvalues (EISPACK hqr), eigenvectors by inverse iteration on the Hessenberg matrix, all in long double.
// ---------------------------------------------------------------------------------------------
namespace {

typedef std::vector<long double> LVec;

// A <- D^-1 A D with D = diag(scale), powers of two (EISPACK balanc without the permutations)
void balance(int n, LVec &A, LVec &scale) {
  scale.assign(n, 1.0L);
  const long double RADIX = 2.0L, SQRDX = RADIX * RADIX;
  bool done = false;
  while (!done) {
    done = true;
    for (int i = 0; i < n; i++) {
      long double r = 0.0L, c = 0.0L;
      for (int j = 0; j < n; j++)
        if (j != i) { c += fabsl(A[(size_t)j * n + i]); r += fabsl(A[(size_t)i * n + j]); }
      if (c == 0.0L || r == 0.0L) continue;
      long double g = r / RADIX, f = 1.0L;
      const long double s = c + r;
      while (c < g) { f *= RADIX; c *= SQRDX; }
      g = r * RADIX;
      while (c > g) { f /= RADIX; c /= SQRDX; }
      if ((c + r) / f < 0.95L * s) {
        done = false;
        g = 1.0L / f;
        scale[i] *= f;
        for (int j = 0; j < n; j++) A[(size_t)i * n + j] *= g;
        for (int j = 0; j < n; j++) A[(size_t)j * n + i] *= f;
      }
    }
  }
}

// A <- Q^T A Q upper Hessenberg (Householder); Q (row-major, n x n) returned explicitly
void hessenberg(int n, LVec &A, LVec &Q) {
  Q.assign((size_t)n * n, 0.0L);
  for (int i = 0; i < n; i++) Q[(size_t)i * n + i] = 1.0L;
  LVec v(n);
  for (int k = 0; k + 2 < n; k++) {
    long double nx = 0.0L;
    for (int i = k + 1; i < n; i++) nx += A[(size_t)i * n + k] * A[(size_t)i * n + k];
    nx = sqrtl(nx);
    if (nx == 0.0L) continue;
    const long double x0 = A[(size_t)(k + 1) * n + k], alpha = x0 < 0 ? nx : -nx;
    long double vv = 0.0L;
    for (int i = k + 1; i < n; i++) { v[i] = A[(size_t)i * n + k]; }
    v[k + 1] -= alpha;
    for (int i = k + 1; i < n; i++) vv += v[i] * v[i];
    if (vv == 0.0L) continue;
    const long double beta = 2.0L / vv;
    for (int j = 0; j < n; j++) {                       // A <- (I - beta v v^T) A
      long double s = 0.0L;
      for (int i = k + 1; i < n; i++) s += v[i] * A[(size_t)i * n + j];
      s *= beta;
      for (int i = k + 1; i < n; i++) A[(size_t)i * n + j] -= s * v[i];
    }
    for (int i = 0; i < n; i++) {                       // A <- A (I - beta v v^T),  Q <- Q (I - beta v v^T)
      long double s = 0.0L, t = 0.0L;
      for (int j = k + 1; j < n; j++) { s += A[(size_t)i * n + j] * v[j]; t += Q[(size_t)i * n + j] * v[j]; }
      s *= beta; t *= beta;
      for (int j = k + 1; j < n; j++) { A[(size_t)i * n + j] -= s * v[j]; Q[(size_t)i * n + j] -= t * v[j]; }
    }
    for (int i = k + 2; i < n; i++) A[(size_t)i * n + k] = 0.0L;
  }
}

// Eigenvalues (wr, wi) of the upper Hessenberg matrix a (destroyed): EISPACK hqr, Francis double-shift QR
bool hqr(int n, LVec a, LVec &wr, LVec &wi) {
  auto A = [&](int i, int j) -> long double & { return a[(size_t)(i - 1) * n + (j - 1)]; };   // 1-based, as EISPACK
  wr.assign(n + 1, 0.0L); wi.assign(n + 1, 0.0L);
  long double anorm = 0.0L;
  for (int i = 1; i <= n; i++)
    for (int j = std::max(i - 1, 1); j <= n; j++) anorm += fabsl(A(i, j));
  int nn = n, l = 1;
  long double t = 0.0L, p = 0.0L, q = 0.0L, r = 0.0L, s, w, x, y, z;
  while (nn >= 1) {
    int its = 0;
    do {
      for (l = nn; l >= 2; l--) {
        s = fabsl(A(l - 1, l - 1)) + fabsl(A(l, l));
        if (s == 0.0L) s = anorm;
        if (fabsl(A(l, l - 1)) + s == s) { A(l, l - 1) = 0.0L; break; }
      }
      x = A(nn, nn);
      if (l == nn) { wr[nn] = x + t; wi[nn--] = 0.0L; }
      else {
        y = A(nn - 1, nn - 1);
        w = A(nn, nn - 1) * A(nn - 1, nn);
        if (l == nn - 1) {
          p = 0.5L * (y - x);
          q = p * p + w;
          z = sqrtl(fabsl(q));
          x += t;
          if (q >= 0.0L) {
            z = p + (p >= 0 ? z : -z);
            wr[nn - 1] = wr[nn] = x + z;
            if (z != 0.0L) wr[nn] = x - w / z;
            wi[nn - 1] = wi[nn] = 0.0L;
          } else {
            wr[nn - 1] = wr[nn] = x + p;
            wi[nn - 1] = -(wi[nn] = z);
          }
          nn -= 2;
        } else {
          if (its == 60) return false;
          if (its == 10 || its == 20 || its == 40) {       // exceptional shifts
            t += x;
            for (int i = 1; i <= nn; i++) A(i, i) -= x;
            s = fabsl(A(nn, nn - 1)) + fabsl(A(nn - 1, nn - 2));
            y = x = 0.75L * s;
            w = -0.4375L * s * s;
          }
          ++its;
          int m;
          for (m = nn - 2; m >= l; m--) {
            z = A(m, m);
            r = x - z;
            s = y - z;
            p = (r * s - w) / A(m + 1, m) + A(m, m + 1);
            q = A(m + 1, m + 1) - z - r - s;
            r = A(m + 2, m + 1);
            s = fabsl(p) + fabsl(q) + fabsl(r);
            p /= s; q /= s; r /= s;
            if (m == l) break;
            const long double u = fabsl(A(m, m - 1)) * (fabsl(q) + fabsl(r));
            const long double v = fabsl(p) * (fabsl(A(m - 1, m - 1)) + fabsl(z) + fabsl(A(m + 1, m + 1)));
            if (u + v == v) break;
          }
          for (int i = m + 2; i <= nn; i++) {
            A(i, i - 2) = 0.0L;
            if (i != m + 2) A(i, i - 3) = 0.0L;
          }
          for (int k = m; k <= nn - 1; k++) {
            if (k != m) {
              p = A(k, k - 1);
              q = A(k + 1, k - 1);
              r = 0.0L;
              if (k != nn - 1) r = A(k + 2, k - 1);
              if ((x = fabsl(p) + fabsl(q) + fabsl(r)) != 0.0L) { p /= x; q /= x; r /= x; }
            }
            const long double sq = sqrtl(p * p + q * q + r * r);
            if ((s = (p >= 0 ? sq : -sq)) != 0.0L) {
              if (k == m) { if (l != m) A(k, k - 1) = -A(k, k - 1); }
              else A(k, k - 1) = -s * x;
              p += s;
              x = p / s; y = q / s; z = r / s;
              q /= p; r /= p;
              for (int j = k; j <= nn; j++) {
                p = A(k, j) + q * A(k + 1, j);
                if (k != nn - 1) { p += r * A(k + 2, j); A(k + 2, j) -= p * z; }
                A(k + 1, j) -= p * y;
                A(k, j) -= p * x;
              }
              const int mmin = nn < k + 3 ? nn : k + 3;
              for (int i = l; i <= mmin; i++) {
                p = x * A(i, k) + y * A(i, k + 1);
                if (k != nn - 1) { p += z * A(i, k + 2); A(i, k + 2) -= p * r; }
                A(i, k + 1) -= p * q;
                A(i, k) -= p;
              }
            }
          }
        }
      }
    } while (l < nn - 1);
  }
  wr.erase(wr.begin()); wi.erase(wi.begin());
  return true;
}

// Eigenvector y of the upper Hessenberg matrix H for its eigenvalue mu: inverse iteration, (H - mu I) = LU with partial pivoting
// (neighbouring rows only), a zero pivot replaced by eps |H|
void hess_inverse_iteration(int n, const LVec &H, long double mu, long double hnorm, LVec &y) {
  LVec U((size_t)n * n);
  for (size_t i = 0; i < U.size(); i++) U[i] = H[i];
  for (int i = 0; i < n; i++) U[(size_t)i * n + i] -= mu;
  std::vector<char> swp(n, 0);
  LVec lm(n, 0.0L);
  const long double tiny = 1e-19L * (hnorm > 0 ? hnorm : 1.0L);
  for (int k = 0; k + 1 < n; k++) {
    if (fabsl(U[(size_t)(k + 1) * n + k]) > fabsl(U[(size_t)k * n + k])) {
      swp[k] = 1;
      for (int j = k; j < n; j++) std::swap(U[(size_t)k * n + j], U[(size_t)(k + 1) * n + j]);
    }
    if (U[(size_t)k * n + k] == 0.0L) U[(size_t)k * n + k] = tiny;
    const long double f = U[(size_t)(k + 1) * n + k] / U[(size_t)k * n + k];
    lm[k] = f;
    U[(size_t)(k + 1) * n + k] = 0.0L;
    for (int j = k + 1; j < n; j++) U[(size_t)(k + 1) * n + j] -= f * U[(size_t)k * n + j];
  }
  if (U[(size_t)(n - 1) * n + n - 1] == 0.0L) U[(size_t)(n - 1) * n + n - 1] = tiny;
  y.assign(n, 1.0L);
  for (int it = 0; it < 3; it++) {
    for (int k = 0; k + 1 < n; k++) {                     // L
      if (swp[k]) std::swap(y[k], y[k + 1]);
      y[k + 1] -= lm[k] * y[k];
    }
    for (int i = n - 1; i >= 0; i--) {                    // U
      long double s = y[i];
      for (int j = i + 1; j < n; j++) s -= U[(size_t)i * n + j] * y[j];
      y[i] = s / U[(size_t)i * n + i];
    }
    long double mx = 0.0L;
    for (int i = 0; i < n; i++) mx = std::max(mx, fabsl(y[i]));
    if (!(mx > 0.0L) || !std::isfinite((double)mx)) return;
    for (int i = 0; i < n; i++) y[i] /= mx;
  }
}

// In-place inverse of a dense n x n matrix (LU with partial pivoting); false if singular
bool invert(int n, LVec &A) {
  LVec inv((size_t)n * n, 0.0L);
  for (int i = 0; i < n; i++) inv[(size_t)i * n + i] = 1.0L;
  for (int k = 0; k < n; k++) {
    int piv = k;
    for (int i = k + 1; i < n; i++) if (fabsl(A[(size_t)i * n + k]) > fabsl(A[(size_t)piv * n + k])) piv = i;
    if (A[(size_t)piv * n + k] == 0.0L) return false;
    if (piv != k)
      for (int j = 0; j < n; j++) { std::swap(A[(size_t)k * n + j], A[(size_t)piv * n + j]); std::swap(inv[(size_t)k * n + j], inv[(size_t)piv * n + j]); }
    const long double d = A[(size_t)k * n + k];
    for (int i = 0; i < n; i++) {
      if (i == k) continue;
      const long double f = A[(size_t)i * n + k] / d;
      if (f == 0.0L) continue;
      for (int j = 0; j < n; j++) { A[(size_t)i * n + j] -= f * A[(size_t)k * n + j]; inv[(size_t)i * n + j] -= f * inv[(size_t)k * n + j]; }
    }
    for (int j = 0; j < n; j++) { A[(size_t)k * n + j] /= d; inv[(size_t)k * n + j] /= d; }
  }
  A.swap(inv);
  return true;
}

// Real eigenvalues (ascending) and eigenvectors (columns of V, row-major n x n) of a dense real matrix A whose spectrum is
// real and simple; false on complex or repeated eigenvalues or if the QR iteration does not converge
bool eig_real_simple(int n, const LVec &A0, LVec &lam, LVec &V) {
  LVec A = A0, scale, Q, wr, wi;
  balance(n, A, scale);
  hessenberg(n, A, Q);
  long double hnorm = 0.0L;
  for (int i = 0; i < n; i++) for (int j = std::max(i - 1, 0); j < n; j++) hnorm = std::max(hnorm, fabsl(A[(size_t)i * n + j]));
  if (!hqr(n, A, wr, wi)) return false;
  for (int i = 0; i < n; i++) if (wi[i] != 0.0L) return false;
  std::sort(wr.begin(), wr.end());
  for (int i = 0; i + 1 < n; i++)                       // (a gap of a few thousand rounding units of |H|: not distinguishable)
    if (wr[i + 1] - wr[i] <= 1e-15L * hnorm) return false;
  lam = wr;
  V.assign((size_t)n * n, 0.0L);
  LVec y;
  for (int q = 0; q < n; q++) {
    hess_inverse_iteration(n, A, lam[q], hnorm, y);
    for (int i = 0; i < n; i++) {                       // x = D Q y
      long double s = 0.0L;
      for (int j = 0; j < n; j++) s += Q[(size_t)i * n + j] * y[j];
      V[(size_t)i * n + q] = scale[i] * s;
    }
  }
  for (size_t i = 0; i < V.size(); i++) if (!std::isfinite((double)V[i])) return false;
  return true;
}

// S, S^-1, lam of a centro-symmetric M x M matrix A in the parity mode layout (spec_line's; see above)
static bool parity_eig(int M, const LVec &A, LVec &S, LVec &Sinv, LVec &lam) {
  const int m = M - 1, He = (M + 1) / 2, Ho = M / 2;
  const bool has_mid = (M & 1) != 0;
  S.assign((size_t)M * M, 0.0L); Sinv.assign((size_t)M * M, 0.0L);
  lam.assign(M, 0.0L);
  for (int parity = 0; parity < 2; parity++) {            // 0: even, 1: odd
    const int h = parity == 0 ? He : Ho;
    if (h == 0) continue;
    const long double sg = parity == 0 ? 1.0L : -1.0L;
    LVec Ah((size_t)h * h), lh, V;
    for (int i = 0; i < h; i++)
      for (int j = 0; j < h; j++)
        Ah[(size_t)i * h + j] = (has_mid && parity == 0 && j == h - 1) ? A[(size_t)i * M + j] : A[(size_t)i * M + j] + sg * A[(size_t)i * M + (m - j)];
    if (!eig_real_simple(h, Ah, lh, V)) return false;
    // columns normalised as full-line vectors: the half coordinate i < h stands for two points (one: the middle point)
    for (int q = 0; q < h; q++) {
      long double nrm = 0.0L;
      for (int i = 0; i < h; i++) nrm += ((has_mid && parity == 0 && i == h - 1) ? 1.0L : 2.0L) * V[(size_t)i * h + q] * V[(size_t)i * h + q];
      nrm = sqrtl(nrm);
      // sign: the largest component positive (a deterministic choice)
      int im = 0;
      for (int i = 1; i < h; i++) if (fabsl(V[(size_t)i * h + q]) > fabsl(V[(size_t)im * h + q])) im = i;
      if (V[(size_t)im * h + q] < 0) nrm = -nrm;
      for (int i = 0; i < h; i++) V[(size_t)i * h + q] /= nrm;
    }
    LVec Vi = V;
    if (!invert(h, Vi)) return false;
    for (int q = 0; q < h; q++) {
      const int pos = parity == 0 ? q : m - q;
      lam[pos] = lh[q];
      for (int i = 0; i < h; i++) {
        const long double v = V[(size_t)i * h + q];
        const bool mid = has_mid && parity == 0 && i == h - 1;
        // S^-1 S = I with rows of the same parity: the half-coordinate inverse, halved where a coordinate stands for two points
        const long double r = mid ? Vi[(size_t)q * h + i] : 0.5L * Vi[(size_t)q * h + i];
        S[(size_t)i * M + pos] = v;
        Sinv[(size_t)pos * M + i] = r;
        if (!mid) { S[(size_t)(m - i) * M + pos] = sg * v; Sinv[(size_t)pos * M + (m - i)] = sg * r; }
      }
    }
  }
  return true;
}

}  // namespace

bool spec_line(int P, std::vector<long double> &S, std::vector<long double> &Sinv, std::vector<long double> &lam) {
  const int n = P - 1, M = P - 2;
  if (M < 1) return false;
  std::vector<long double> D((size_t)P * P), A((size_t)M * M);
  for (int i = 0; i < P; i++) for (int j = 0; j < P; j++) D[(size_t)i * P + j] = dentry(i, j, n);
  for (int i = 0; i < M; i++)
    for (int j = 0; j < M; j++) {
      long double s = 0.0L;
      for (int q = 0; q < P; q++) s += D[(size_t)(i + 1) * P + q] * D[(size_t)q * P + (j + 1)];
      A[(size_t)i * M + j] = -s;
    }
  return parity_eig(M, A, S, Sinv, lam);
}

// ---------------------------------------------------------------------------------------------
// The same line operator with a Neumann or Robin condition at either end (cheb_helmholtz_create_bc).  End e of the line gets
// alpha_e u + beta_e du/dnu = g_e with du/dnu the outward derivative (+D at index 0, -D at index n); its collocation row
//     B_row = [alpha_0 e_0 + beta_0 D_0 ; alpha_1 e_n - beta_1 D_n]          (2 x P)
// gives the end values from the interior ones, u_B = Q u_I + B_BB^-1 g with Q = -B_BB^-1 B_BI, and eliminating them from
// -(D D) u at the interior nodes leaves  A~ = -(DD)_II - (DD)_IB Q  and the lift  L = (DD)_IB B_BB^-1  of the boundary data.
// Equal ends: A~ is centro-symmetric and goes through the parity split above (the raw transforms and the one-launch z solve stay
// usable).  Different ends: one dense eigenproblem, modes by ascending eigenvalue (parity = false).  A Neumann/Neumann line has
// the constants as its null space: that eigenvalue is set to exactly 0, which is what the solve's singular-mode test looks for.
// ---------------------------------------------------------------------------------------------
int spec_line_bc(int P, const double *bc4, std::vector<long double> &S, std::vector<long double> &Sinv, std::vector<long double> &lam,
                 std::vector<long double> &Q, std::vector<long double> &L, std::vector<long double> &Binv, bool &parity) {
  if (P < 3) return SPEC_BC_SIZE;
  for (int e = 0; e < 2; e++) {
    const double a = bc4[2 * e], b = bc4[2 * e + 1];
    if (!std::isfinite(a) || !std::isfinite(b) || a < 0.0 || b < 0.0 || (a == 0.0 && b == 0.0)) return SPEC_BC_COND;
  }
  const int n = P - 1, M = P - 2;
  const long double a0 = bc4[0], b0 = bc4[1], a1 = bc4[2], b1 = bc4[3];
  const bool dirichlet = bc4[0] == 1.0 && bc4[1] == 0.0 && bc4[2] == 1.0 && bc4[3] == 0.0;
  parity = bc4[0] == bc4[2] && bc4[1] == bc4[3];
  LVec D((size_t)P * P), DD((size_t)P * P), Br((size_t)2 * P);
  for (int i = 0; i < P; i++) for (int j = 0; j < P; j++) D[(size_t)i * P + j] = dentry(i, j, n);
  for (int i = 0; i < P; i++)
    for (int j = 0; j < P; j++) {
      long double s = 0.0L;
      for (int q = 0; q < P; q++) s += D[(size_t)i * P + q] * D[(size_t)q * P + j];
      DD[(size_t)i * P + j] = s;
    }
  for (int j = 0; j < P; j++) {
    Br[j] = (j == 0 ? a0 : 0.0L) + b0 * D[j];
    Br[(size_t)P + j] = (j == n ? a1 : 0.0L) - b1 * D[(size_t)n * P + j];
  }
  const long double b00 = Br[0], b01 = Br[n], b10 = Br[P], b11 = Br[(size_t)P + n], det = b00 * b11 - b01 * b10;
  if (!(det != 0.0L) || !std::isfinite((double)det)) return SPEC_BC_SINGULAR;
  Binv.assign(4, 0.0L);
  Binv[0] = b11 / det; Binv[1] = -b01 / det; Binv[2] = -b10 / det; Binv[3] = b00 / det;
  if (dirichlet) { Binv[0] = 1.0L; Binv[1] = 0.0L; Binv[2] = 0.0L; Binv[3] = 1.0L; }
  Q.assign((size_t)2 * M, 0.0L); L.assign((size_t)M * 2, 0.0L);
  for (int e = 0; e < 2; e++)
    for (int j = 0; j < M; j++) if (!dirichlet) Q[(size_t)e * M + j] = -(Binv[2 * e] * Br[j + 1] + Binv[2 * e + 1] * Br[(size_t)P + j + 1]);
  for (int i = 0; i < M; i++)
    for (int e = 0; e < 2; e++) L[(size_t)i * 2 + e] = DD[(size_t)(i + 1) * P] * Binv[e] + DD[(size_t)(i + 1) * P + n] * Binv[2 + e];
  if (dirichlet) return spec_line(P, S, Sinv, lam) ? 0 : SPEC_BC_EIG;       // Q = 0, A~ = A_1: spec_line's matrices, bit for bit
  LVec A((size_t)M * M);
  for (int i = 0; i < M; i++)
    for (int j = 0; j < M; j++)
      A[(size_t)i * M + j] = -DD[(size_t)(i + 1) * P + j + 1] - (DD[(size_t)(i + 1) * P] * Q[j] + DD[(size_t)(i + 1) * P + n] * Q[(size_t)M + j]);
  if (parity) {
    if (!parity_eig(M, A, S, Sinv, lam)) return SPEC_BC_EIG;
  } else {
    LVec V;
    if (!eig_real_simple(M, A, lam, V)) return SPEC_BC_EIG;
    for (int q = 0; q < M; q++) {                        // unit columns, the largest component positive (as spec_line)
      long double nrm = 0.0L;
      int im = 0;
      for (int i = 0; i < M; i++) { nrm += V[(size_t)i * M + q] * V[(size_t)i * M + q]; if (fabsl(V[(size_t)i * M + q]) > fabsl(V[(size_t)im * M + q])) im = i; }
      nrm = sqrtl(nrm);
      if (V[(size_t)im * M + q] < 0) nrm = -nrm;
      for (int i = 0; i < M; i++) V[(size_t)i * M + q] /= nrm;
    }
    Sinv = V;
    if (!invert(M, Sinv)) return SPEC_BC_EIG;
    S.swap(V);
  }
  if (bc4[0] == 0.0 && bc4[2] == 0.0) {                  // Neumann / Neumann: the constant mode, eigenvalue exactly 0
    int iz = 0;
    for (int i = 1; i < M; i++) if (fabsl(lam[i]) < fabsl(lam[iz])) iz = i;
    long double lmax = 0.0L;
    for (int i = 0; i < M; i++) lmax = std::max(lmax, fabsl(lam[i]));
    if (fabsl(lam[iz]) > 1e-10L * (lmax > 1.0L ? lmax : 1.0L)) return SPEC_BC_EIG;
    lam[iz] = 0.0L;
  }
  return 0;
}

// centro-symmetric (part = 1) or centro-antisymmetric (part = 0) part of a dense M x M matrix
void centro_part(int M, const std::vector<long double> &A, int part, std::vector<long double> &out) {
  out.resize((size_t)M * M);
  const int m = M - 1;
  for (int i = 0; i < M; i++)
    for (int j = 0; j < M; j++) {
      const long double a = A[(size_t)i * M + j], b = A[(size_t)(m - i) * M + (m - j)];
      out[(size_t)i * M + j] = part ? 0.5L * (a + b) : 0.5L * (a - b);
    }
}

// Lagrange interpolation matrix between two node sets of Chebyshev-Gauss-Lobatto grids (cheb_resample_*, resample.hip):
// R[t][s] (n_out stored rows x n_in stored columns, row-major) maps the values at the stored input nodes to the stored output
// nodes.  Stored node s of a grid of n points is grid index j = s (all nodes) or j = s + 1 (interior: j = 1 .. n-2), angle
// pi j / (n-1).  Generic barycentric weights w_j = 1 / prod_{k != j} (x_j - x_k) over the stored set, second barycentric form;
// every difference of two nodes is formed from the angles (cos a - cos b = -2 sin((a+b)/2) sin((a-b)/2), the half-angles as
// exact integer ratios), so the nodes never lose digits to cancellation.  A row whose output node IS an input node (angle
// indices i (n_in-1) == j (n_out-1), decided in integers) is an exact unit row: equal grids give I, and coarse values are
// injected unchanged into a finer grid that contains their nodes.
// (the rows in long double: resample_matrix_host rounds them once, dealias_matrix_host multiplies them by D first)
static void resample_rows_ld(int n_in, int in_interior, int n_out, int out_interior, long double *R) {
  const int a_in = in_interior ? 1 : 0, a_out = out_interior ? 1 : 0;
  const int K = n_in - 2 * a_in, M = n_out - 2 * a_out;
  const long ni = n_in - 1, no = n_out - 1;
  // x_{i on grid of (m+1) points} - x_{j on grid of (n+1) points}, m, n = intervals
  auto diff = [](long i, long m, long j, long n) -> long double {
    const long double den = 2.0L * (long double)m * (long double)n;
    const long sum = i * n + j * m, dif = i * n - j * m;
    return -2.0L * sinl(PI_L * (long double)sum / den) * sinl(PI_L * (long double)dif / den);
  };
  std::vector<long double> w(K);
  for (int s = 0; s < K; s++) {
    long double prod = 1.0L;
    for (int k = 0; k < K; k++)
      if (k != s) prod *= diff(s + a_in, ni, k + a_in, ni);
    w[s] = 1.0L / prod;
  }
  std::vector<long double> c(K);
  for (int t = 0; t < M; t++) {
    const long i = t + a_out;
    long double *row = R + (size_t)t * K;
    int hit = -1;
    for (int s = 0; s < K && hit < 0; s++)
      if (i * ni == (long)(s + a_in) * no) hit = s;
    if (hit >= 0) {
      for (int s = 0; s < K; s++) row[s] = s == hit ? 1.0L : 0.0L;
      continue;
    }
    long double sum = 0.0L;
    for (int s = 0; s < K; s++) { c[s] = w[s] / diff(i, no, s + a_in, ni); sum += c[s]; }
    for (int s = 0; s < K; s++) row[s] = c[s] / sum;
  }
}

void resample_matrix_host(int n_in, int in_interior, int n_out, int out_interior, double *R) {
  const size_t K = n_in - (in_interior ? 2 : 0), M = n_out - (out_interior ? 2 : 0);
  std::vector<long double> Rl(M * K);
  resample_rows_ld(n_in, in_interior, n_out, out_interior, Rl.data());
  for (size_t e = 0; e < M * K; e++) R[e] = (double)Rl[e];
}

// Chebyshev coefficient transforms on the n = N + 1 Gauss-Lobatto nodes (cheb_modal_*, modal.hip), c_0 = c_N = 2, otherwise 1:
//   backward  B[j][k] = T_k(x_j) = cos(pi j k / N)                       (coefficients -> values)
//   forward   T[k][j] = 2 / (N c_k c_j) cos(pi j k / N)                  (values -> coefficients),  B T = I
//   weights   w = I^T T,  I_k = 2 / (1 - k^2) for even k, 0 for odd k     (Clenshaw-Curtis: exact up to degree N, sum w = 2)
//   filter    F = B diag(sigma) T
// The cosine: j k is reduced modulo 2N in integers and folded into 0 .. N (cos is even and 2 pi-periodic), then
// cos(pi r / N) = sin(pi (N - 2r) / 2N) with the argument in [-pi/2, pi/2] -- unreduced, PI_L's own rounding error times j k makes
// the entries of a 1024-point matrix wrong in the 14th digit.  2 j k an odd multiple of N gives N - 2r = 0: an exact 0.
static long double cos_jk(long j, long k, long N) {
  long r = (j * k) % (2 * N);
  if (r > N) r = 2 * N - r;
  const long m = N - 2 * r;
  if (m == 0) return 0.0L;
  if (m == N) return 1.0L;
  if (m == -N) return -1.0L;
  const long double s = sinl(PI_L * (long double)(m < 0 ? -m : m) / (2.0L * (long double)N));
  return m < 0 ? -s : s;
}

static long double modal_entry(int n, int which, int row, int col) {
  const long N = n - 1;
  if (which) return cos_jk(row, col, N);                                     // B[j = row][k = col]
  const long double ck = (row == 0 || row == N) ? 2.0L : 1.0L, cj = (col == 0 || col == N) ? 2.0L : 1.0L;
  return 2.0L / ((long double)N * ck * cj) * cos_jk(col, row, N);            // T[k = row][j = col]
}

void modal_matrix_host(int n, int which, double *M) {
  for (int r = 0; r < n; r++)
    for (int c = 0; c < n; c++) M[(size_t)r * n + c] = (double)modal_entry(n, which, r, c);
}

void modal_weights_host(int n, double *w) {
  for (int j = 0; j < n; j++) {
    long double s = 0.0L;
    for (int k = 0; k < n; k += 2) s += 2.0L / (1.0L - (long double)k * k) * modal_entry(n, 0, k, j);
    w[j] = (double)s;
  }
}

// sigma all ones: the identity, exactly; modes with sigma = 0 are skipped
void modal_filter_matrix_host(int n, const double *sigma, double *F) {
  bool ones = true;
  for (int k = 0; k < n; k++) ones = ones && sigma[k] == 1.0;
  if (ones) {
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) F[(size_t)i * n + j] = i == j ? 1.0 : 0.0;
    return;
  }
  std::vector<int> act;
  for (int k = 0; k < n; k++) if (sigma[k] != 0.0) act.push_back(k);
  const size_t na = act.size();
  std::vector<long double> Bs((size_t)n * na), Tt((size_t)n * na), acc(n);     // B[i][k] sigma_k and T[k][j] as [j][k], active k only
  for (int i = 0; i < n; i++)
    for (size_t a = 0; a < na; a++) {
      Bs[(size_t)i * na + a] = modal_entry(n, 1, i, act[a]) * (long double)sigma[act[a]];
      Tt[(size_t)i * na + a] = modal_entry(n, 0, act[a], i);
    }
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      const long double *b = &Bs[(size_t)i * na], *t = &Tt[(size_t)j * na];
      long double s = 0.0L;
      for (size_t a = 0; a < na; a++) s += b[a] * t[a];
      F[(size_t)i * n + j] = (double)s;
    }
}

// Dealiased products (cheb_dealias_*, dealias.hip): n coarse and m >= n fine points of one direction, N = n - 1, M = m - 1.
//   which = 0  R (m x n): resample_matrix_host(n, m), bit for bit
//   which = 1  P (n x m) = B_n T_m[0:n, :]: fine values -> fine coefficients, modes 0 .. N kept, evaluated at the coarse nodes
//              (m == n: B T = I, written as the exact identity)
//   which = 2  G (m x n) = R D_n: differentiate on the coarse grid and interpolate, one matrix
// For M > 3N/2 the aliases of the modes M < k <= 2N of a product of two degree-N interpolants land at 2M - k > N, which P drops:
// P ((R u) o (R v)) is then the exact degree-N truncation of the product.  The smallest such m is ceil(3n/2).
int dealias_fine_size(int n) { return (3 * n + 1) / 2; }

void dealias_matrix_host(int n, int m, int which, double *A) {
  if (which == 0) { resample_matrix_host(n, 0, m, 0, A); return; }
  const size_t sn = n, sm = m;
  if (which == 1) {
    if (m == n) {
      for (size_t i = 0; i < sn; i++)
        for (size_t j = 0; j < sn; j++) A[i * sn + j] = i == j ? 1.0 : 0.0;
      return;
    }
    std::vector<long double> B(sn * sn), Tt(sm * sn);                         // B_n[i][k]; T_m[k][j] as [j][k], k < n
    for (int i = 0; i < n; i++)
      for (int k = 0; k < n; k++) B[i * sn + k] = modal_entry(n, 1, i, k);
    for (int j = 0; j < m; j++)
      for (int k = 0; k < n; k++) Tt[j * sn + k] = modal_entry(m, 0, k, j);
    for (size_t i = 0; i < sn; i++)
      for (size_t j = 0; j < sm; j++) {
        const long double *b = &B[i * sn], *t = &Tt[j * sn];
        long double s = 0.0L;
        for (size_t k = 0; k < sn; k++) s += b[k] * t[k];
        A[i * sm + j] = (double)s;
      }
    return;
  }
  std::vector<long double> R(sm * sn), Dt(sn * sn);                           // D_n as [j][s]
  resample_rows_ld(n, 0, m, 0, R.data());
  for (int s = 0; s < n; s++)
    for (int j = 0; j < n; j++) Dt[j * sn + s] = dentry(s, j, n - 1);
  for (size_t i = 0; i < sm; i++)
    for (size_t j = 0; j < sn; j++) {
      const long double *r = &R[i * sn], *dd = &Dt[j * sn];
      long double s = 0.0L;
      for (size_t k = 0; k < sn; k++) s += r[k] * dd[k];
      A[i * sn + j] = (double)s;
    }
}

// Evaluation at arbitrary points (cheb_points_*, points.hip).  The node table x_j = cos(pi j / N) comes from cos_jk, so x_0 = 1,
// x_N = -1, x_j = -x_{N-j} and the middle node of an odd n are exact.
void points_nodes_host(int n, double *x) {
  for (int j = 0; j < n; j++) x[j] = (double)cos_jk(j, 1, n - 1);
}

// Node spacings (cheb_stats_*, stats.hip).  The gap between the nodes j and j + 1 of n = N + 1 points is
//   x_j - x_{j+1} = cos(pi j / N) - cos(pi (j + 1) / N) = 2 sin(pi (2j + 1) / 2N) sin(pi / 2N),
// a product, so nothing cancels next to the walls, where the gaps are of the order N^-2.  2j + 1 is folded into 1 .. N in integers
// (sin(pi - t) = sin t): both arguments lie in (0, pi/2].  h_j = the smaller of the gaps on either side of node j, the one gap
// there is at j = 0 and j = N.  The gaps are symmetric, gap_j = gap_{N-1-j}, exactly.
static long double stats_gap(long j, long N) {
  long m = 2 * j + 1;
  if (m > N) m = 2 * N - m;
  return 2.0L * sinl(PI_L * (long double)m / (2.0L * (long double)N)) * sinl(PI_L / (2.0L * (long double)N));
}

static long double stats_spacing_ld(int j, int n) {
  const long N = n - 1;
  if (j == 0) return stats_gap(0, N);
  if (j == N) return stats_gap(N - 1, N);
  const long double a = stats_gap(j - 1, N), b = stats_gap(j, N);
  return a < b ? a : b;
}

void stats_spacing_host(int n, double *h) {
  for (int j = 0; j < n; j++) h[j] = (double)stats_spacing_ld(j, n);
}

// r_j = s / h_j: the quotient in long double, rounded once
void stats_rate_host(int n, double s, double *r) {
  for (int j = 0; j < n; j++) r[j] = (double)((long double)s / stats_spacing_ld(j, n));
}

// Row of a coordinate x: l_j = (w_j / (x - x_j)) / sum_k w_k / (x - x_k), w_j = (-1)^j, halved at both ends, in the nearest-node
// form: s = the node nearest to x (the lowest index on a tie), d_j = x - x_j, r_s = 1, r_j = (w_j / w_s) (d_s / d_j) otherwise
// (|d_s / d_j| <= 1: nothing overflows), l = r / sum r, the sum in ascending j.  w_j / w_s is +-1/2, +-1 or +-2, so an entry
// costs one rounding for d_j, one for the quotient and one for the division by the sum.  d_s == 0: the exact unit row; a NaN or
// infinite coordinate: a row of NaN; |x| > 1 extrapolates by the same formula.  Long double on the DOUBLE node table (the
// polynomial the device interpolates is the one through the rounded nodes), rounded once.
// the row of one finite coordinate in long double, before the rounding
static void points_row_ld(int n, const double *xn, double x, long double *l) {
  const int N = n - 1;
  const long double xt = x;
  int s = 0;
  long double best = fabsl(xt - (long double)xn[0]);
  for (int j = 1; j < n; j++) { const long double a = fabsl(xt - (long double)xn[j]); if (a < best) { best = a; s = j; } }
  const long double ds = xt - (long double)xn[s];
  if (ds == 0.0L) { for (int j = 0; j < n; j++) l[j] = j == s ? 1.0L : 0.0L; return; }
  const long double hs = (s == 0 || s == N) ? 0.5L : 1.0L;
  long double sum = 0.0L;
  for (int j = 0; j < n; j++) {
    if (j == s) l[j] = 1.0L;
    else {
      const long double hj = (j == 0 || j == N) ? 0.5L : 1.0L;
      l[j] = (((j - s) & 1) ? -hj : hj) / hs * (ds / (xt - (long double)xn[j]));
    }
    sum += l[j];
  }
  for (int j = 0; j < n; j++) l[j] = l[j] / sum;
}

void points_matrix_host(int n, int m, const double *x, double *R) {
  std::vector<double> xn(n);
  points_nodes_host(n, xn.data());
  std::vector<long double> r(n);
  for (int t = 0; t < m; t++) {
    double *row = R + (size_t)t * n;
    if (!std::isfinite(x[t])) { for (int j = 0; j < n; j++) row[j] = std::numeric_limits<double>::quiet_NaN(); continue; }
    points_row_ld(n, xn.data(), x[t], r.data());
    for (int j = 0; j < n; j++) row[j] = (double)r[j];
  }
}

// Rows of the interpolant's derivative, l'_j(x) = d l_j / dx (cheb_points_dmatrix_host; the device twin is k_points_rows where it writes derivative rows).  With
// c_j = w_j / w_s, q_j = c_j / d_j, r_j = q_j d_s (j != s), R = 1 + sum r_j, Q2 = sum q_k / d_k, T = sum q_k (x_s - x_k) / d_k, the
// sums over k != s in ascending k:
//   l'_j = (q_j / R) ((1 + d_s^2 Q2) / R - d_s / d_j)   (j != s),     l'_s = -T / R^2
// the exact derivative of the rational function points_row_ld evaluates.  Nothing divides by d_s; d_s == 0 gives l'_j = q_j,
// l'_s = -sum q_k, a row of the differentiation matrix on the double nodes.  Long double on the DOUBLE node table, rounded once;
// a NaN or infinite coordinate: a row of NaN.
void points_dmatrix_host(int n, int m, const double *x, double *R) {
  const int N = n - 1;
  std::vector<double> xn(n);
  points_nodes_host(n, xn.data());
  std::vector<long double> q(n);
  for (int t = 0; t < m; t++) {
    double *row = R + (size_t)t * n;
    if (!std::isfinite(x[t])) { for (int j = 0; j < n; j++) row[j] = std::numeric_limits<double>::quiet_NaN(); continue; }
    const long double xt = x[t];
    int s = 0;
    long double best = fabsl(xt - (long double)xn[0]);
    for (int j = 1; j < n; j++) { const long double a = fabsl(xt - (long double)xn[j]); if (a < best) { best = a; s = j; } }
    const long double xs = xn[s], ds = xt - xs, hs = (s == 0 || s == N) ? 0.5L : 1.0L;
    long double Rs = 0.0L, Q2 = 0.0L, T = 0.0L;
    for (int j = 0; j < n; j++) {
      if (j == s) continue;
      const long double hj = (j == 0 || j == N) ? 0.5L : 1.0L, dj = xt - (long double)xn[j];
      q[j] = (((j - s) & 1) ? -hj : hj) / hs / dj;
      Rs += q[j] * ds;
      Q2 += q[j] / dj;
      T += q[j] * (xs - (long double)xn[j]) / dj;
    }
    Rs = 1.0L + Rs;
    const long double g0 = (1.0L + ds * ds * Q2) / Rs;
    for (int j = 0; j < n; j++)
      row[j] = j == s ? (double)(-T / (Rs * Rs)) : (double)(q[j] / Rs * (g0 - ds / (xt - (long double)xn[j])));
  }
}

// Weight vectors of the partial contractions (cheb_reduce_*, reduce.hip): what one contracted direction of n points is summed
// against.  INTEGRAL: modal_weights_host; MEAN: half of it (the interval has length 2; the halving is exact); NODE j: the unit
// vector e_j; DNODE j: row j of D_n; POINT x: the row of points_matrix_host; DPOINT x: r(x)^T D_n, r the long double row on the
// double node table, the product formed before the one rounding (as G in dealias_matrix_host).  Returns 0, 1 (kind) or 2 (j).
int reduce_weights_host(int n, int kind, double arg, double *w) {
  if (kind == REDUCE_W_INTEGRAL) { modal_weights_host(n, w); return 0; }
  if (kind == REDUCE_W_MEAN) {
    for (int j = 0; j < n; j++) {
      long double s = 0.0L;
      for (int k = 0; k < n; k += 2) s += 2.0L / (1.0L - (long double)k * k) * modal_entry(n, 0, k, j);
      w[j] = (double)(0.5L * s);
    }
    return 0;
  }
  if (kind == REDUCE_W_NODE || kind == REDUCE_W_DNODE) {
    if (!(arg >= 0.0 && arg <= (double)(n - 1)) || arg != (double)(int)arg) return 2;
    const int i = (int)arg;
    for (int j = 0; j < n; j++) w[j] = kind == REDUCE_W_NODE ? (j == i ? 1.0 : 0.0) : (double)dentry(i, j, n - 1);
    return 0;
  }
  if (kind == REDUCE_W_POINT) { points_matrix_host(n, 1, &arg, w); return 0; }
  if (kind == REDUCE_W_DPOINT) {
    if (!std::isfinite(arg)) { for (int j = 0; j < n; j++) w[j] = std::numeric_limits<double>::quiet_NaN(); return 0; }
    std::vector<double> xn(n);
    points_nodes_host(n, xn.data());
    std::vector<long double> r(n);
    points_row_ld(n, xn.data(), arg, r.data());
    for (int k = 0; k < n; k++) {
      long double s = 0.0L;
      for (int j = 0; j < n; j++) s += r[j] * dentry(j, k, n - 1);
      w[k] = (double)s;
    }
    return 0;
  }
  return 1;
}

// ---------------------------------------------------------------------------------------------
// Periodic (Fourier) directions.  n nodes x_j = -1 + 2 j / n, j = 0 .. n-1, period 2, no duplicated end point.
//   D_F = pi D_theta, theta = pi (x + 1):  D_theta[i][j] = 1/2 (-1)^(i-j) cot(pi (i-j) / n)  (n even),
//                                                          1/2 (-1)^(i-j) / sin(pi (i-j) / n) (n odd),   zero diagonal.
// D_F is circulant and odd, hence centro-antisymmetric; for even n it annihilates the Nyquist vector (-1)^j.  The second
// derivative is D_F D_F (long double, rounded once: the convention of diffmat_create_dd, not the textbook D^(2), which differs at
// the Nyquist mode), centro-symmetric.  Every sine / cosine takes its argument as an integer multiple of pi / n reduced in
// integers and folded into [0, pi/2], as sin_half above.
// ---------------------------------------------------------------------------------------------
// sin(pi m / n), any integer m
static long double sin_pi(long m, long n) {
  long r = m % (2 * n);
  if (r < 0) r += 2 * n;
  long double sg = 1.0L;
  if (r >= n) { r -= n; sg = -1.0L; }
  if (2 * r > n) r = n - r;
  if (r == 0) return 0.0L;
  if (2 * r == n) return sg;
  return sg * sinl(PI_L * (long double)r / (long double)n);
}
static long double cos_pi(long m, long n) { return sin_pi(2 * m + n, 2 * n); }

static long double fourier_dentry(int i, int j, int n) {
  if (i == j) return 0.0L;
  const long m = i - j;
  const long double sg = (m & 1) ? -1.0L : 1.0L, s = sin_pi(m, n);
  return PI_L * 0.5L * sg * ((n & 1) ? 1.0L / s : cos_pi(m, n) / s);
}

void fourier_nodes_host(int n, double *x) {
  for (int j = 0; j < n; j++) x[j] = (double)((long double)(2 * j - n) / (long double)n);
}

void fourier_diff_ld(int n, int order, std::vector<long double> &A) {
  std::vector<long double> D((size_t)n * n);
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) D[(size_t)i * n + j] = fourier_dentry(i, j, n);
  if (order == 1) { A.swap(D); return; }
  A.assign((size_t)n * n, 0.0L);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      long double s = 0.0L;
      for (int q = 0; q < n; q++) s += D[(size_t)i * n + q] * D[(size_t)q * n + j];
      A[(size_t)i * n + j] = s;
    }
}

// Position -> mode in spec_line's parity layout, the flip j -> n-1-j reflecting about c = -1/n: the even modes at p < ceil(n/2) are
// the constant (p = 0) and cos(pi k (x - c)) at p = k; the odd ones at n-1-q are, for even n, the Nyquist vector (q = 0) and
// sin(pi k (x - c)) at q = k, for odd n sin at q = k - 1; 1 <= k <= floor((n-1)/2).  kind: 0 cos (k = 0: the constant), 1 sin,
// 2 Nyquist (k = n / 2).
void fourier_modes_host(int n, int *k, int *kind) {
  const int K = (n - 1) / 2;
  k[0] = 0; kind[0] = 0;
  for (int q = 1; q <= K; q++) { k[q] = q; kind[q] = 0; }
  if (!(n & 1)) { k[n - 1] = n / 2; kind[n - 1] = 2; }
  for (int q = 1; q <= K; q++) { const int pos = (n & 1) ? n - q : n - 1 - q; k[pos] = q; kind[pos] = 1; }
}

// B (which = 1: values <- coefficients; column p holds mode p with amplitude 1, so the constant's coefficient is the mean) or its
// inverse T (which = 0: row p = mode p times 1/n for the constant and the Nyquist vector, 2/n otherwise).  Entries of half a line,
// mirrored with the mode's sign: every column of B and every row of T carries its parity exactly.
void fourier_modal_ld(int n, int which, std::vector<long double> &M) {
  std::vector<int> k(n), kind(n);
  fourier_modes_host(n, k.data(), kind.data());
  M.assign((size_t)n * n, 0.0L);
  const int H = (n + 1) / 2;
  for (int p = 0; p < n; p++) {
    const long double sg = kind[p] == 0 ? 1.0L : -1.0L;
    const long double w = which ? 1.0L : ((kind[p] == 2 || k[p] == 0) ? 1.0L : 2.0L) / (long double)n;
    for (int j = 0; j < H; j++) {
      long double v;
      if (kind[p] == 2) v = (j & 1) ? -1.0L : 1.0L;
      else if (kind[p] == 0) v = cos_pi((long)k[p] * (2 * j + 1 - n), n);
      else v = sin_pi((long)k[p] * (2 * j + 1 - n), n);
      v *= w;
      const int jm = n - 1 - j;
      if (which) { M[(size_t)j * n + p] = v; M[(size_t)jm * n + p] = jm == j ? v : sg * v; }
      else { M[(size_t)p * n + j] = v; M[(size_t)p * n + jm] = jm == j ? v : sg * v; }
    }
  }
}

// The line of the solve: A_1 = -s^2 D_F D_F on all n points = S diag(lam) S^-1 in closed form, S = B and S^-1 = T above,
// lam = s^2 (pi k)^2; the constant's and the Nyquist vector's eigenvalue is exactly 0.  No eigensolver runs.
void fourier_line(int n, double s, std::vector<long double> &S, std::vector<long double> &Sinv, std::vector<long double> &lam) {
  std::vector<int> k(n), kind(n);
  fourier_modes_host(n, k.data(), kind.data());
  fourier_modal_ld(n, 1, S);
  fourier_modal_ld(n, 0, Sinv);
  lam.assign(n, 0.0L);
  for (int p = 0; p < n; p++)
    if (kind[p] != 2 && k[p] != 0) { const long double a = PI_L * (long double)k[p] * (long double)s; lam[p] = a * a; }
}

// Dealiased products on a periodic direction (cheb_dealias_create_basis): n coarse nodes x_j = -1 + 2 j / n, m >= n fine
// nodes y_i = -1 + 2 i / m, K = floor(n / 2).  The interpolant of n periodic values is sum_j u_j r_j(x),
//   r_j(x) = (1/n) [1 + 2 sum_{k=1}^{K} cos pi k (x - x_j)]                              (n odd)
//   r_j(x) = (1/n) [1 + 2 sum_{k=1}^{K-1} cos pi k (x - x_j) + cos pi K (x - x_j)]       (n even: the Nyquist vector is cos pi K (x + 1))
//   which = 0  R (m x n): R[i][j] = r_j(y_i); a fine node that is a coarse node gives the exact unit row
//   which = 1  P (n x m): P[i][j] = (1/m) [1 + 2 sum_{k=1}^{K} cos pi k (x_i - y_j)], the fine-grid function's Fourier series cut at
//              |k| <= K, at the coarse nodes (m == n: the exact identity).  For even n the wavenumber K is kept with what the coarse
//              grid sees of it, cos pi K (x + 1): the square of the Nyquist vector, 1 at every node, comes back as 1/2.
//   which = 2  G (m x n) = R D_F, the product in long double, rounded once
// Every cosine takes the integer multiple 2 k a of pi / (n m), a = i n - j m (R) or i m - j n (P), through cos_pi (one table); the sums run in
// ascending k from the 1.  The Dirichlet kernel of P vanishes where (2K + 1) a is a multiple of n m and a is not: an exact 0.
// A product of two interpolants reaches wavenumber 2K; on m points it folds onto 2K - m, which P drops iff m - 2K > K: the
// smallest such m is 3K + 1 (NOT ceil(3n/2): for even n that is 3K, and 2K folds onto -K).
int fourier_dealias_fine_size(int n) { return 3 * (n / 2) + 1; }

// tab[t] = cos(2 pi t / (n m)), 0 <= t < n m: every cosine of R and P, each evaluated once
static void fourier_cos_table(long nm, std::vector<long double> &tab) {
  tab.resize((size_t)nm);
  for (long t = 0; t < nm; t++) tab[(size_t)t] = cos_pi(2 * t, nm);
}
static inline long double tab_cos(const std::vector<long double> &tab, long ka, long nm) {
  long r = ka % nm;
  return tab[(size_t)(r < 0 ? r + nm : r)];
}

static void fourier_interp_ld(int n, int m, std::vector<long double> &R) {
  const int K = n / 2, Kfull = (n & 1) ? K : K - 1;
  const long nm = (long)n * m;
  std::vector<long double> tab;
  fourier_cos_table(nm, tab);
  R.assign((size_t)m * n, 0.0L);
  for (int i = 0; i < m; i++) {
    long double *row = &R[(size_t)i * n];
    if (((long)i * n) % m == 0) { row[(long)i * n / m] = 1.0L; continue; }
    for (int j = 0; j < n; j++) {
      const long a = (long)i * n - (long)j * m;
      long double s = 1.0L;
      for (int k = 1; k <= Kfull; k++) s += 2.0L * tab_cos(tab, k * a, nm);
      if (!(n & 1)) s += tab_cos(tab, K * a, nm);
      row[j] = s / (long double)n;
    }
  }
}

void fourier_dealias_matrix_host(int n, int m, int which, double *A) {
  const size_t sn = n, sm = m;
  if (which == 1) {
    const int K = n / 2;
    const long nm = (long)n * m;
    std::vector<long double> tab;
    if (m != n) fourier_cos_table(nm, tab);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < m; j++) {
        double &out = A[i * sm + j];
        if (m == n) { out = i == j ? 1.0 : 0.0; continue; }
        const long a = (long)i * m - (long)j * n;
        if (a % nm != 0 && ((2L * K + 1) * a) % nm == 0) { out = 0.0; continue; }
        long double s = 1.0L;
        for (int k = 1; k <= K; k++) s += 2.0L * tab_cos(tab, k * a, nm);
        out = (double)(s / (long double)m);
      }
    return;
  }
  std::vector<long double> R;
  fourier_interp_ld(n, m, R);
  if (which == 0) { for (size_t e = 0; e < sm * sn; e++) A[e] = (double)R[e]; return; }
  std::vector<long double> D;
  fourier_diff_ld(n, 1, D);
  for (size_t i = 0; i < sm; i++)
    for (size_t j = 0; j < sn; j++) {
      long double s = 0.0L;
      for (size_t q = 0; q < sn; q++) s += R[i * sn + q] * D[q * sn + j];
      A[i * sn + j] = (double)s;
    }
}

// Evaluation at arbitrary points of a periodic direction (cheb_points_create_basis, k_points_frows of points.hip).  The device table
// of an extent n, 3 n doubles: the nodes of fourier_nodes_host at [0, n), then sin(pi m / n) at [n, 2n) and cos(pi m / n) at
// [2n, 3n), m = 0 .. n-1, each rounded once.
void fourier_points_table_host(int n, double *tab) {
  fourier_nodes_host(n, tab);
  for (int j = 0; j < n; j++) { tab[n + j] = (double)sin_pi(j, n); tab[2 * n + j] = (double)cos_pi(j, n); }
}

// cos / sin (pi k t) for a long double t: k t is reduced modulo 2 before it meets pi
static void cossin_pik(int k, long double t, long double *c, long double *s) {
  const long double r = fmodl((long double)k * t, 2.0L);
  *c = cosl(PI_L * r); *s = sinl(PI_L * r);
}

// Rows of the trigonometric interpolant (deriv = 0) or of its derivative (deriv = 1) at m arbitrary coordinates, by the cosine sums
// of fourier_dealias_matrix_host's comment with t = x - x_j: x is first wrapped into [-1, 1] (x - 2 rint(x / 2), exact), the sums run
// in ascending k.  Long double, rounded once; a NaN or infinite coordinate gives a row of NaN.
void fourier_points_matrix_host(int n, int m, const double *x, int deriv, double *R) {
  const int K = n / 2, Kfull = (n & 1) ? K : K - 1;
  for (int t = 0; t < m; t++) {
    double *row = R + (size_t)t * n;
    if (!std::isfinite(x[t])) { for (int j = 0; j < n; j++) row[j] = std::numeric_limits<double>::quiet_NaN(); continue; }
    const long double xr = (long double)x[t] - 2.0L * rintl(0.5L * (long double)x[t]);
    for (int j = 0; j < n; j++) {
      const long double dj = xr - (long double)(2 * j - n) / (long double)n;
      long double acc = deriv ? 0.0L : 1.0L, c, s;
      for (int k = 1; k <= Kfull; k++) {
        cossin_pik(k, dj, &c, &s);
        acc += deriv ? -2.0L * (PI_L * (long double)k) * s : 2.0L * c;
      }
      if (!(n & 1)) {
        cossin_pik(K, dj, &c, &s);
        acc += deriv ? -(PI_L * (long double)K) * s : c;
      }
      row[j] = (double)(acc / (long double)n);
    }
  }
}

hipError_t diffmat_create_fourier(int n, int order, DiffMat *out) {
  if (n < 2 || n > 256) return hipErrorInvalidValue;
  std::vector<long double> A;
  fourier_diff_ld(n, order, A);
  return diffmat_from_dense(n, A.data(), order == 2 ? 1 : 0, out);
}

void diffmat_destroy(DiffMat *m) {
  if (m->fragE) (void)hipFree(m->fragE);
  if (m->fragO) (void)hipFree(m->fragO);
  if (m->longDT) (void)hipFree(m->longDT);
  if (m->longD) (void)hipFree(m->longD);
  m->fragE = m->fragO = m->fragE2 = m->fragO2 = m->longDT = m->longD = nullptr;
}

}  // namespace chebhip
