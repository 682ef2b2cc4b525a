// precond.hip -- the finite-difference preconditioner of the reference on the device.
//
// The reference preconditions its Krylov solves with a low-order matrix on the collocation nodes:
//   * FormJacobian (elliptic.C:537-590): the 2d+1-point finite-difference matrix P of
//     -div(eta grad u) - div(deta u grad u0) on the Gauss-Lobatto grid, Dirichlet rows eliminated, handed to
//     PCILU with 2 levels of fill (elliptic.C:184-185);
//   * StokesPCSetUp0 (stokes.C:1160-1241): the same stencil with eta only, per velocity component (MatVVPC),
//     inside KSPVelocity / KSPSchurVelocity (stokes.C:328-341).
// Here P is kept as 2d+1 coefficient arrays in the interior (global-vector) layout and applied by a stencil
// kernel (fd_mult: what MatMult on the AIJ matrix would give, used by the tests and by the defect correction
// below).  The approximate solve that ILU provides in the reference is replaced by something that suits the
// chip: on the tensor grid the constant-coefficient part of P is  sum_k I x .. x T_k x .. x I  with a 1-D
// three-point operator T_k, which is diagonalised ONCE (diffmat.cpp: fdm_line), so that
//     P_1^-1 = (S_0 x S_1 x S_2) diag(1 / (l_i + l_j + l_k)) (S_0^-1 x S_1^-1 x S_2^-1)
// is 2d batched dense line transforms -- one raw-mode launch of the very sweep kernel the operator itself runs on; where
// that cannot run, a dense line product with S^-1 forward and the centro-symmetric plus the centro-antisymmetric part of S,
// two launches, backward (line_transform_g) -- and one pointwise scaling.  For eta == 1 that is the exact inverse of P; for variable coefficients the approximate solve is
// `sweeps` iterations of GMRES on P z = r with P_1^-1 (1/eta) as its right preconditioner (sweeps = 0: that
// preconditioner alone) -- a varying, hence flexible, preconditioner for the outer FGMRES, as ILU(2) is not.
//
// The same pipeline diagonalises the SPECTRAL operator (Haidvogel-Zang): with the line operator A_1 = -(D D)[interior]
// (diffmat.cpp: spec_line) in place of T, the solve is the exact inverse of MatMult_Elliptic at eta == 1, shifted by sigma
// (every modal weight becomes 1 / (sigma + l_i + l_j + l_k): sigma rides on a per-handle copy of dimension 0's eigenvalues).
// Such a handle has no stencil: ell_pc_create_spectral gives z = (sigma I + A)^-1 (r / eta), cheb_helmholtz_* the bare solve.
#include "../../include/chebhip.h"
#include "ops.h"
#include "opfun.h"
#include "sweep.h"
#include "timers.h"
#include <cmath>
#include <array>
#include <map>
#include <new>
#include <tuple>
#include <vector>

using namespace chebhip;

namespace {

constexpr int MAXD = 10;
struct Geo { int d; int dims[MAXD]; long gs[MAXD]; };      // local extents, interior strides

// One row of P per interior node, exactly the arithmetic of elliptic.C:556-579 (gradu[j] null: the deta * du0
// terms are absent, stokes.C:1217-1222).  cf[0] diagonal, cf[1+2j] / cf[2+2j] the neighbours at -1 / +1 along
// dimension j; a neighbour on the boundary has no column (MatSetValues drops negative indices): coefficient 0.
struct GradPtrs { const double *p[MAXD]; };
struct CoordPtrs { const double *p[MAXD]; };
__global__ void k_fd_assemble(Geo geo, long N, long G, const int *__restrict__ ixL, const double *__restrict__ eta,
                              const double *__restrict__ deta, GradPtrs gu, CoordPtrs xs, double *__restrict__ cf,
                              double *__restrict__ eta_g) {
  GS_LOOP(l, N) {
    const int g = ixL[l];
    if (g < 0) continue;
    long rem = l, ls[MAXD]; int ind[MAXD];
    { long s = 1; for (int j = geo.d - 1; j >= 0; j--) { ls[j] = s; s *= geo.dims[j]; } }
    for (int j = 0; j < geo.d; j++) { ind[j] = (int)(rem / ls[j]); rem -= (long)ind[j] * ls[j]; }
    double v0 = 0.0;
    for (int j = 0; j < geo.d; j++) {
      const long iM = l - ls[j], iP = l + ls[j];
      const double x0 = xs.p[j][ind[j]], xMM = xs.p[j][ind[j] - 1], xPP = xs.p[j][ind[j] + 1];
      const double xM = 0.5 * (xMM + x0), idxM = 1.0 / (x0 - xMM), xP = 0.5 * (x0 + xPP), idxP = 1.0 / (xPP - x0), idx = 1.0 / (xP - xM);
      const double eM = 0.5 * (eta[iM] + eta[l]), eP = 0.5 * (eta[iP] + eta[l]);
      double tM = 0.0, tP = 0.0;
      if (gu.p[j]) {
        const double deM = 0.5 * (deta[iM] + deta[l]), du0M = 0.5 * (gu.p[j][iM] + gu.p[j][l]);
        const double deP = 0.5 * (deta[iP] + deta[l]), du0P = 0.5 * (gu.p[j][iP] + gu.p[j][l]);
        tM = 0.5 * deM * du0M; tP = 0.5 * deP * du0P;
      }
      const double vM = -idx * (idxM * eM - tM), vP = -idx * (idxP * eP + tP);
      v0 += idx * (idxP * eP + idxM * eM - (tP - tM));
      cf[(long)(1 + 2 * j) * G + g] = ixL[iM] >= 0 ? vM : 0.0;
      cf[(long)(2 + 2 * j) * G + g] = ixL[iP] >= 0 ? vP : 0.0;
    }
    cf[g] = v0;
    eta_g[g] = eta[l];
  }
}

// slab mode: only the viscosity at the interior nodes is needed (P_1^-1 (r / eta))
__global__ void k_eta_g(long N, const int *__restrict__ ixL, const double *__restrict__ eta, double *__restrict__ eta_g) {
  GS_LOOP(l, N) { const int g = ixL[l]; if (g >= 0) eta_g[g] = eta[l]; }
}

// y = P x on nf stacked fields of G interior values each
__global__ void k_fd_mult(Geo geo, long G, int nf, const double *__restrict__ cf, const double *__restrict__ x, double *__restrict__ y) {
  GS_LOOP(t, G * nf) {
    const long f = t / G, g = t - f * G;
    const double *xf = x + f * G;
    double s = cf[g] * xf[g];
    for (int j = 0; j < geo.d; j++) {
      const double cM = cf[(long)(1 + 2 * j) * G + g], cP = cf[(long)(2 + 2 * j) * G + g];
      if (cM != 0.0) s += cM * xf[g - geo.gs[j]];
      if (cP != 0.0) s += cP * xf[g + geo.gs[j]];
    }
    y[t] = s;
  }
}

// modal scaling: t /= (l_0[i_0] + ... + l_{d-1}[i_{d-1}])
// A sum that is exactly 0 is the dropped mode of a singular solve (sigma = 0, Neumann on every face: each direction's zero
// eigenvalue is set to exactly 0 when its line is built, and every other sum is > 0); every weight path gives it weight 0.
struct LamPtrs { const double *p[MAXD]; };
__global__ void k_modal_scale(Geo geo, long G, int nf, LamPtrs lam, double *__restrict__ t) {
  GS_LOOP(q, G * nf) {
    long g = q % G; double s = 0.0;
    for (int j = 0; j < geo.d; j++) { const long i = g / geo.gs[j]; g -= i * geo.gs[j]; s += lam.p[j][i]; }
    t[q] = s != 0.0 ? t[q] / s : 0.0;
  }
}
// The same for d <= 3 without an integer-division chain per element (four 64-bit divisions cost more than the pass moves):
// block (x, line, field) scales a piece of one line of the last dimension; the line's indices are formed once per block.
__global__ __launch_bounds__(256) void k_modal_scale3(int d, int n1, int nl, long G, const double *__restrict__ l0, const double *__restrict__ l1,
                                                      const double *__restrict__ l2, double *__restrict__ t) {
  const unsigned line = blockIdx.y;                       // d = 3: i0 * n1 + i1; d = 2: i0; d = 1: 0
  double s = 0.0;
  if (d == 3) { const unsigned i0 = line / (unsigned)n1, i1 = line - i0 * (unsigned)n1; s = l0[i0] + l1[i1]; }
  else if (d == 2) s = l0[line];
  const double *ll = d == 3 ? l2 : (d == 2 ? l1 : l0);
  double *row = t + (long)blockIdx.z * G + (long)line * nl;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nl; i += gridDim.x * 256) { const double w = s + ll[i]; row[i] = w != 0.0 ? row[i] / w : 0.0; }
}

// w = 1 / (l_0[i_0] + ... + l_{d-1}[i_{d-1}]) on nf stacked copies of the interior grid (d <= 3): the operand of the last forward
// line transform when it applies the modal scaling itself (OUT_MUL, sweep.h) -- one pass over the nf G values less per solve
__global__ __launch_bounds__(256) void k_modal_weights3(int d, int n1, int nl, long G, const double *__restrict__ l0, const double *__restrict__ l1,
                                                        const double *__restrict__ l2, double *__restrict__ w) {
  const unsigned line = blockIdx.y;
  double s = 0.0;
  if (d == 3) { const unsigned i0 = line / (unsigned)n1, i1 = line - i0 * (unsigned)n1; s = l0[i0] + l1[i1]; }
  else if (d == 2) s = l0[line];
  const double *ll = d == 3 ? l2 : (d == 2 ? l1 : l0);
  double *row = w + (long)blockIdx.z * G + (long)line * nl;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nl; i += gridDim.x * 256) { const double w = s + ll[i]; row[i] = w != 0.0 ? 1.0 / w : 0.0; }
}

// out = (a - (y ? y : 0)) / eta_g  on nf stacked fields
// einv = 1 / eta_g on nf stacked copies: the operand of the first forward line transform when it divides by the viscosity itself (IN_MUL)
__global__ void k_eta_inverse(long G, const double *__restrict__ eta_g, double *__restrict__ einv) {
  const long f0 = (long)blockIdx.y * G;
  GS_LOOP(g, G) einv[f0 + g] = 1.0 / eta_g[g];
}
// (field = blockIdx.y: no 64-bit modulo per element)
__global__ void k_resid_over_eta(long G, int nf, const double *__restrict__ a, const double *__restrict__ y,
                                 const double *__restrict__ eta_g, double *__restrict__ out) {
  const long f0 = (long)blockIdx.y * G;
  GS_LOOP(g, G) { const long q = f0 + g; const double r = y ? a[q] - y[q] : a[q]; out[q] = r / eta_g[g]; }
}

// node-major interleaved (I nodes x d components, the reference's velocity vectors) <-> component-major
// one thread per node: its nf values are contiguous on the node-major side (a wave moves 64 nf contiguous doubles) and
// coalesced field by field on the other
__global__ void k_deinterleave(long G, int nf, const double *__restrict__ a, double *__restrict__ b) {
  GS_LOOP(g, G) { for (int f = 0; f < nf; f++) b[(long)f * G + g] = a[g * nf + f]; }
}
__global__ void k_interleave(long G, int nf, const double *__restrict__ b, double *__restrict__ a) {
  GS_LOOP(g, G) { for (int f = 0; f < nf; f++) a[g * nf + f] = b[(long)f * G + g]; }
}
// out (component-major) = a (node-major) / eta_g: the first step of P_1^-1 (1/eta) on the Stokes velocity vectors, without a
// component-major copy of the right-hand side in between
__global__ void k_deinterleave_over_eta(long G, int nf, const double *__restrict__ a, const double *__restrict__ eta_g, double *__restrict__ out) {
  GS_LOOP(g, G) { const double e = eta_g[g]; for (int f = 0; f < nf; f++) out[(long)f * G + g] = a[g * nf + f] / e; }
}

// ---------------------------------------------------------------------------------------------
// k_fdm_zsolve16: the last forward line transform, the modal scaling and the first backward line transform of the fast-diagonalisation
// solve in ONE launch.  The three act on the same contiguous lines (the last dimension) -- y = S ( W .* (S^-1 x) ) line by line -- so
// the modal coefficients never have to leave the chip: the parity halves the forward product leaves in the accumulators (the raw-mode
// layout of sweep.h: even modes at positions p < H, odd modes at M-1-q) are exactly the split input the backward product takes.
//   A  x lines -> LDS, parity-split          B  c = S^-1 x on the matrix cores; c .*= W; back to LDS as the already split halves
//   D  y = S c on the matrix cores -> HBM
// 24 B/value (x, W, y) instead of 40 for the two launches it replaces.  Lines of 66 .. 128 interior points (KS = 16), M even; tiles of
// 32 lines.  (W and y move as 8-byte pieces in accumulator layout; 16-byte pieces after a DPP lane exchange, as in the sweep kernels'
// epilogue, were built and gave nothing: 144 -> 145-147 us for the MatVVPC solve.)
typedef double fz_v4 __attribute__((ext_vector_type(4)));
struct FzParams { int M, H; unsigned ncols, ntiles; const double *x; double *y; const double *FE, *FO, *BE, *BO;
                  // the modal weights 1 / ((l_0[i] + l_1[j]) + l_z[k]) are formed on the fly (the association of k_modal_weights3: the same
                  // bits as its array W, which cost this launch a third of its bytes): line -> (i, j) within a field of `flines` lines
                  int d, n1; unsigned flines; const double *l0, *l1, *lz; };
// (image row pitch: odd, as in sweep_vec.hip / stokes.hip -- conflict-free operand reads, 8-byte-aligned lines)
constexpr int FZ_PAD = 1;
constexpr int FZ_KS = 16, FZ_LDJ = 4 * FZ_KS + FZ_PAD, FZ_NT = 32;
__device__ __forceinline__ void fz_put2(double *dst, double2 v) {
  if (FZ_LDJ % 2 == 0) *(double2 *)dst = v; else { dst[0] = v.x; dst[1] = v.y; }
}
__global__ __launch_bounds__(256, 3) void k_fdm_zsolve16(const FzParams p) {
  // Workgroups of 256 threads (wave = m-tile, two sub-tiles of 16 lines), three per CU, out of phase with each other; the matrix
  // fragments are fetched from L2 per stage (64 KB) rather than held: 168 registers have to do
  __shared__ __attribute__((aligned(16))) double sE[FZ_NT * FZ_LDJ], sO[FZ_NT * FZ_LDJ];
  const int tid = threadIdx.x, lane = tid & 63, mt = tid >> 6;
  const int kq = lane >> 4, l16 = lane & 15;
  const int M = p.M, H = p.H, mm = M - 1;
  const int oi = mt * 16 + l16;                                        // modal position / output point of this lane (mirror: mm - oi)
  auto chains = [&](const double *AE, const double *AO, fz_v4 (&ce)[2], fz_v4 (&co)[2]) {
    asm volatile("" : "+s"(AE), "+s"(AO));
    double ae[FZ_KS], ao[FZ_KS];
#pragma unroll
    for (int s = 0; s < FZ_KS; s++) { const long q = ((long)(mt * FZ_KS + s)) * 64 + lane; ae[s] = AE[q]; ao[s] = AO[q]; }
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      ce[sub] = fz_v4{0.0, 0.0, 0.0, 0.0}; co[sub] = fz_v4{0.0, 0.0, 0.0, 0.0};
      const int frag = (sub * 16 + l16) * FZ_LDJ + kq;
#pragma unroll
      for (int s = 0; s < FZ_KS; s++) {
        ce[sub] = __builtin_amdgcn_mfma_f64_16x16x4f64(sE[frag + 4 * s], ae[s], ce[sub], 0, 0, 0);
        co[sub] = __builtin_amdgcn_mfma_f64_16x16x4f64(sO[frag + 4 * s], ao[s], co[sub], 0, 0, 0);
      }
    }
  };
  const double lze = oi < H ? p.lz[oi] : 0.0, lzo = oi < H ? p.lz[mm - oi] : 0.0;      // this lane's two modes along z
  for (unsigned tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    // ---- A: four slots per thread: line, points (j, j + 1) and their mirrors (mm - j - 1, mm - j); H odd: the last pair is its own mirror
    {
      double2 rj[4], rm[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int id = tid + 256 * u, line = id >> 5, j = 2 * (id & 31);
        const unsigned gl = tile * FZ_NT + line;
        rj[u] = make_double2(0.0, 0.0); rm[u] = rj[u];
        if (j < H && gl < p.ncols) { rj[u] = *(const double2 *)(p.x + (long)gl * M + j); rm[u] = *(const double2 *)(p.x + (long)gl * M + (mm - j - 1)); }
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int id = tid + 256 * u, line = id >> 5, j = 2 * (id & 31);
        const bool two = j + 1 < H;                                    // (j + 1 == H: that point belongs to the mirror half)
        fz_put2(sE + line * FZ_LDJ + j, make_double2(rj[u].x + rm[u].y, two ? rj[u].y + rm[u].x : 0.0));
        fz_put2(sO + line * FZ_LDJ + j, make_double2(rj[u].x - rm[u].y, two ? rj[u].y - rm[u].x : 0.0));
      }
    }
    __syncthreads();
    // ---- B: modal coefficients, scaled, back to LDS as the split halves of the backward product
    {
      double we[2][4], wo[2][4];
#pragma unroll
      for (int sub = 0; sub < 2; sub++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const unsigned gl = tile * FZ_NT + sub * 16 + 4 * r + kq;
          const bool ok = oi < H && gl < p.ncols;
          double sxy = 0.0;
          if (ok) {
            const unsigned lf = gl % p.flines;
            if (p.d == 3) { const unsigned i0 = lf / (unsigned)p.n1, i1 = lf - i0 * (unsigned)p.n1; sxy = p.l0[i0] + p.l1[i1]; }
            else sxy = p.l0[lf];
          }
          const double se = sxy + lze, so = sxy + lzo;                 // (0: the dropped mode of a singular solve)
          we[sub][r] = ok && se != 0.0 ? 1.0 / se : 0.0; wo[sub][r] = ok && so != 0.0 ? 1.0 / so : 0.0;
        }
      fz_v4 ce[2], co[2];
      chains(p.FE, p.FO, ce, co);
      __syncthreads();                                                 // every wave has finished reading the x images
#pragma unroll
      for (int sub = 0; sub < 2; sub++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int line = sub * 16 + 4 * r + kq;
          sE[line * FZ_LDJ + oi] = we[sub][r] * ce[sub][r];             // (positions H .. 4 KS - 1 get 0: the zero padding of the images)
          sO[line * FZ_LDJ + oi] = wo[sub][r] * co[sub][r];
        }
    }
    __syncthreads();
    // ---- D: y = S c: row i <- E + O, row mm - i <- E - O (the backward matrix is stored centro-symmetric)
    {
      fz_v4 ce[2], co[2];
      chains(p.BE, p.BO, ce, co);
#pragma unroll
      for (int sub = 0; sub < 2; sub++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const unsigned gl = tile * FZ_NT + sub * 16 + 4 * r + kq;
          if (oi < H && gl < p.ncols) {
            double *row = p.y + (long)gl * M;
            row[oi] = ce[sub][r] + co[sub][r]; row[mm - oi] = ce[sub][r] - co[sub][r];
          }
        }
    }
    __syncthreads();                                                   // the images are rewritten by the next tile
  }
}

// parity: the modes use the parity layout (raw transforms, OUT_MUL and k_fdm_zsolve16 usable); a line whose two ends differ has
// ascending modes and runs the dense / two-launch transforms only.  bcm (boundary-condition lines): Q (2 x M), L^T (2 x M), B_BB^-1 (2 x 2)
// Fdense: S^-1 itself (M x M, row-major, rounded once): the forward transform where it cannot be one raw launch (line_transform_g)
struct LineMats { DiffMat Bcs, Bca, Fraw, Braw; double *lam = nullptr; double *bcm = nullptr; double *Fdense = nullptr; int M = 0; bool ok = false, parity = true; };
// lines are shared by the directions of equal extent, equal end conditions (alpha_first, beta_first, alpha_last, beta_last) AND
// equal scale (cheb_helmholtz_create_box; 1 everywhere else)
// ... AND equal basis (BASIS_FOURIER: a periodic line of cheb_helmholtz_create_basis, whose end conditions are unused)
typedef std::tuple<int, std::array<double, 4>, double, int> LineKey;
static const std::array<double, 4> BC_DIRICHLET = {1.0, 0.0, 1.0, 0.0};

// The line of a direction of scale s = 2 / length (cheb_helmholtz_create_box): the operator is -s^2 (D D) and the end condition
// alpha u + beta s du/dnu = g, so the line is spec_line_bc's for the ends (alpha, beta s) with lam and L times s^2 (in long double:
// the caller rounds once); S, S^-1, Q and B_BB^-1 are that line's own.  s = 1 is spec_line_bc itself, bit for bit.
int spec_line_box(int P, const double *bc4, double s, std::vector<long double> &S, std::vector<long double> &Sinv, std::vector<long double> &lam,
                  std::vector<long double> &Q, std::vector<long double> &L, std::vector<long double> &Binv, bool &parity) {
  const double e4[4] = {bc4[0], bc4[1] * s, bc4[2], bc4[3] * s};
  const int rc = spec_line_bc(P, e4, S, Sinv, lam, Q, L, Binv, parity);
  if (rc || s == 1.0) return rc;
  const long double s2 = (long double)s * (long double)s;
  for (auto &v : lam) v *= s2;
  for (auto &v : L) v *= s2;
  return 0;
}

}  // namespace

enum LineKind { LINE_FD = 0, LINE_SPECTRAL = 1 };

struct chebhip_fdpc {
  Geo geo;
  int kind = LINE_FD;                          // LINE_SPECTRAL: lines from spec_line, no stencil (sweeps = 0 only)
  bool bare = false;                           // no operator behind the handle (cheb_helmholtz): no eta, no update
  double *lam0 = nullptr;                      // spectral: sigma + eigenvalues of dimension 0 (a copy: lines[] is shared by directions)
  long N = 0, G = 0;
  int M[MAXD] = {0};                           // unknowns along direction k: dims[k] - 2, or dims[k] on a periodic direction
  int basis[MAXD] = {0};                       // BASIS_CGL / BASIS_FOURIER (cheb_helmholtz_create_basis only)
  int nf = 1;                                  // 1: scalar operator; d: Stokes velocity (component-major inside)
  bool interleaved = false;                    // vectors at the ABI are node-major (Stokes)
  std::map<LineKey, LineMats> lines;           // per distinct (extent, end conditions)
  LineMats *ln[MAXD] = {nullptr};              // direction k's entry of lines
  std::vector<unsigned> inner_g, ncols_g;
  double *xs[MAXD] = {nullptr};
  double *cf = nullptr, *eta_g = nullptr;
  double *t0 = nullptr, *t1 = nullptr, *t2 = nullptr, *t3 = nullptr, *t4 = nullptr, *t5 = nullptr;   // nf * G each
  double *W = nullptr; bool W_tried = false;   // reciprocal modal weights, nf stacked copies (built on first use: fdm_solve)
  double *Einv = nullptr; bool Einv_ok = false;   // 1 / eta_g, nf stacked copies (rebuilt by fdpc_update; used by fdm_solve)
  int sweeps = 1;
  chebhip_fgmres *inner = nullptr; int inner_m = 0;   // the approximate solve with variable coefficients
  bool assembled = false;
  ell_op *eop = nullptr; stokes_op *sop = nullptr;
  // Slab mode: the handle holds the interior nodes of a slab of planes of dimension 0; the line transforms along
  // dimension 0 need whole lines and go through `dim0` (slabx.hip: slab -> pencil, chebhip_fdpc_pencil_transform, back).
  // geo.dims[0] is the GLOBAL extent (matrices, eigenvalues), i0_off the global index of the slab's first interior plane.
  // Only the fast-diagonalisation solve z = P_1^-1 (r / eta) (sweeps = 0) exists on slabs: the stencil of P would need halos.
  bool slab = false; chebhip_fdpc_dim0_fn dim0 = nullptr; void *dim0_ctx = nullptr; long i0_off = 0;
};

static void fdpc_free(chebhip_fdpc *pc) {
  if (!pc) return;
  if (pc->inner) chebhip_fgmres_destroy(pc->inner);
  for (auto &kv : pc->lines) {
    if (!kv.second.ok) continue;
    diffmat_destroy(&kv.second.Bcs); diffmat_destroy(&kv.second.Bca);
    diffmat_destroy(&kv.second.Fraw); diffmat_destroy(&kv.second.Braw);
    if (kv.second.lam) (void)hipFree(kv.second.lam);
    if (kv.second.bcm) (void)hipFree(kv.second.bcm);
    if (kv.second.Fdense) (void)hipFree(kv.second.Fdense);
  }
  for (int k = 0; k < MAXD; k++) if (pc->xs[k]) (void)hipFree(pc->xs[k]);
  double *all[] = {pc->cf, pc->eta_g, pc->t0, pc->t1, pc->t2, pc->t3, pc->t4, pc->t5, pc->W, pc->Einv, pc->lam0};
  for (double *p : all) if (p) (void)hipFree(p);
  delete pc;
}

// kind: LINE_FD (the finite-difference matrix) or LINE_SPECTRAL (sigma + the collocation operator at eta == 1); bare: a spectral
// handle without an operator (v0.ixL / eta unused): only the buffers of the plain solve are allocated
// bc (spectral only; may be null = Dirichlet everywhere): 4 d end conditions, spec_line_bc; scale (with bc only; may be null = 1
// everywhere): d scales, spec_line_box; basis (with bc only; may be null = CGL everywhere): BASIS_FOURIER makes direction k a
// periodic line of M = dims[k] unknowns (fourier_line: closed form, parity layout, no Q, L or B_BB^-1), v0.G counted accordingly
static int fdpc_create(const FdView &v0, int nf, bool interleaved, chebhip_fdpc **out, int gP0 = 0, int kind = LINE_FD, double sigma = 0.0,
                       bool bare = false, const double *bc = nullptr, const double *scale = nullptr, const int *basis = nullptr) {
  *out = nullptr;
  FdView v = v0;
  std::vector<int> gdims(v0.dims, v0.dims + (v0.d >= 1 && v0.d <= MAXD ? v0.d : 0));
  if (gP0 > 0 && !gdims.empty()) { gdims[0] = gP0; v.dims = gdims.data(); }      // slab mode: matrices of the global extent
  if (v.d < 1 || v.d > MAXD) return chebhip_fail(CHEBHIP_ERR_DIMS, "d = %d out of range", v.d);
  for (int k = 0; k < v.d; k++) {
    if (basis && basis[k] == BASIS_FOURIER) {
      if (v.dims[k] < 2) return chebhip_fail(CHEBHIP_ERR_SIZE, "dims[%d] = %d: a periodic direction needs at least 2 points", k, v.dims[k]);
      if (v.dims[k] > 256) return chebhip_fail(CHEBHIP_ERR_ARG, "dims[%d] = %d: a periodic direction supports at most 256 points", k, v.dims[k]);
      continue;
    }
    if (v.dims[k] < 3) return chebhip_fail(CHEBHIP_ERR_SIZE, "dims[%d] = %d: the preconditioner needs interior nodes", k, v.dims[k]);
    if (v.dims[k] > 258) return chebhip_fail(CHEBHIP_ERR_ARG, "dims[%d] = %d: fast diagonalisation supports at most 258 points per line", k, v.dims[k]);
  }
  chebhip_fdpc *pc = new (std::nothrow) chebhip_fdpc;
  if (!pc) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  pc->geo.d = v.d; pc->N = v.N; pc->G = v.G; pc->nf = nf; pc->interleaved = interleaved;
  pc->kind = kind; pc->bare = bare;
  if (kind == LINE_SPECTRAL) { pc->sweeps = 0; pc->assembled = bare; }
  for (int k = 0; k < v.d; k++) {
    pc->geo.dims[k] = v.dims[k];
    pc->basis[k] = basis ? basis[k] : BASIS_CGL;
    pc->M[k] = pc->basis[k] == BASIS_FOURIER ? v.dims[k] : v.dims[k] - 2;
  }
  { long s = 1; for (int k = v.d - 1; k >= 0; k--) { pc->geo.gs[k] = s; s *= pc->M[k]; } }
  pc->inner_g.resize(v.d); pc->ncols_g.resize(v.d);
  for (int k = 0; k < v.d; k++) {
    const int P = v.dims[k], M = pc->M[k];
    const bool fourier = pc->basis[k] == BASIS_FOURIER;
    pc->inner_g[k] = (unsigned)pc->geo.gs[k];
    pc->ncols_g[k] = (unsigned)(v.G / M);                      // (dimension 0 of a slab: unused, its transforms run on pencils)
    std::vector<double> x(P);
    for (int i = 0; i < P; i++) x[i] = cos(i * 3.14159265358979323846 / (P - 1));          // elliptic.C:279, stokes.C:296
    HIP_TRY_OR(hipMalloc((void **)&pc->xs[k], P * sizeof(double)), fdpc_free(pc));
    HIP_TRY_OR(hipMemcpy(pc->xs[k], x.data(), P * sizeof(double), hipMemcpyHostToDevice), fdpc_free(pc));
    std::array<double, 4> bk = BC_DIRICHLET;
    if (bc && !fourier) for (int e = 0; e < 4; e++) bk[e] = bc[4 * k + e];
    const double sk = bc && scale ? scale[k] : 1.0;
    const LineKey key(P, bk, sk, pc->basis[k]);
    if (pc->lines.count(key)) { pc->ln[k] = &pc->lines[key]; continue; }
    LineMats lm;
    std::vector<long double> S, Si, lam, part, Qb, Lb, Bi;
    if (fourier) fourier_line(P, sk, S, Si, lam);
    else if (bc) {
      bool par = true;
      const int rc = spec_line_box(P, bk.data(), sk, S, Si, lam, Qb, Lb, Bi, par);
      if (rc) {
        fdpc_free(pc);
        if (rc == SPEC_BC_COND) return chebhip_fail(CHEBHIP_ERR_ARG, "bc of dimension %d: (alpha, beta) must be finite, >= 0 and not both 0", k);
        if (rc == SPEC_BC_SINGULAR) return chebhip_fail(CHEBHIP_ERR_ARG, "bc of dimension %d: the end rows are singular", k);
        return chebhip_fail(CHEBHIP_ERR_ARG, "eigen-decomposition of the %d-point spectral line operator (bc of dimension %d) failed", P, k);
      }
      lm.parity = par;
      std::vector<double> h((size_t)4 * M + 4);
      for (int j = 0; j < M; j++) {
        h[j] = (double)Qb[j]; h[(size_t)M + j] = (double)Qb[(size_t)M + j];
        h[(size_t)2 * M + j] = (double)Lb[(size_t)2 * j]; h[(size_t)3 * M + j] = (double)Lb[(size_t)2 * j + 1];
      }
      for (int e = 0; e < 4; e++) h[(size_t)4 * M + e] = (double)Bi[e];
      HIP_TRY_OR(hipMalloc((void **)&lm.bcm, h.size() * sizeof(double)), fdpc_free(pc));
      HIP_TRY_OR(hipMemcpy(lm.bcm, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice), fdpc_free(pc));
    } else if (!(kind == LINE_SPECTRAL ? spec_line(P, S, Si, lam) : fdm_line(P, S, Si, lam))) {
      fdpc_free(pc);
      return chebhip_fail(CHEBHIP_ERR_ARG, "eigen-decomposition of the %d-point %s line operator failed", P, kind == LINE_SPECTRAL ? "spectral" : "finite-difference");
    }
    centro_part(M, S, 1, part);  HIP_TRY_OR(diffmat_from_dense(M, part.data(), 1, &lm.Bcs), fdpc_free(pc));
    centro_part(M, S, 0, part);  HIP_TRY_OR(diffmat_from_dense(M, part.data(), 0, &lm.Bca), fdpc_free(pc));
    if (lm.parity) {
      // The same two transforms as ONE product each.  fdm_line orders the modes by parity (even modes at the positions
      // p < H, the q-th odd mode at M-1-q), so with e, o the parity split of a nodal line
      //   forward:  c_p = sum_j Sinv[p][j] e_j (p < H),  c_{M-1-q} = sum_j Sinv[M-1-q][j] o_j      -> halves stored raw
      //   backward: x_i = sum_p S[i][p] c_p + sum_q S[i][M-1-q] c_{M-1-q},  x_{M-1-i} = the difference -> input taken raw
      const int m = M - 1, Hh = (M + 1) / 2;
      std::vector<long double> E((size_t)Hh * Hh, 0.0L), O((size_t)Hh * Hh, 0.0L);
      for (int q = 0; q < Hh; q++)
        for (int j = 0; j < Hh; j++) {
          E[(size_t)q * Hh + j] = Si[(size_t)q * M + j];
          O[(size_t)q * Hh + j] = (2 * q == m || 2 * j == m) ? 0.0L : Si[(size_t)(m - q) * M + j];
        }
      HIP_TRY_OR(diffmat_from_blocks(M, E.data(), O.data(), 1, &lm.Fraw), fdpc_free(pc));
      for (int i = 0; i < Hh; i++)
        for (int j = 0; j < Hh; j++) {
          E[(size_t)i * Hh + j] = S[(size_t)i * M + j];
          O[(size_t)i * Hh + j] = (2 * j == m) ? 0.0L : S[(size_t)i * M + (m - j)];
        }
      HIP_TRY_OR(diffmat_from_blocks(M, E.data(), O.data(), 1, &lm.Braw), fdpc_free(pc));
    }
    {
      std::vector<double> sd((size_t)M * M); for (size_t i = 0; i < sd.size(); i++) sd[i] = (double)Si[i];
      HIP_TRY_OR(hipMalloc((void **)&lm.Fdense, sd.size() * sizeof(double)), fdpc_free(pc));
      HIP_TRY_OR(hipMemcpy(lm.Fdense, sd.data(), sd.size() * sizeof(double), hipMemcpyHostToDevice), fdpc_free(pc));
      lm.M = M;
    }
    std::vector<double> ld(M); for (int i = 0; i < M; i++) ld[i] = (double)lam[i];
    HIP_TRY_OR(hipMalloc((void **)&lm.lam, M * sizeof(double)), fdpc_free(pc));
    HIP_TRY_OR(hipMemcpy(lm.lam, ld.data(), M * sizeof(double), hipMemcpyHostToDevice), fdpc_free(pc));
    lm.ok = true;
    pc->lines[key] = lm;
    pc->ln[k] = &pc->lines[key];
  }
  if (kind == LINE_SPECTRAL) {
    const int M0 = pc->M[0];
    std::vector<double> l0(M0);
    HIP_TRY_OR(hipMemcpy(l0.data(), pc->ln[0]->lam, M0 * sizeof(double), hipMemcpyDeviceToHost), fdpc_free(pc));
    for (int i = 0; i < M0; i++) l0[i] += sigma;
    HIP_TRY_OR(hipMalloc((void **)&pc->lam0, M0 * sizeof(double)), fdpc_free(pc));
    HIP_TRY_OR(hipMemcpy(pc->lam0, l0.data(), M0 * sizeof(double), hipMemcpyHostToDevice), fdpc_free(pc));
  }
  const size_t gb = (size_t)(v.G > 0 ? v.G : 1) * sizeof(double);
  if (kind == LINE_FD) HIP_TRY_OR(hipMalloc((void **)&pc->cf, (2 * v.d + 1) * gb), fdpc_free(pc));
  if (!bare) HIP_TRY_OR(hipMalloc((void **)&pc->eta_g, gb), fdpc_free(pc));
  HIP_TRY_OR(hipMalloc((void **)&pc->t0, nf * gb), fdpc_free(pc)); HIP_TRY_OR(hipMalloc((void **)&pc->t1, nf * gb), fdpc_free(pc));
  if (!bare) {
    HIP_TRY_OR(hipMalloc((void **)&pc->t2, nf * gb), fdpc_free(pc)); HIP_TRY_OR(hipMalloc((void **)&pc->t3, nf * gb), fdpc_free(pc));
    HIP_TRY_OR(hipMalloc((void **)&pc->t4, nf * gb), fdpc_free(pc)); HIP_TRY_OR(hipMalloc((void **)&pc->t5, nf * gb), fdpc_free(pc));
  }
  // the operand arrays of the pointwise steps that ride inside the line transforms (fdm_solve: filled on first use / by update);
  // allocated here so that no solve meets a hipMalloc.  A failed allocation only means the separate passes run.
  if (!opt(OPT_FDM_PASSES) && v.G > 0) {
    bool any_long = false;
    for (int k = 0; k < v.d; k++) any_long = any_long || pc->M[k] > 64;
    if (v.d >= 2 && v.d <= 3 && hipMalloc((void **)&pc->W, nf * gb) != hipSuccess) { pc->W = nullptr; (void)hipGetLastError(); }
    if (any_long && !bare && hipMalloc((void **)&pc->Einv, nf * gb) != hipSuccess) { pc->Einv = nullptr; (void)hipGetLastError(); }
  }
  *out = pc;
  return 0;
}

// 1 / eta for the first forward transform (lines of more than 64 points only: the kernels that take IN_MUL)
static int fdpc_eta_inverse(chebhip_fdpc *pc, hipStream_t st) {
  pc->Einv_ok = false;
  if (opt(OPT_FDM_PASSES) || pc->G == 0) return 0;
  bool any_long = false;
  for (int k = 0; k < pc->geo.d; k++) any_long = any_long || pc->M[k] > 64;
  if (!any_long) return 0;
  if (!pc->Einv) return 0;              // (allocated at create)
  hipLaunchKernelGGL(k_eta_inverse, dim3(grid1d(pc->G, 256, 4096), (unsigned)pc->nf), dim3(256), 0, st, pc->G, (const double *)pc->eta_g, pc->Einv);
  HIP_TRY(hipGetLastError());
  pc->Einv_ok = true;
  return 0;
}

static int fdpc_update(chebhip_fdpc *pc, hipStream_t st) {
  if (pc->bare) return 0;
  FdView v;
  int rc = pc->eop ? ell_op_fd_view_any(pc->eop, &v, nullptr) : stokes_op_fd_view_any(pc->sop, &v, nullptr);
  if (!rc && pc->eop) rc = ell_op_sync_coeffs(pc->eop, (void *)st);
  if (rc) return rc;
  if (pc->G == 0) { pc->assembled = true; return 0; }
  if (pc->slab || pc->kind == LINE_SPECTRAL) {            // no stencil: only eta at the interior nodes
    hipLaunchKernelGGL(k_eta_g, dim3(grid1d(pc->N, 256, 4096)), dim3(256), 0, st, pc->N, v.ixL, v.eta, pc->eta_g);
    HIP_TRY(hipGetLastError());
    pc->assembled = true;
    return fdpc_eta_inverse(pc, st);
  }
  GradPtrs gu; CoordPtrs xs;
  for (int k = 0; k < MAXD; k++) { gu.p[k] = k < v.d ? v.gradu[k] : nullptr; xs.p[k] = pc->xs[k]; }
  hipLaunchKernelGGL(k_fd_assemble, dim3(grid1d(pc->N, 256, 4096)), dim3(256), 0, st, pc->geo, pc->N, pc->G, v.ixL, v.eta, v.deta, gu, xs, pc->cf, pc->eta_g);
  HIP_TRY(hipGetLastError());
  pc->assembled = true;
  return fdpc_eta_inverse(pc, st);
}

// y = S^-1 x (forward) or S x (backward) along dimension k of nf stacked interior fields (x != y): one raw-mode launch
// where the 16-byte kernels can run it, otherwise one dense line product (forward) or the centro-symmetric plus the
// centro-antisymmetric part (backward, two launches)
// mul (forward transforms only; may be null): the result is multiplied by this array as it is stored (OUT_MUL) where the one-launch
// form runs, and *fused says whether it was
// in_mul (forward only; may be null): every input element is multiplied by this array as it is loaded (IN_MUL) -- the caller has
// asked line_in_mul_ok first
// route (may be null): the CHEBHIP_FDPC_ROUTE_* bits of the launches chosen; dry: choose only, launch nothing
static int line_transform_g(LineMats &lm, unsigned ncols, unsigned inner, bool backward, const double *x, double *y, hipStream_t st,
                            const double *mul = nullptr, bool *fused = nullptr, const double *in_mul = nullptr, int *route = nullptr, bool dry = false);
// nf (0: the handle's): the stacked fields of this call, at most the handle's (cheb_opfun: its inputs forward, its outputs backward)
static int line_transform(chebhip_fdpc *pc, int k, bool backward, const double *x, double *y, hipStream_t st, const double *mul = nullptr, bool *fused = nullptr,
                          const double *in_mul = nullptr, int nf = 0, int *route = nullptr, bool dry = false) {
  if (fused) *fused = false;
  if (route) *route = 0;
  if (nf == 0) nf = pc->nf;
  if (pc->slab && k == 0) return dry ? 0 : pc->dim0(pc->dim0_ctx, backward ? 1 : 0, nf, x, y, (void *)st);      // collective: every rank of the slab partition
  return line_transform_g(*pc->ln[k], pc->ncols_g[k] * (unsigned)nf, pc->inner_g[k], backward, x, y, st, mul, fused, in_mul, route, dry);
}
static SweepParams line_in_mul_params(unsigned ncols, unsigned inner, const double *x, double *y, const double *in_mul) {
  SweepParams sm = {};
  sm.ncols = ncols; sm.inner = inner; sm.in0 = x; sm.in1 = in_mul; sm.in_mode = IN_MUL; sm.out = y; sm.alpha = 1.0; sm.out_mode = OUT_STORE; sm.raw = 1;
  return sm;
}
static bool line_in_mul_ok(chebhip_fdpc *pc, int k, const double *x, double *y, const double *in_mul) {
  if ((pc->slab && k == 0) || !in_mul) return false;
  const unsigned ncols = pc->ncols_g[k] * (unsigned)pc->nf;
  return ncols != 0 && pc->ln[k]->parity && sweep_vec_raw_eligible(pc->ln[k]->Fraw, line_in_mul_params(ncols, pc->inner_g[k], x, y, in_mul));
}
static int line_transform_g(LineMats &lm, unsigned ncols, unsigned inner, bool backward, const double *x, double *y, hipStream_t st,
                            const double *mul, bool *fused, const double *in_mul, int *route, bool dry) {
  if (fused) *fused = false;
  if (route) *route = 0;
  if (ncols == 0) return 0;
  if (in_mul && !backward) {
    if (route) *route = CHEBHIP_FDPC_ROUTE_RAW | CHEBHIP_FDPC_ROUTE_FUSED_MUL;
    if (!dry) HIP_TRY(sweep_launch(lm.Fraw, line_in_mul_params(ncols, inner, x, y, in_mul), st));
    return 0;
  }
  SweepParams sp = {};
  sp.ncols = ncols; sp.inner = inner;
  sp.in0 = x; sp.in_mode = IN_PLAIN; sp.out = y; sp.alpha = 1.0;
  sp.out_mode = OUT_STORE;
  if (mul && fused && !backward && lm.parity) {
    SweepParams sm = sp; sm.out_mode = OUT_MUL; sm.acc = mul; sm.raw = 1;
    if (sweep_vec_raw_eligible(lm.Fraw, sm)) {
      if (route) *route = CHEBHIP_FDPC_ROUTE_RAW | CHEBHIP_FDPC_ROUTE_FUSED_MUL;
      if (!dry) HIP_TRY(sweep_launch(lm.Fraw, sm, st));
      *fused = true; return 0;
    }
  }
  if (lm.parity && sweep_vec_raw_eligible(backward ? lm.Braw : lm.Fraw, sp)) {       // one launch: the parity split is the transform's own
    sp.raw = backward ? 2 : 1;
    if (route) *route = CHEBHIP_FDPC_ROUTE_RAW;
    if (!dry) HIP_TRY(sweep_launch(backward ? lm.Braw : lm.Fraw, sp, st));
    return 0;
  }
  // Forward, not as one raw launch: ONE dense line product with S^-1 itself (linegemm.hip: any stride, any alignment).  S^-1 is
  // neither centro-symmetric nor centro-antisymmetric, so as the sum of its two parts (the form of the backward transform below)
  // element i carried the roundings of rows i AND m - i of S^-1 -- where |S^-1[m-i][m-j]| >> |S^-1[i][j]| a relative error of
  // 1e-12 and more (tests/test_gpu_fdm.py); the dense product forms a row from its own entries.  (S in two parts meets the
  // row-wise bar: its columns, not its rows, are the parity modes.)
  if (!backward) {
    if (route) *route = CHEBHIP_FDPC_ROUTE_DENSE;
    if (dry) return 0;
    const ResampleDir rp{lm.Fdense, x, y, ncols / inner, (unsigned)lm.M, (unsigned)lm.M, inner, ncols};
    HIP_TRY(resample_launch(rp, st));
    return 0;
  }
  // (GENERAL: by sweep_launch's own dispatch test)
  if (route) *route = CHEBHIP_FDPC_ROUTE_TWO_LAUNCH | (sweep_takes_vec(lm.Bcs, sp) ? 0 : CHEBHIP_FDPC_ROUTE_GENERAL);
  if (dry) return 0;
  HIP_TRY(sweep_launch(lm.Bcs, sp, st));
  sp.out_mode = OUT_ACC; sp.acc = y;
  HIP_TRY(sweep_launch(lm.Bca, sp, st));
  return 0;
}

// What a solve on this handle does that does not depend on the caller's vectors: the order of the forward transforms, the
// eigenvalue arrays, whether the weight array W is used, whether the last forward transform carries the modal scaling on its
// store (it runs between the handle's own buffers t0 / t1 whenever d >= 2: decided on them) and whether k_fdm_zsolve16 runs.
struct FdmPlan { int d; int order[MAXD]; LamPtrs lam; int nl; long lines; bool w_ok, zsolve, last_fused; };
static FdmPlan fdm_plan(chebhip_fdpc *pc) {
  FdmPlan pl = {};
  const int d = pl.d = pc->geo.d;
  // Forward transforms commute: on slabs in 3-D the first one is a local direction (1) rather than the collective one (0), so that
  // it can take the division by eta on its load side.  Dimension d-1 stays LAST in every order: it takes the modal scaling on its
  // store side, and the one-launch z solve below replaces exactly that transform (a 2-D slab therefore keeps the order 0, 1: its
  // only local direction is the last one, and the division by eta is the separate pass).
  for (int k = 0; k < d; k++) pl.order[k] = k;
  if (pc->slab && d >= 3) { pl.order[0] = 1; pl.order[1] = 0; }
  for (int k = 0; k < MAXD; k++) pl.lam.p[k] = k < d ? pc->ln[k]->lam : nullptr;
  if (pc->lam0) pl.lam.p[0] = pc->lam0;                   // spectral: sigma + l_0 (every weight path reads dimension 0's array)
  pl.nl = pc->M[d - 1];
  pl.lines = pc->G / pl.nl;
  if (pc->slab && d >= 2) pl.lam.p[0] += pc->i0_off;      // the slab's first interior plane is plane i0_off of the global line
  // The modal scaling rides on the store of the last forward transform (dimension d-1 > 0: local on slabs too) where that
  // transform is one launch of the 16-byte kernels: it multiplies by W = 1 / (l_i + l_j + l_k), built on first use (the
  // separate pass divides: the two differ in the last bit).  Option "fdm_passes" = 1 keeps both pointwise passes (A/B).
  pl.w_ok = pc->W && d >= 2 && d <= 3 && pl.lines > 0 && pl.lines <= 65535 && pc->nf <= 65535 && !opt(OPT_FDM_PASSES);
  // The last forward transform, the scaling and the first backward transform act on the same contiguous lines: one launch
  // (k_fdm_zsolve16) where those lines have 66 .. 128 interior points, an even number of them (option "fdm_z_separate" = 1: A/B)
  {
    const int M = pc->M[d - 1];
    LineMats &lm = *pc->ln[d - 1];
    pl.zsolve = pl.w_ok && d >= 2 && lm.parity && !opt(OPT_FDM_Z_SEPARATE) && !opt(OPT_NO_RAW_TRANSFORMS) && !opt(OPT_GENERAL_KERNELS) && (M & 1) == 0 &&
                lm.Fraw.KS == FZ_KS && lm.Braw.KS == FZ_KS && lm.Braw.sym == 1 && pc->G * pc->nf / M < 0x7fffffffL - FZ_NT;
  }
  if (pl.w_ok && !pl.zsolve) {
    const double *s = (d - 1) & 1 ? pc->t0 : pc->t1; double *t = (d - 1) & 1 ? pc->t1 : pc->t0;      // forward transform q reads what q - 1 wrote
    (void)line_transform(pc, d - 1, false, s, t, nullptr, pc->W, &pl.last_fused, nullptr, 0, nullptr, true);
  }
  return pl;
}
// W is filled on first use rather than at create: a slab handle learns its plane offset after create
static int fdm_weights(chebhip_fdpc *pc, const FdmPlan &pl, hipStream_t st) {
  if (!pl.w_ok || pc->W_tried) return 0;
  pc->W_tried = true;
  const int n1 = pl.d == 3 ? pc->M[1] : 1;
  hipLaunchKernelGGL(k_modal_weights3, dim3((unsigned)((pl.nl + 255) / 256), (unsigned)pl.lines, (unsigned)pc->nf), dim3(256), 0, st, pl.d, n1, pl.nl, pc->G,
                     pl.lam.p[0], pl.lam.p[1], pl.lam.p[2], pc->W);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ONE step of the solve along direction k, x -> y (CHEBHIP_FDPC_STEP_*; SCALE alone works in place and takes y == x); fdm_solve is
// a sequence of these calls and chebhip_fdpc_step is one of them on the caller's arrays.  A mode the solve does not take for this
// handle, this direction, these pointers and the current options is refused (CHEBHIP_ERR_ARG), never replaced by another route.
// route (may be null): the CHEBHIP_FDPC_ROUTE_* bits of what runs; dry: decide only.
static int fdm_step(chebhip_fdpc *pc, const FdmPlan &pl, int k, int mode, const double *x, double *y, hipStream_t st, int *route = nullptr, bool dry = false) {
  const int d = pl.d;
  if (route) *route = 0;
  if (k < 0 || k >= d) return chebhip_fail(CHEBHIP_ERR_ARG, "fdpc step: direction %d of %d", k, d);
  const bool first = k == pl.order[0], lastdir = k == pl.order[d - 1];
  int rc = 0, rt = 0;
  switch (mode) {
    case CHEBHIP_FDPC_STEP_FORWARD_OVER_ETA: {
      if (pc->bare || !first) return chebhip_fail(CHEBHIP_ERR_ARG, "fdpc step: the division by eta belongs to the first direction of a handle with an operator");
      if (pl.zsolve && lastdir) return chebhip_fail(CHEBHIP_ERR_ARG, "fdpc step: direction %d runs inside the one-launch z solve", k);
      const double *src = x, *in_mul = nullptr;
      // (dry, on a handle that has not been assembled yet: what its first update will leave -- fdpc_eta_inverse fills Einv wherever it was allocated)
      const bool einv_ok = dry && !pc->assembled ? pc->Einv != nullptr : pc->Einv_ok;
      if (einv_ok && !opt(OPT_FDM_PASSES) && d >= 2 && line_in_mul_ok(pc, k, x, y, pc->Einv)) in_mul = pc->Einv;
      else {
        if (!dry) hipLaunchKernelGGL(k_resid_over_eta, dim3(grid1d(pc->G, 256, 4096), (unsigned)pc->nf), dim3(256), 0, st, pc->G, pc->nf, x, (const double *)nullptr,
                                     (const double *)pc->eta_g, pc->t3);
        src = pc->t3; rt = CHEBHIP_FDPC_ROUTE_ETA_PASS;
      }
      if (!dry && (rc = fdm_weights(pc, pl, st))) return rc;
      int r2 = 0;
      if ((rc = line_transform(pc, k, false, src, y, st, nullptr, nullptr, in_mul, 0, &r2, dry))) return rc;
      rt |= r2;
      break;
    }
    case CHEBHIP_FDPC_STEP_FORWARD:
    case CHEBHIP_FDPC_STEP_FORWARD_SCALED: {
      const bool want = mode == CHEBHIP_FDPC_STEP_FORWARD_SCALED;
      if (pl.zsolve && lastdir) return chebhip_fail(CHEBHIP_ERR_ARG, "fdpc step: direction %d runs inside the one-launch z solve", k);
      // (a Stokes handle divides by eta while it pulls the components apart, chebhip_fdpc_apply, and by the first transform on
      // component-major vectors, chebhip_fdpc_apply_cm: both forms of its first direction are the solve's own)
      if (!want && first && !pc->bare && !pc->interleaved) return chebhip_fail(CHEBHIP_ERR_ARG, "fdpc step: the first direction of this handle divides by eta (FORWARD_OVER_ETA)");
      const bool scaled = lastdir && d >= 2 && pl.last_fused;
      if (want != scaled) return chebhip_fail(CHEBHIP_ERR_ARG, want ? "fdpc step: direction %d does not carry the modal scaling on its store" :
                                                                      "fdpc step: direction %d carries the modal scaling on its store (FORWARD_SCALED)", k);
      bool f = false;
      if (want) {
        (void)line_transform(pc, k, false, x, y, st, pc->W, &f, nullptr, 0, nullptr, true);
        if (!f) return chebhip_fail(CHEBHIP_ERR_ARG, "fdpc step: these arrays cannot take the one-launch transform that carries the modal scaling");
      }
      if (!dry && (rc = fdm_weights(pc, pl, st))) return rc;
      if ((rc = line_transform(pc, k, false, x, y, st, want ? pc->W : nullptr, want ? &f : nullptr, nullptr, 0, &rt, dry))) return rc;
      break;
    }
    case CHEBHIP_FDPC_STEP_SCALE: {
      if (!lastdir || pl.zsolve || (d >= 2 && pl.last_fused)) return chebhip_fail(CHEBHIP_ERR_ARG, "fdpc step: no separate modal scaling pass after direction %d on this handle", k);
      if (pc->slab && !(d <= 3 && pl.lines <= 65535 && pc->nf <= 65535)) return chebhip_fail(CHEBHIP_ERR_ARG, "slab-mode preconditioner: d <= 3 and at most 65535 lines per slab");
      const bool three = d <= 3 && pl.lines <= 65535 && pc->nf <= 65535;
      rt = three ? CHEBHIP_FDPC_ROUTE_SCALE3 : CHEBHIP_FDPC_ROUTE_SCALE_GENERAL;
      if (dry || pl.lines == 0) break;       // (a slab without interior planes: nothing to scale; it still takes part in the transforms along dimension 0)
      if (y != x) HIP_TRY(hipMemcpyAsync(y, x, (size_t)pc->G * pc->nf * sizeof(double), hipMemcpyDeviceToDevice, st));
      if (three) {
        const int n1 = d == 3 ? pc->M[1] : 1;
        hipLaunchKernelGGL(k_modal_scale3, dim3((unsigned)((pl.nl + 255) / 256), (unsigned)pl.lines, (unsigned)pc->nf), dim3(256), 0, st, d, n1, pl.nl, pc->G,
                           pl.lam.p[0], pl.lam.p[1], pl.lam.p[2], y);
      } else
        hipLaunchKernelGGL(k_modal_scale, dim3(grid1d(pc->G * pc->nf, 256, 4096)), dim3(256), 0, st, pc->geo, pc->G, pc->nf, pl.lam, y);
      break;
    }
    case CHEBHIP_FDPC_STEP_ZSOLVE: {
      if (!lastdir || !pl.zsolve) return chebhip_fail(CHEBHIP_ERR_ARG, "fdpc step: the one-launch z solve does not run on this handle (direction %d)", k);
      if (((uintptr_t)x | (uintptr_t)y) & 15) return chebhip_fail(CHEBHIP_ERR_ARG, "fdpc step: the one-launch z solve takes 16-byte-aligned arrays (the handle's own)");
      rt = CHEBHIP_FDPC_ROUTE_ZSOLVE | CHEBHIP_FDPC_ROUTE_RAW | CHEBHIP_FDPC_ROUTE_FUSED_MUL;
      if (dry) break;
      if ((rc = fdm_weights(pc, pl, st))) return rc;
      const int M = pc->M[d - 1];
      LineMats &lm = *pc->ln[d - 1];
      FzParams fp = {};
      fp.M = M; fp.H = (M + 1) / 2; fp.ncols = (unsigned)(pc->G * pc->nf / M); fp.ntiles = (fp.ncols + FZ_NT - 1) / FZ_NT;
      fp.x = x; fp.y = y;
      fp.d = d; fp.n1 = d == 3 ? pc->M[1] : 1; fp.flines = (unsigned)(pc->G / M);
      fp.l0 = pl.lam.p[0]; fp.l1 = pl.lam.p[1]; fp.lz = pl.lam.p[d - 1];
      fp.FE = lm.Fraw.fragE; fp.FO = lm.Fraw.fragO; fp.BE = lm.Braw.fragE; fp.BO = lm.Braw.fragO;
      hipError_t cu_err; const int ncu = sweep_num_cus(&cu_err); HIP_TRY(cu_err);
      const unsigned grid = fp.ntiles < 3u * (unsigned)ncu ? fp.ntiles : 3u * (unsigned)ncu;       // three workgroups per CU
      if (grid) hipLaunchKernelGGL(k_fdm_zsolve16, dim3(grid), dim3(256), 0, st, fp);
      break;
    }
    case CHEBHIP_FDPC_STEP_BACKWARD: {
      if (pl.zsolve && lastdir) return chebhip_fail(CHEBHIP_ERR_ARG, "fdpc step: direction %d runs inside the one-launch z solve", k);
      if ((rc = line_transform(pc, k, true, x, y, st, nullptr, nullptr, nullptr, 0, &rt, dry))) return rc;
      break;
    }
    default: return chebhip_fail(CHEBHIP_ERR_ARG, "fdpc step: unknown mode %d", mode);
  }
  if (route) *route = rt;
  if (!dry) HIP_TRY(hipGetLastError());
  return 0;
}

// z = P_1^-1 r (the constant-coefficient part, exactly), or z = P_1^-1 (r / eta) with over_eta; r is not modified; t0 / t1 (/ t3 with
// over_eta) are scratch (r, z must be none of them)
static int fdm_solve(chebhip_fdpc *pc, const double *r, double *z, hipStream_t st, bool over_eta = false) {
  const FdmPlan pl = fdm_plan(pc);
  const int d = pl.d;
  const double *src = r;
  double *a = pc->t0, *b = pc->t1;
  int rc;
  for (int q = 0; q < (pl.zsolve ? d - 1 : d); q++) {
    const int mode = q == 0 && over_eta ? CHEBHIP_FDPC_STEP_FORWARD_OVER_ETA : (q == d - 1 && q > 0 && pl.last_fused ? CHEBHIP_FDPC_STEP_FORWARD_SCALED : CHEBHIP_FDPC_STEP_FORWARD);
    if ((rc = fdm_step(pc, pl, pl.order[q], mode, src, a, st))) return rc;
    src = a; std::swap(a, b);
  }
  if (pl.zsolve) {
    if ((rc = fdm_step(pc, pl, d - 1, CHEBHIP_FDPC_STEP_ZSOLVE, src, a, st))) return rc;
    src = a; std::swap(a, b);
  } else if (!(d >= 2 && pl.last_fused)) {
    if ((rc = fdm_step(pc, pl, d - 1, CHEBHIP_FDPC_STEP_SCALE, src, (double *)src, st))) return rc;
  }
  for (int k = (pl.zsolve ? d - 2 : d - 1); k >= 0; k--) {
    double *dst = (k == 0) ? z : a;
    if ((rc = fdm_step(pc, pl, k, CHEBHIP_FDPC_STEP_BACKWARD, src, dst, st))) return rc;
    src = dst; std::swap(a, b);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

static int fdpc_mult(chebhip_fdpc *pc, const double *x, double *y, hipStream_t st) {
  if (pc->slab) return chebhip_fail(CHEBHIP_ERR_ARG, "chebhip_fdpc_mult: the stencil of P is not available on slabs (no halo exchange)");
  if (pc->kind == LINE_SPECTRAL) return chebhip_fail(CHEBHIP_ERR_ARG, "chebhip_fdpc_mult: a spectral preconditioner has no stencil");
  if (!pc->assembled) { int rc = fdpc_update(pc, st); if (rc) return rc; }
  if (pc->G == 0) return 0;
  const long n = pc->G * pc->nf;
  const double *xin = x; double *yout = y;
  if (pc->interleaved) { hipLaunchKernelGGL(k_deinterleave, dim3(grid1d(pc->G, 256, 4096)), dim3(256), 0, st, pc->G, pc->nf, x, pc->t2); xin = pc->t2; yout = pc->t3; }
  hipLaunchKernelGGL(k_fd_mult, dim3(grid1d(n, 256, 4096)), dim3(256), 0, st, pc->geo, pc->G, pc->nf, (const double *)pc->cf, xin, yout);
  if (pc->interleaved) hipLaunchKernelGGL(k_interleave, dim3(grid1d(pc->G, 256, 4096)), dim3(256), 0, st, pc->G, pc->nf, (const double *)pc->t3, y);
  HIP_TRY(hipGetLastError());
  return 0;
}

// component-major callbacks of the inner solve: y = P x and z = P_1^-1 (r / eta)
static int cb_fd_mult(void *ctx, const double *x, double *y, void *stream) {
  chebhip_fdpc *pc = (chebhip_fdpc *)ctx;
  hipLaunchKernelGGL(k_fd_mult, dim3(grid1d(pc->G * pc->nf, 256, 4096)), dim3(256), 0, (hipStream_t)stream, pc->geo, pc->G, pc->nf, (const double *)pc->cf, x, y);
  HIP_TRY(hipGetLastError());
  return 0;
}
static int cb_fdm(void *ctx, const double *r, double *z, void *stream) {
  chebhip_fdpc *pc = (chebhip_fdpc *)ctx;
  return fdm_solve(pc, r, z, (hipStream_t)stream, true);
}

static int fdpc_apply(chebhip_fdpc *pc, const double *r, double *z, hipStream_t st) {
  if (!pc->assembled) { int rc = fdpc_update(pc, st); if (rc) return rc; }
  if (pc->slab && pc->sweeps != 0) return chebhip_fail(CHEBHIP_ERR_ARG, "slab-mode preconditioner: sweeps must be 0 (P_1^-1 (r / eta))");
  if (pc->G == 0 && !pc->slab) return 0;              // (a slab without unknowns still takes part in the exchanges of dimension 0)
  const long n = pc->G * pc->nf;
  // component-major copies of r and of the iterate where the ABI vectors are node-major (Stokes velocity)
  const double *rin = r; double *zc = z;
  if (pc->interleaved && pc->sweeps == 0) {    // z = P_1^-1 (r / eta), the division applied while the components are pulled apart
    zc = pc->t4;
    hipLaunchKernelGGL(k_deinterleave_over_eta, dim3(grid1d(pc->G, 256, 4096)), dim3(256), 0, st, pc->G, pc->nf, r, (const double *)pc->eta_g, pc->t3);
    int rc = fdm_solve(pc, pc->t3, zc, st); if (rc) return rc;
  } else if (pc->sweeps == 0) {                // z = P_1^-1 (r / eta)
    int rc = cb_fdm(pc, rin, zc, st); if (rc) return rc;
  } else {
    if (pc->interleaved) { hipLaunchKernelGGL(k_deinterleave, dim3(grid1d(pc->G, 256, 4096)), dim3(256), 0, st, pc->G, pc->nf, r, pc->t2); rin = pc->t2; zc = pc->t4; }
    // `sweeps` iterations of GMRES on P z = r, right-preconditioned by P_1^-1 (1/eta): monotone in the residual for
    // any coefficient state (a stationary defect correction diverges once eta varies by more than a factor ~2)
    if (!pc->inner || pc->inner_m != pc->sweeps) {
      if (pc->inner) chebhip_fgmres_destroy(pc->inner);
      pc->inner = nullptr;
      int rc = chebhip_fgmres_create(n, pc->sweeps, &pc->inner); if (rc) return rc;
      pc->inner_m = pc->sweeps;
    }
    int rc = chebhip_fgmres_set_tolerances(pc->inner, 1e-12, 1e-300, pc->sweeps); if (rc) return rc;
    if ((rc = chebhip_fgmres_solve(pc->inner, cb_fd_mult, pc, cb_fdm, pc, rin, zc, 0, st))) return rc;
  }
  if (pc->interleaved) hipLaunchKernelGGL(k_interleave, dim3(grid1d(pc->G, 256, 4096)), dim3(256), 0, st, pc->G, pc->nf, (const double *)zc, z);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- C ABI: scalar elliptic operator -------------------------------------------------------------
extern "C" int ell_pc_create(ell_op *op, chebhip_fdpc **out) {
  if (!op || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  FdView v; int rc = ell_op_fd_view(op, &v); if (rc) return rc;
  rc = fdpc_create(v, 1, false, out); if (rc) return rc;
  (*out)->eop = op;
  return 0;
}

// ---- C ABI: Stokes velocity block (MatVVPC) ------------------------------------------------------
extern "C" int stokes_pc_create(stokes_op *op, chebhip_fdpc **out) {
  if (!op || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  FdView v; int rc = stokes_op_fd_view(op, &v); if (rc) return rc;
  rc = fdpc_create(v, v.d, true, out); if (rc) return rc;
  (*out)->sop = op;
  return 0;
}

// ---- slab mode (called by the slab drivers of slabx.hip) -------------------------------------------------------
static int fdpc_make_slab(chebhip_fdpc *pc, long i0_off, chebhip_fdpc_dim0_fn dim0, void *ctx) {
  if (!dim0 || i0_off < 0) return chebhip_fail(CHEBHIP_ERR_ARG, "slab-mode preconditioner: bad arguments");
  if (pc->geo.d < 2 || pc->geo.d > 3) return chebhip_fail(CHEBHIP_ERR_DIMS, "slab-mode preconditioner: d = 2 or 3");
  pc->slab = true; pc->dim0 = dim0; pc->dim0_ctx = ctx; pc->i0_off = i0_off; pc->sweeps = 0;
  return 0;
}
extern "C" int stokes_pc_create_slab(stokes_op *op, long i0_offset, chebhip_fdpc_dim0_fn dim0, void *ctx, chebhip_fdpc **out) {
  if (!op || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  FdView v; int gP0 = 0; int rc = stokes_op_fd_view_any(op, &v, &gP0); if (rc) return rc;
  rc = fdpc_create(v, v.d, true, out, gP0); if (rc) return rc;
  (*out)->sop = op;
  if ((rc = fdpc_make_slab(*out, i0_offset, dim0, ctx))) { fdpc_free(*out); *out = nullptr; }
  return rc;
}
extern "C" int ell_pc_create_slab(ell_op *op, long i0_offset, chebhip_fdpc_dim0_fn dim0, void *ctx, chebhip_fdpc **out) {
  if (!op || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  FdView v; int gP0 = 0; int rc = ell_op_fd_view_any(op, &v, &gP0); if (rc) return rc;
  rc = fdpc_create(v, 1, false, out, gP0); if (rc) return rc;
  (*out)->eop = op;
  if ((rc = fdpc_make_slab(*out, i0_offset, dim0, ctx))) { fdpc_free(*out); *out = nullptr; }
  return rc;
}
// The line transform along dimension 0 on a pencil: `nfields` stacked arrays (M0, ncol), lines of M0 = dims[0] - 2 interior
// points with stride ncol.  backward = 0: S^-1 (nodal -> modal), 1: S.
extern "C" int chebhip_fdpc_pencil_transform(chebhip_fdpc *pc, int backward, int nfields, long ncol, const double *in_dev, double *out_dev, void *stream) {
  if (!pc || nfields < 1 || ncol < 0 || ((!in_dev || !out_dev) && ncol > 0)) return chebhip_fail(CHEBHIP_ERR_ARG, "bad argument");
  if (ncol == 0) return 0;
  if ((unsigned long long)nfields * (unsigned long long)ncol > 0x7fffffffull) return chebhip_fail(CHEBHIP_ERR_DIMS, "pencil too large");
  return line_transform_g(*pc->ln[0], (unsigned)(nfields * ncol), (unsigned)ncol, backward != 0, in_dev, out_dev, (hipStream_t)stream);
}

extern "C" int chebhip_fdpc_destroy(chebhip_fdpc *pc) { fdpc_free(pc); return 0; }
extern "C" int chebhip_fdpc_update(chebhip_fdpc *pc, void *stream) { if (!pc) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle"); return fdpc_update(pc, (hipStream_t)stream); }
extern "C" int chebhip_fdpc_set_sweeps(chebhip_fdpc *pc, int sweeps) {
  if (!pc || sweeps < 0 || sweeps > 64) return chebhip_fail(CHEBHIP_ERR_ARG, "sweeps must be in 0..64");
  if (pc->slab && sweeps != 0) return chebhip_fail(CHEBHIP_ERR_ARG, "slab-mode preconditioner: sweeps must be 0");
  if (pc->kind == LINE_SPECTRAL && sweeps != 0) return chebhip_fail(CHEBHIP_ERR_ARG, "spectral preconditioner: sweeps must be 0");
  pc->sweeps = sweeps; return 0;
}
extern "C" int chebhip_fdpc_mult(chebhip_fdpc *pc, const double *x, double *y, void *stream) {
  if (!pc || ((!x || !y) && pc->G)) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (x && x == y) return chebhip_fail(CHEBHIP_ERR_ARG, "x and y must be distinct");
  return fdpc_mult(pc, x, y, (hipStream_t)stream);
}
// Stokes velocity preconditioner on component-major vectors: r, z are nf = d stacked interior fields, which is the layout the
// line transforms work in -- z = P_1^-1 (r / eta) with no (de)interleaving pass on either side
extern "C" int chebhip_fdpc_apply_cm(void *ctx, const double *r, double *z, void *stream) {
  chebhip_fdpc *pc = (chebhip_fdpc *)ctx;
  if (!pc || ((!r || !z) && pc->G)) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (r && r == z) return chebhip_fail(CHEBHIP_ERR_ARG, "r and z must be distinct");
  if (!pc->interleaved || pc->sweeps != 0) return chebhip_fail(CHEBHIP_ERR_ARG, "chebhip_fdpc_apply_cm: a Stokes velocity preconditioner with sweeps = 0");
  StageTimer tm(CHEBHIP_STAGE_FDPC_APPLY, stream);
  hipStream_t st = (hipStream_t)stream;
  if (!pc->assembled) { int rc = fdpc_update(pc, st); if (rc) return rc; }
  if (pc->G == 0 && !pc->slab) return 0;
  return cb_fdm(pc, r, z, st);
}
extern "C" int chebhip_fdpc_apply(void *ctx, const double *r, double *z, void *stream) {
  chebhip_fdpc *pc = (chebhip_fdpc *)ctx;
  if (!pc || ((!r || !z) && pc->G)) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (r && r == z) return chebhip_fail(CHEBHIP_ERR_ARG, "r and z must be distinct");
  StageTimer tm(CHEBHIP_STAGE_FDPC_APPLY, stream);
  return fdpc_apply(pc, r, z, (hipStream_t)stream);
}

// One step of the solve on the caller's arrays (nf stacked interior fields, component-major on a Stokes handle): fdm_step above,
// the very function fdm_solve is made of.  Serial handles only: a slab's dimension 0 is a collective.
static int fdpc_step_check(chebhip_fdpc *pc) {
  if (!pc) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (pc->slab) return chebhip_fail(CHEBHIP_ERR_ARG, "chebhip_fdpc_step: not on slab handles");
  if (pc->G == 0) return chebhip_fail(CHEBHIP_ERR_ARG, "chebhip_fdpc_step: the handle has no unknowns");
  return 0;
}
extern "C" int chebhip_fdpc_step(chebhip_fdpc *pc, int k, int mode, const double *x_dev, double *y_dev, void *stream) {
  int rc = fdpc_step_check(pc); if (rc) return rc;
  if (!x_dev || !y_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL vector");
  if (x_dev == y_dev && mode != CHEBHIP_FDPC_STEP_SCALE) return chebhip_fail(CHEBHIP_ERR_ARG, "chebhip_fdpc_step: x and y must be distinct (SCALE alone works in place)");
  const double *own[] = {pc->t0, pc->t1, pc->t3};
  for (const double *p : own) if (p && (x_dev == p || y_dev == p)) return chebhip_fail(CHEBHIP_ERR_ARG, "chebhip_fdpc_step: the handle's own scratch");
  hipStream_t st = (hipStream_t)stream;
  if (!pc->assembled && (rc = fdpc_update(pc, st))) return rc;
  return fdm_step(pc, fdm_plan(pc), k, mode, x_dev, y_dev, st);
}
extern "C" int chebhip_fdpc_step_route(chebhip_fdpc *pc, int k, int mode) {
  if (fdpc_step_check(pc)) return -1;
  // the arrays of a solve's inner steps: the handle's own, in the order the solve alternates them
  int route = 0;
  if (fdm_step(pc, fdm_plan(pc), k, mode, mode == CHEBHIP_FDPC_STEP_SCALE ? pc->t1 : pc->t0, pc->t1, nullptr, &route, true)) return -1;
  return route;
}
extern "C" int chebhip_fdpc_line_host(int P, double *S, double *Sinv, double *lam) {
  if (P < 3) return chebhip_fail(CHEBHIP_ERR_SIZE, "P = %d: a line needs interior nodes (P >= 3)", P);
  if (P > 258) return chebhip_fail(CHEBHIP_ERR_ARG, "P = %d: at most 258 points per line", P);
  if (!S || !Sinv || !lam) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  std::vector<long double> s, si, l;
  if (!fdm_line(P, s, si, l)) return chebhip_fail(CHEBHIP_ERR_ARG, "eigen-decomposition of the %d-point finite-difference line operator failed", P);
  const int M = P - 2;
  for (size_t i = 0; i < (size_t)M * M; i++) { S[i] = (double)s[i]; Sinv[i] = (double)si[i]; }
  for (int i = 0; i < M; i++) lam[i] = (double)l[i];
  return 0;
}

// ---- C ABI: the spectral preconditioner and the direct Helmholtz solve ------------------------------------------
static int check_sigma(double sigma) {
  if (!(sigma >= 0.0) || !std::isfinite(sigma)) return chebhip_fail(CHEBHIP_ERR_ARG, "sigma = %g must be finite and >= 0", sigma);
  return 0;
}

extern "C" int ell_pc_create_spectral(ell_op *op, double sigma, chebhip_fdpc **out) {
  if (!op || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  *out = nullptr;
  int rc = check_sigma(sigma); if (rc) return rc;
  FdView v; rc = ell_op_fd_view(op, &v); if (rc) return rc;             // (refuses slab-mode handles)
  rc = fdpc_create(v, 1, false, out, 0, LINE_SPECTRAL, sigma); if (rc) return rc;
  (*out)->eop = op;
  return 0;
}

// ---- boundary conditions (cheb_helmholtz_create_bc): the lift of the boundary data and the full-grid extension -------------------
namespace {

// full-grid geometry: extents, row-major strides of the full grid (ls) and of the unknowns (gs), sizes per field (NB = N - G).
// Direction k has M[k] unknowns starting at full-grid index off[k]: (P - 2, 1) between two walls, (P, 0) on a periodic direction
// (cheb_helmholtz_create_basis), which has no face data and no end values.
// 32-bit: a boundary-condition handle has nf N <= 2^31 - 1 (helmholtz_create), so every index below fits.
struct BcGeo { int d; int P[MAXD]; int M[MAXD]; int off[MAXD]; int ls[MAXD]; int gs[MAXD]; int N, G, NB; };
struct BcMats { const double *m[MAXD]; };      // per direction: Q row 0, Q row 1, L column 0, L column 1 (M each), B_BB^-1 (4)

// Position of a boundary node in the compact boundary layout (row-major order over the nodes that are end nodes of some wall
// direction, ell_op_set_dirichlet): its full-grid index minus the number of unknown nodes before it.  The node is end `last` of
// direction k on a line whose indices in directions < k are j[]; the count stops at the first wall end (0: no unknown of that
// subtree comes before; n: all do); a periodic direction m < k counts j[m] whole blocks of unknowns and never ends the walk.
template <int DC>
__device__ __forceinline__ int bc_before(const BcGeo &g, const int *j, int k, bool last) {
  int c = 0;
  bool done = false;
  for (int m = 0; m < (DC ? DC : MAXD); m++)
    if (m < k && !done) {
      if (!g.off[m]) c += j[m] * g.gs[m];
      else if (j[m] == 0) done = true;
      else if (j[m] == g.P[m] - 1) { c += g.M[m] * g.gs[m]; done = true; }
      else c += (j[m] - 1) * g.gs[m];
    }
  return last && !done ? c + g.M[k] * g.gs[k] : c;
}

// t = f + sum over the wall directions k of L_k (g at the two faces of direction k), nf stacked unknown fields (field = blockIdx.y).
// One thread per unknown, the last index fastest: for k < d-1 consecutive threads read consecutive face values; for k = d-1 a
// line's threads share its two values.  The terms are added in k's order, each as L0 g0 + L1 g1.  (DC: d known at compile time,
// 0: any d up to MAXD.)
template <int DC>
__global__ __launch_bounds__(256) void k_bc_lift(BcGeo geo, BcMats bm, const double *__restrict__ f, const double *__restrict__ g,
                                                 double *__restrict__ t) {
  const int d = DC ? DC : geo.d;
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q >= (unsigned)geo.G) return;
  const int fo = blockIdx.y;
  const double *gf = g + fo * geo.NB;
  int i[MAXD];
  unsigned r = q;
  for (int m = (DC ? DC : MAXD) - 1; m > 0; m--)
    if (m < d) { const unsigned Mm = (unsigned)geo.M[m]; i[m] = (int)(r % Mm); r /= Mm; }
  i[0] = (int)r;
  int base = 0;
  for (int m = 0; m < (DC ? DC : MAXD); m++) if (m < d) base += (i[m] + geo.off[m]) * geo.ls[m];
  double s = f[fo * geo.G + (int)q];
  int c = 0;                                   // unknown nodes before the first face node: sum_{m < k} i_m gs_m
  for (int k = 0; k < (DC ? DC : MAXD); k++)
    if (k < d) {
      if (geo.off[k]) {
        const int M = geo.M[k];
        const double *L = bm.m[k] + 2 * M;
        const int b0 = base - (i[k] + 1) * geo.ls[k] - c;
        const int b1 = b0 + (geo.P[k] - 1) * geo.ls[k] - M * geo.gs[k];
        s += L[i[k]] * gf[b0] + L[M + i[k]] * gf[b1];
      }
      c += i[k] * geo.gs[k];
    }
  t[fo * geo.G + (int)q] = s;
}

// End values of the wall direction k < d-1 on nf stacked full grids (field = blockIdx.y): u_end = Q_k u_line + B_BB^-1 g_line on
// every line whose indices in directions < k are any and in directions > k unknowns.  A workgroup takes 64 lines, consecutive in
// the last index (a wave reads 64 consecutive values at every step), and splits each line into four segments, one per wave (one
// thread per line would leave a single wave per SIMD at 256^3); the partial sums meet in LDS.  A Dirichlet end (beta = 0) is
// B_BB^-1 g, a copy for alpha = 1.  src (the FIRST wall direction only, where every direction before k is periodic and these lines
// hold every unknown exactly once): the lines' unknowns are read from the solution in the unknown layout and embedded into u on
// the way.
constexpr int BC_SEG = 4;
template <int DC>
__global__ __launch_bounds__(256) void k_bc_extend_col(BcGeo geo, int k, const double *__restrict__ bm, int dir0, int dir1, int nlines,
                                                       const double *__restrict__ src, const double *__restrict__ g, double *__restrict__ u) {
  __shared__ double red[2][BC_SEG][64];
  const int d = DC ? DC : geo.d;
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const unsigned t = blockIdx.x * 64u + lane;
  const bool ok = t < (unsigned)nlines;
  const int fo = blockIdx.y;
  double *uf = u + fo * geo.N;
  const int M = geo.M[k], ls = geo.ls[k], lend = (geo.P[k] - 1) * ls;
  int j[MAXD];
  unsigned r = ok ? t : 0u;
  int base = 0, ibase = 0;
  for (int m = (DC ? DC : MAXD) - 1; m >= 0; m--) {
    if (m >= d || m == k) continue;
    const unsigned rad = (unsigned)(m < k ? geo.P[m] : geo.M[m]);
    const int x = (int)(r % rad); r /= rad;
    j[m] = m < k ? x : x + geo.off[m];
    base += j[m] * geo.ls[m];
    ibase += (j[m] - geo.off[m]) * geo.gs[m];  // (read with src only: then off[m] = 0 for every m < k)
  }
  const int per = (M + BC_SEG - 1) / BC_SEG, i0 = seg * per, i1 = i0 + per < M ? i0 + per : M;
  double s0 = 0.0, s1 = 0.0;
  if (ok) {
    if (src) {
      const double *sf = src + fo * geo.G + ibase;
      const int gk = geo.gs[k];
#pragma unroll 4
      for (int i = i0; i < i1; i++) {
        const double v = sf[i * gk];
        uf[base + (i + 1) * ls] = v;
        s0 += bm[i] * v; s1 += bm[M + i] * v;
      }
    } else if (!(dir0 && dir1)) {
#pragma unroll 4
      for (int i = i0; i < i1; i++) { const double v = uf[base + (i + 1) * ls]; s0 += bm[i] * v; s1 += bm[M + i] * v; }
    }
  }
  red[0][seg][lane] = s0; red[1][seg][lane] = s1;
  __syncthreads();
  if (seg != 0 || !ok) return;
  s0 = red[0][0][lane]; s1 = red[1][0][lane];
  for (int q = 1; q < BC_SEG; q++) { s0 += red[0][q][lane]; s1 += red[1][q][lane]; }
  double g0 = 0.0, g1 = 0.0;
  if (g) {
    const double *gf = g + fo * geo.NB;
    g0 = gf[base - bc_before<DC>(geo, j, k, false)];
    g1 = gf[base + lend - bc_before<DC>(geo, j, k, true)];
  }
  const double *Bi = bm + 4 * M;
  uf[base] = dir0 ? Bi[0] * g0 : s0 + (Bi[0] * g0 + Bi[1] * g1);
  uf[base + lend] = dir1 ? Bi[3] * g1 : s1 + (Bi[2] * g0 + Bi[3] * g1);
}

// The same for the last direction, whose lines are contiguous: one wave per line (four per workgroup) reduces Q_k u_line across its
// lanes.  src (the first wall direction, as above): every earlier direction is periodic, so line t of u is line t of the solution.
template <int DC>
__global__ __launch_bounds__(256) void k_bc_extend_row(BcGeo geo, const double *__restrict__ bm, int dir0, int dir1, int nlines,
                                                       const double *__restrict__ src, const double *__restrict__ g, double *__restrict__ u) {
  const int d = DC ? DC : geo.d, k = d - 1;
  const unsigned t = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (t >= (unsigned)nlines) return;           // (wave-uniform)
  const int fo = blockIdx.y;
  double *uf = u + fo * geo.N;
  const int M = geo.M[k], lane = threadIdx.x & 63, lend = geo.P[k] - 1;
  int j[MAXD];
  unsigned r = t;
  int base = 0;
  for (int m = (DC ? DC : MAXD) - 2; m >= 0; m--) {
    if (m >= k) continue;
    const int x = (int)(r % (unsigned)geo.P[m]); r /= (unsigned)geo.P[m];
    j[m] = x; base += x * geo.ls[m];
  }
  double s0 = 0.0, s1 = 0.0;
  if (src) {
    const double *sf = src + fo * geo.G + (int)t * M;
    for (int i = lane; i < M; i += 64) { const double v = sf[i]; uf[base + 1 + i] = v; s0 += bm[i] * v; s1 += bm[M + i] * v; }
  } else if (!(dir0 && dir1)) {
    for (int i = lane; i < M; i += 64) { const double v = uf[base + 1 + i]; s0 += bm[i] * v; s1 += bm[M + i] * v; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64); }
  if (lane == 0) {
    double g0 = 0.0, g1 = 0.0;
    if (g) {
      const double *gf = g + fo * geo.NB;
      g0 = gf[base - bc_before<DC>(geo, j, k, false)];
      g1 = gf[base + lend - bc_before<DC>(geo, j, k, true)];
    }
    const double *Bi = bm + 4 * M;
    uf[base] = dir0 ? Bi[0] * g0 : s0 + (Bi[0] * g0 + Bi[1] * g1);
    uf[base + lend] = dir1 ? Bi[3] * g1 : s1 + (Bi[2] * g0 + Bi[3] * g1);
  }
}

}  // namespace

struct cheb_helmholtz {
  chebhip_fdpc *pc = nullptr;
  long n = 0;                                  // nfields * unknowns per field
  // boundary-condition handles (helmholtz_create) only: full-grid geometry, per-direction end flags (beta = 0), the singular flag,
  // two nfields * G buffers
  bool bc = false; int singular = 0;
  bool zero_modes = false;                     // every direction has a zero eigenvalue: singular at sigma = 0 (helmholtz_set_sigma)
  BcGeo geo = {};
  int dir[MAXD][2] = {};
  double *t = nullptr, *z = nullptr;
};

// The argument checks of every Helmholtz handle, and its sizes: N full-grid values and G unknowns per field.  basis: NULL (walls
// everywhere) or as in helmholtz_create.  full: the handle addresses full grids with 32-bit indices, so the bound is on their values
// and not on the unknowns.
static int helmholtz_sizes(int d, const int *dims, const int *basis, double sigma, int nfields, bool full, long *N_out, long *G_out) {
  if (!dims || d < 1 || d > MAXD) return chebhip_fail(CHEBHIP_ERR_DIMS, "d = %d must be in 1..10", d);
  int rc = check_sigma(sigma); if (rc) return rc;
  if (nfields < 1 || nfields > 16) return chebhip_fail(CHEBHIP_ERR_ARG, "nfields = %d must be in 1..16", nfields);
  long N = 1, G = 1;
  for (int k = 0; k < d; k++) {
    const bool fourier = basis && basis[k] == BASIS_FOURIER;
    if (fourier) {
      if (dims[k] < 2) return chebhip_fail(CHEBHIP_ERR_SIZE, "dims[%d] = %d: a periodic direction needs at least 2 points", k, dims[k]);
      if (dims[k] > 256) return chebhip_fail(CHEBHIP_ERR_ARG, "dims[%d] = %d: a periodic direction supports at most 256 points", k, dims[k]);
    } else {
      if (dims[k] < 3) return chebhip_fail(CHEBHIP_ERR_SIZE, "dims[%d] = %d: the solve needs interior nodes", k, dims[k]);
      if (dims[k] > 258) return chebhip_fail(CHEBHIP_ERR_ARG, "dims[%d] = %d: fast diagonalisation supports at most 258 points per line", k, dims[k]);
    }
    G *= fourier ? dims[k] : dims[k] - 2;
    N *= dims[k];                              // (<= 3^d G: no overflow under either bound)
    if (full && N * nfields > 0x7fffffffL) return chebhip_fail(CHEBHIP_ERR_DIMS, "more than 2^31 - 1 full-grid values");
    if (!full && G * nfields > 0x7fffffffL) return chebhip_fail(CHEBHIP_ERR_DIMS, "more than 2^31 - 1 unknowns");
  }
  *N_out = N; *G_out = G;
  return 0;
}

extern "C" int cheb_helmholtz_create(int d, const int *dims, double sigma, int nfields, cheb_helmholtz **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  long N, G;
  int rc = helmholtz_sizes(d, dims, nullptr, sigma, nfields, false, &N, &G); if (rc) return rc;
  FdView v; v.d = d; v.dims = dims; v.N = N; v.G = G;
  cheb_helmholtz *h = new (std::nothrow) cheb_helmholtz;
  if (!h) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  rc = fdpc_create(v, nfields, false, &h->pc, 0, LINE_SPECTRAL, sigma, true);
  if (rc) { delete h; return rc; }
  h->n = G * nfields;
  *out = h;
  return 0;
}

extern "C" int cheb_helmholtz_solve(cheb_helmholtz *h, const double *f_dev, double *u_dev, void *stream) {
  if (!h || !h->pc) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (!f_dev || !u_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL vector");
  // the first forward transform reads f into scratch and the last backward one writes u: u == f is safe
  return fdm_solve(h->pc, f_dev, u_dev, (hipStream_t)stream);
}

extern "C" int cheb_helmholtz_apply(void *h, const double *x_dev, double *y_dev, void *stream) {
  return cheb_helmholtz_solve((cheb_helmholtz *)h, x_dev, y_dev, stream);
}

extern "C" int cheb_helmholtz_destroy(cheb_helmholtz *h) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  fdpc_free(h->pc);
  if (h->t) (void)hipFree(h->t);
  if (h->z) (void)hipFree(h->z);
  delete h;
  return 0;
}

extern "C" long cheb_helmholtz_size(const cheb_helmholtz *h) { return h ? h->n : -1; }
extern "C" chebhip_fdpc *cheb_helmholtz_fdpc(cheb_helmholtz *h) { return h ? h->pc : nullptr; }

extern "C" int cheb_helmholtz_line_host(int P, double *S, double *Sinv, double *lam) {
  if (P < 3) return chebhip_fail(CHEBHIP_ERR_SIZE, "P = %d: a line needs interior nodes (P >= 3)", P);
  if (P > 258) return chebhip_fail(CHEBHIP_ERR_ARG, "P = %d: at most 258 points per line", P);
  if (!S || !Sinv || !lam) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  std::vector<long double> s, si, l;
  if (!spec_line(P, s, si, l)) return chebhip_fail(CHEBHIP_ERR_ARG, "eigen-decomposition of the %d-point spectral line operator failed", P);
  const int M = P - 2;
  for (size_t i = 0; i < (size_t)M * M; i++) { S[i] = (double)s[i]; Sinv[i] = (double)si[i]; }
  for (int i = 0; i < M; i++) lam[i] = (double)l[i];
  return 0;
}

// ---- C ABI: host matrices of a periodic direction; they need no device ------------------------------------------------
static int check_fourier_extent(int n) {
  if (n < 2) return chebhip_fail(CHEBHIP_ERR_SIZE, "n = %d: a periodic direction needs at least 2 points", n);
  if (n > 256) return chebhip_fail(CHEBHIP_ERR_ARG, "n = %d: a periodic direction supports at most 256 points", n);
  return 0;
}
extern "C" int cheb_fourier_nodes_host(int n, double *x) {
  int rc = check_fourier_extent(n); if (rc) return rc;
  if (!x) return chebhip_fail(CHEBHIP_ERR_ARG, "x is NULL");
  fourier_nodes_host(n, x);
  return 0;
}
extern "C" int cheb_fourier_diff_matrix_host(int n, int order, double *D) {
  int rc = check_fourier_extent(n); if (rc) return rc;
  if (order != 1 && order != 2) return chebhip_fail(CHEBHIP_ERR_ARG, "order = %d is neither 1 nor 2", order);
  if (!D) return chebhip_fail(CHEBHIP_ERR_ARG, "D is NULL");
  std::vector<long double> A;
  fourier_diff_ld(n, order, A);
  for (size_t e = 0; e < A.size(); e++) D[e] = (double)A[e];
  return 0;
}
extern "C" int cheb_fourier_line_host(int n, double scale, double *S, double *Sinv, double *lam) {
  int rc = check_fourier_extent(n); if (rc) return rc;
  if (!S || !Sinv || !lam) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (!std::isfinite(scale) || !(scale > 0.0)) return chebhip_fail(CHEBHIP_ERR_ARG, "scale = %g must be finite and > 0", scale);
  std::vector<long double> s, si, l;
  fourier_line(n, scale, s, si, l);
  for (size_t e = 0; e < s.size(); e++) { S[e] = (double)s[e]; Sinv[e] = (double)si[e]; }
  for (int i = 0; i < n; i++) lam[i] = (double)l[i];
  return 0;
}
extern "C" int cheb_fourier_modal_matrix_host(int n, int which, double *M) {
  int rc = check_fourier_extent(n); if (rc) return rc;
  if (which != 0 && which != 1) return chebhip_fail(CHEBHIP_ERR_ARG, "which = %d is neither 0 (forward) nor 1 (backward)", which);
  if (!M) return chebhip_fail(CHEBHIP_ERR_ARG, "M is NULL");
  std::vector<long double> A;
  fourier_modal_ld(n, which, A);
  for (size_t e = 0; e < A.size(); e++) M[e] = (double)A[e];
  return 0;
}
extern "C" int cheb_fourier_modes_host(int n, int *k, int *kind) {
  int rc = check_fourier_extent(n); if (rc) return rc;
  if (!k || !kind) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  fourier_modes_host(n, k, kind);
  return 0;
}

// ---- C ABI: the Helmholtz solve with Dirichlet, Neumann or Robin ends --------------------------------------------
// scale (NULL: 1 everywhere): the box [-1/s_0, 1/s_0] x ..: (sigma - sum_k s_k^2 d_k^2) u = f, alpha u + beta s_k du/dnu = g
// basis (cheb_helmholtz_create_basis; NULL: walls everywhere, cheb_helmholtz_create_box itself): basis[k] = 1 makes direction k
// periodic -- dims[k] unknowns on the nodes -1 + 2 j / dims[k], no faces; its bc entries are not read (bc may be NULL if every
// direction is periodic)
static int helmholtz_create(int d, const int *dims, const int *basis, const double *bc, const double *scale, double sigma, int nfields,
                            cheb_helmholtz **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  long N, G;
  int rc = helmholtz_sizes(d, dims, basis, sigma, nfields, true, &N, &G); if (rc) return rc;
  bool any_per = false, all_per = basis != nullptr;
  for (int k = 0; basis && k < d; k++) {
    if (basis[k] != BASIS_CGL && basis[k] != BASIS_FOURIER) return chebhip_fail(CHEBHIP_ERR_ARG, "basis[%d] = %d is neither 0 (CGL) nor 1 (Fourier)", k, basis[k]);
    any_per = any_per || basis[k] == BASIS_FOURIER; all_per = all_per && basis[k] == BASIS_FOURIER;
  }
  auto fourier = [&](int k) { return basis && basis[k] == BASIS_FOURIER; };
  if (!bc && !all_per) return chebhip_fail(CHEBHIP_ERR_ARG, "bc is NULL");
  for (int k = 0; scale && k < d; k++)
    if (!std::isfinite(scale[k]) || !(scale[k] > 0.0)) return chebhip_fail(CHEBHIP_ERR_ARG, "scale[%d] = %g must be finite and > 0", k, scale[k]);
  for (int k = 0; k < d; k++)
    for (int e = 0; e < 2 && !fourier(k); e++) {
      const double a = bc[4 * k + 2 * e], b = bc[4 * k + 2 * e + 1];
      if (!std::isfinite(a) || !std::isfinite(b) || a < 0.0 || b < 0.0 || (a == 0.0 && b == 0.0))
        return chebhip_fail(CHEBHIP_ERR_ARG, "bc[%d] %s end: (alpha, beta) = (%g, %g) must be finite, >= 0 and not both 0", k, e ? "last" : "first", a, b);
    }
  FdView v; v.d = d; v.dims = dims; v.N = N; v.G = G;
  cheb_helmholtz *h = new (std::nothrow) cheb_helmholtz;
  if (!h) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  std::vector<double> bcd;                     // the end conditions fdpc_create reads: Dirichlet placeholders on periodic directions
  if (any_per) {
    bcd.resize((size_t)4 * d);
    for (int k = 0; k < d; k++) for (int e = 0; e < 4; e++) bcd[(size_t)4 * k + e] = fourier(k) ? BC_DIRICHLET[e] : bc[4 * k + e];
    bc = bcd.data();
  }
  rc = fdpc_create(v, nfields, false, &h->pc, 0, LINE_SPECTRAL, sigma, true, bc, scale, any_per ? basis : nullptr);
  if (rc) { delete h; return rc; }
  h->n = G * nfields; h->bc = true;
  BcGeo &geo = h->geo;
  geo.d = d; geo.N = (int)N; geo.G = (int)G; geo.NB = (int)(N - G);
  for (int k = d - 1, s = 1, si = 1; k >= 0; k--) {
    geo.P[k] = dims[k]; geo.off[k] = fourier(k) ? 0 : 1; geo.M[k] = dims[k] - 2 * geo.off[k];
    geo.ls[k] = s; geo.gs[k] = si;
    s *= geo.P[k]; si *= geo.M[k];
  }
  // singular: some modal sum is exactly 0 -- sigma = 0 and every direction has a zero eigenvalue (Neumann / Neumann: the constant;
  // periodic: the constant and, for an even extent, the Nyquist vector).  Every product of such modes is dropped.
  bool neumann = true;
  for (int k = 0; k < d; k++) {
    if (fourier(k)) { h->dir[k][0] = h->dir[k][1] = 0; continue; }
    h->dir[k][0] = bc[4 * k + 1] == 0.0; h->dir[k][1] = bc[4 * k + 3] == 0.0;
    neumann = neumann && bc[4 * k] == 0.0 && bc[4 * k + 2] == 0.0;
  }
  h->zero_modes = neumann;
  h->singular = sigma == 0.0 && neumann;
  if (hipMalloc((void **)&h->t, (size_t)G * nfields * sizeof(double)) != hipSuccess ||
      hipMalloc((void **)&h->z, (size_t)G * nfields * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    cheb_helmholtz_destroy(h);
    return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of device memory (%ld values)", 2 * G * nfields);
  }
  *out = h;
  return 0;
}

extern "C" int cheb_helmholtz_create_box(int d, const int *dims, const double *bc, const double *scale, double sigma, int nfields,
                                         cheb_helmholtz **out) {
  return helmholtz_create(d, dims, nullptr, bc, scale, sigma, nfields, out);
}

extern "C" int cheb_helmholtz_create_basis(int d, const int *dims, const int *basis, const double *bc, const double *scale, double sigma, int nfields,
                                           cheb_helmholtz **out) {
  if (out) *out = nullptr;
  if (!basis) return chebhip_fail(CHEBHIP_ERR_ARG, "basis is NULL");
  return helmholtz_create(d, dims, basis, bc, scale, sigma, nfields, out);
}

extern "C" int cheb_helmholtz_create_bc(int d, const int *dims, const double *bc, double sigma, int nfields, cheb_helmholtz **out) {
  return cheb_helmholtz_create_box(d, dims, bc, nullptr, sigma, nfields, out);
}

#define BC_LAUNCH(KERNEL, grid, ...)                                                                          \
  do {                                                                                                       \
    switch (geo.d) {                                                                                         \
      case 1: hipLaunchKernelGGL(KERNEL<1>, grid, dim3(256), 0, st, __VA_ARGS__); break;                     \
      case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(256), 0, st, __VA_ARGS__); break;                     \
      case 3: hipLaunchKernelGGL(KERNEL<3>, grid, dim3(256), 0, st, __VA_ARGS__); break;                     \
      default: hipLaunchKernelGGL(KERNEL<0>, grid, dim3(256), 0, st, __VA_ARGS__); break;                    \
    }                                                                                                        \
  } while (0)

static bool overlaps(const double *a, long na, const double *b, long nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)nb * sizeof(double) && pb < pa + (uintptr_t)na * sizeof(double);
}

// u (nf full grids) from the unknown fields z and the boundary data g (null: zero data, u_B = Q u_I): end values of the wall
// directions in ascending order, the lines of one reading the edges the one before has written; the first of them embeds the
// unknowns.  No wall at all: the unknown layout IS the full grid.
static int bc_extend(const cheb_helmholtz *h, int nf, const double *z, const double *g_dev, double *u_dev, hipStream_t st) {
  const BcGeo &geo = h->geo;
  const int d = geo.d;
  bool first = true;
  long before = 1;                             // prod_{m < k} P_m
  for (int k = 0; k < d; k++) {
    if (geo.off[k]) {
      const double *src = first ? z : nullptr, *bm = h->pc->ln[k]->bcm;
      first = false;
      if (k < d - 1) {
        long nl = before;
        for (int m = k + 1; m < d; m++) nl *= geo.M[m];
        BC_LAUNCH(k_bc_extend_col, dim3((unsigned)((nl + 63) / 64), (unsigned)nf), geo, k, bm, h->dir[k][0], h->dir[k][1], (int)nl, src, g_dev, u_dev);
      } else {
        BC_LAUNCH(k_bc_extend_row, dim3((unsigned)((before + 3) / 4), (unsigned)nf), geo, bm, h->dir[k][0], h->dir[k][1], (int)before, src, g_dev, u_dev);
      }
      HIP_TRY(hipGetLastError());
    }
    before *= geo.P[k];
  }
  if (first) HIP_TRY(hipMemcpyAsync(u_dev, z, (size_t)nf * geo.N * sizeof(double), hipMemcpyDeviceToDevice, st));
  return 0;
}

// ---- what the variable-coefficient operator (varhelm.hip, through csrc/ops.h) needs of a boundary-condition handle it owns -----------
// bc_extend on the caller's arrays: u (nfields full grids) from z (nfields unknown fields) and g (may be null)
int helmholtz_extend(const cheb_helmholtz *h, const double *z_dev, const double *g_dev, double *u_dev, void *stream) {
  return bc_extend(h, h->pc->nf, z_dev, g_dev, u_dev, (hipStream_t)stream);
}
// A new shift for the same lines: sigma rides on the handle's copy of dimension 0's eigenvalues and in the weight array built from
// them on first use, nowhere else.  Synchronous (the caller has drained the device: no solve of this handle is in flight).
int helmholtz_set_sigma(cheb_helmholtz *h, double sigma) {
  int rc = check_sigma(sigma); if (rc) return rc;
  chebhip_fdpc *pc = h->pc;
  const int M0 = pc->M[0];
  std::vector<double> l0(M0);
  HIP_TRY(hipMemcpy(l0.data(), pc->ln[0]->lam, M0 * sizeof(double), hipMemcpyDeviceToHost));
  for (int i = 0; i < M0; i++) l0[i] += sigma;
  HIP_TRY(hipMemcpy(pc->lam0, l0.data(), M0 * sizeof(double), hipMemcpyHostToDevice));
  pc->W_tried = false;
  h->singular = sigma == 0.0 && h->zero_modes;
  return 0;
}

// The device memory behind the handle, by the allocations of fdpc_create, helmholtz_create and diffmat.cpp: nfields * G values per field
// buffer (t0, t1, the weight array, t and z of a boundary-condition handle), and per distinct line S^-1 dense, the eigenvalues, the
// end-value matrices and four fragment matrices (one array of cnt + 1032 doubles and one of 3 cnt, cnt = MTP KS 64 -- or cnt each
// for a long line)
size_t helmholtz_work_bytes(const cheb_helmholtz *h) {
  if (!h || !h->pc) return 0;
  const chebhip_fdpc *pc = h->pc;
  const size_t fb = (size_t)(pc->G > 0 ? pc->G : 1) * pc->nf;
  size_t n = 0;
  for (const double *p : {pc->t0, pc->t1, pc->t2, pc->t3, pc->t4, pc->t5, pc->W, pc->Einv, h->t, h->z}) if (p) n += fb;
  if (pc->eta_g) n += fb / pc->nf;
  if (pc->lam0) n += pc->M[0];
  for (int k = 0; k < pc->geo.d; k++) n += pc->geo.dims[k];             // xs
  for (const auto &kv : pc->lines) {
    const LineMats &lm = kv.second;
    if (!lm.ok) continue;
    n += (size_t)lm.M * lm.M + lm.M + (lm.bcm ? 4 * (size_t)lm.M + 4 : 0);
    for (const DiffMat *m : {&lm.Bcs, &lm.Bca, &lm.Fraw, &lm.Braw})
      if (m->fragE) { const size_t cnt = (size_t)m->MTP * m->KS * 64; n += cnt + 1032 + 3 * cnt; }
  }
  return n * sizeof(double);
}

extern "C" int cheb_helmholtz_solve_bc(cheb_helmholtz *h, const double *f_dev, const double *g_dev, double *u_dev, void *stream) {
  if (!h || !h->pc) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (!h->bc) return chebhip_fail(CHEBHIP_ERR_ARG, "cheb_helmholtz_solve_bc: a handle from cheb_helmholtz_create_bc");
  if (!f_dev || !u_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL vector");
  const BcGeo &geo = h->geo;
  const int nf = h->pc->nf;
  const long G = geo.G, N = geo.N, NB = geo.NB;
  if (overlaps(u_dev, nf * N, f_dev, nf * G) || (g_dev && overlaps(u_dev, nf * N, g_dev, nf * NB)))
    return chebhip_fail(CHEBHIP_ERR_ARG, "u may not alias f or g");
  if (g_dev && NB == 0) return chebhip_fail(CHEBHIP_ERR_ARG, "g given, but every direction is periodic: there is no boundary data to lift");
  hipStream_t st = (hipStream_t)stream;
  const double *rhs = f_dev;
  if (g_dev) {                                 // (g = NULL: zero data, nothing to lift)
    BcMats bm;
    for (int k = 0; k < MAXD; k++) bm.m[k] = k < geo.d ? h->pc->ln[k]->bcm : nullptr;
    BC_LAUNCH(k_bc_lift, dim3((unsigned)((G + 255) / 256), (unsigned)nf), geo, bm, f_dev, g_dev, h->t);
    HIP_TRY(hipGetLastError());
    rhs = h->t;
  }
  int rc = fdm_solve(h->pc, rhs, h->z, st); if (rc) return rc;
  return bc_extend(h, nf, h->z, g_dev, u_dev, st);
}


extern "C" long cheb_helmholtz_full_size(const cheb_helmholtz *h) { return h ? (long)h->pc->nf * h->pc->N : -1; }
extern "C" long cheb_helmholtz_boundary_size(const cheb_helmholtz *h) { return h ? (long)h->pc->nf * (h->pc->N - h->pc->G) : -1; }
extern "C" int cheb_helmholtz_singular(const cheb_helmholtz *h) { return h ? h->singular : -1; }

extern "C" int cheb_helmholtz_line_box_host(int P, const double *bc4, double scale, double *S, double *Sinv, double *lam, double *Q, double *L,
                                            double *Binv) {
  if (P < 3) return chebhip_fail(CHEBHIP_ERR_SIZE, "P = %d: a line needs interior nodes (P >= 3)", P);
  if (P > 258) return chebhip_fail(CHEBHIP_ERR_ARG, "P = %d: at most 258 points per line", P);
  if (!bc4 || !S || !Sinv || !lam || !Q || !L || !Binv) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (!std::isfinite(scale) || !(scale > 0.0)) return chebhip_fail(CHEBHIP_ERR_ARG, "scale = %g must be finite and > 0", scale);
  std::vector<long double> s, si, l, q, lf, bi;
  bool parity = true;
  const int rc = spec_line_box(P, bc4, scale, s, si, l, q, lf, bi, parity);
  if (rc == SPEC_BC_COND) return chebhip_fail(CHEBHIP_ERR_ARG, "bc = (%g, %g, %g, %g): each (alpha, beta) must be finite, >= 0 and not both 0", bc4[0], bc4[1], bc4[2], bc4[3]);
  if (rc == SPEC_BC_SINGULAR) return chebhip_fail(CHEBHIP_ERR_ARG, "bc: the end rows are singular");
  if (rc) return chebhip_fail(CHEBHIP_ERR_ARG, "eigen-decomposition of the %d-point spectral line operator with bc failed", P);
  const int M = P - 2;
  for (size_t i = 0; i < (size_t)M * M; i++) { S[i] = (double)s[i]; Sinv[i] = (double)si[i]; }
  for (int i = 0; i < M; i++) lam[i] = (double)l[i];
  for (int i = 0; i < 2 * M; i++) { Q[i] = (double)q[i]; L[i] = (double)lf[i]; }
  for (int i = 0; i < 4; i++) Binv[i] = (double)bi[i];
  return 0;
}

extern "C" int cheb_helmholtz_line_bc_host(int P, const double *bc4, double *S, double *Sinv, double *lam, double *Q, double *L, double *Binv) {
  return cheb_helmholtz_line_box_host(P, bc4, 1.0, S, Sinv, lam, Q, L, Binv);
}

// ---- C ABI: functions of the Helmholtz operator (cheb_opfun_*) -------------------------------------------------------
// The handle is a solver handle of max(nin, nout) fields, of which it uses the lines, the eigenvalues (lam0: sigma + l_0), the two
// transform buffers and, for apply_full, the interior buffer and the extension kernels; the solver's weight array and lift buffer
// are given back at create.  The pointwise step is opfun.hip's kernel, with the table as its argument.
struct cheb_opfun {
  cheb_helmholtz *hz = nullptr;
  int nin = 1, nout = 1;
  bool bc = false;
  long G = 0, N = 0;
  OpfunTable tb = {};
};

extern "C" int cheb_opfun_destroy(cheb_opfun *h) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (h->hz) cheb_helmholtz_destroy(h->hz);
  delete h;
  return 0;
}

// basis null: cheb_opfun_create.  Otherwise the solver handle is cheb_helmholtz_create_basis's (a boundary-condition handle whatever
// bc is: apply_full works, and with every direction periodic it copies, the unknown layout being the full grid)
static int opfun_create(int d, const int *dims, const int *basis, const double *bc, const double *scale, double sigma, int nin, int nout,
                        cheb_opfun **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (nin < 1 || nin > OPFUN_MAX_FIELDS) return chebhip_fail(CHEBHIP_ERR_ARG, "nin = %d must be in 1..16", nin);
  if (nout < 1 || nout > OPFUN_MAX_FIELDS) return chebhip_fail(CHEBHIP_ERR_ARG, "nout = %d must be in 1..16", nout);
  if (!basis && !bc && scale) return chebhip_fail(CHEBHIP_ERR_ARG, "scale needs bc: the box is a boundary-condition handle");
  cheb_opfun *h = new (std::nothrow) cheb_opfun;
  if (!h) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  const int nf = nin > nout ? nin : nout;
  int rc = basis ? cheb_helmholtz_create_basis(d, dims, basis, bc, scale, sigma, nf, &h->hz)
           : bc  ? cheb_helmholtz_create_box(d, dims, bc, scale, sigma, nf, &h->hz)
                 : cheb_helmholtz_create(d, dims, sigma, nf, &h->hz);
  if (rc) { delete h; return rc; }
  h->nin = nin; h->nout = nout; h->bc = h->hz->bc;
  chebhip_fdpc *pc = h->hz->pc;
  h->G = pc->G; h->N = pc->N;
  if (pc->W) { (void)hipFree(pc->W); pc->W = nullptr; }
  if (h->hz->t) { (void)hipFree(h->hz->t); h->hz->t = nullptr; }
  (void)opfun_build_table(nin, nout, 0, nullptr, &h->tb);
  *out = h;
  return 0;
}

extern "C" int cheb_opfun_create(int d, const int *dims, const double *bc, const double *scale, double sigma, int nin, int nout, cheb_opfun **out) {
  return opfun_create(d, dims, nullptr, bc, scale, sigma, nin, nout, out);
}

extern "C" int cheb_opfun_create_basis(int d, const int *dims, const int *basis, const double *bc, const double *scale, double sigma, int nin,
                                       int nout, cheb_opfun **out) {
  if (out) *out = nullptr;
  if (!basis) return chebhip_fail(CHEBHIP_ERR_ARG, "basis is NULL");
  return opfun_create(d, dims, basis, bc, scale, sigma, nin, nout, out);
}

extern "C" int cheb_opfun_set_terms(cheb_opfun *h, int nterms, const cheb_opfun_term *terms) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  OpfunTable tb;
  int rc = opfun_build_table(h->nin, h->nout, nterms, terms, &tb); if (rc) return rc;      // (a refused table leaves the old one in place)
  h->tb = tb;
  return 0;
}

extern "C" long cheb_opfun_size(const cheb_opfun *h, int which) {
  if (!h || which < 0 || which > 2) return -1;
  return which == 0 ? h->nin * h->G : which == 1 ? h->nout * h->G : h->nout * h->N;
}

extern "C" int cheb_opfun_singular(const cheb_opfun *h) { return h ? h->hz->singular : -1; }

// y (nout interior fields: the caller's array or the solver's z, never t0 / t1) from x; d transforms, the mixing launch, d transforms
static int opfun_run(cheb_opfun *h, const double *x, double *y, hipStream_t st) {
  chebhip_fdpc *pc = h->hz->pc;
  const int d = pc->geo.d;
  const double *src = x;
  double *a = pc->t0, *b = pc->t1;
  int rc;
  for (int k = 0; k < d; k++) {
    if ((rc = line_transform(pc, k, false, src, a, st, nullptr, nullptr, nullptr, h->nin))) return rc;
    src = a; std::swap(a, b);
  }
  int M[MAXD]; const double *lam[MAXD];
  for (int k = 0; k < d; k++) { M[k] = pc->M[k]; lam[k] = k == 0 ? pc->lam0 : pc->ln[k]->lam; }
  if ((rc = opfun_mix_launch(h->tb, d, M, pc->G, lam, src, a, st))) return rc;
  src = a; std::swap(a, b);
  for (int k = d - 1; k >= 0; k--) {
    double *dst = k == 0 ? y : a;
    if ((rc = line_transform(pc, k, true, src, dst, st, nullptr, nullptr, nullptr, h->nout))) return rc;
    src = dst; std::swap(a, b);
  }
  return 0;
}

extern "C" int cheb_opfun_apply(cheb_opfun *h, const double *x_dev, double *y_dev, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: NULL handle");
  if (!x_dev || !y_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: NULL array");
  // the first forward transform reads x into scratch and the last backward one writes y: y == x is safe
  if (!(x_dev == y_dev && h->nin == h->nout) && overlaps(x_dev, h->nin * h->G, y_dev, h->nout * h->G))
    return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: y is x (nin == nout) or does not overlap it");
  return opfun_run(h, x_dev, y_dev, (hipStream_t)stream);
}

extern "C" int cheb_opfun_apply_full(cheb_opfun *h, const double *x_dev, double *yfull_dev, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: NULL handle");
  if (!h->bc) return chebhip_fail(CHEBHIP_ERR_ARG, "cheb_opfun_apply_full: a handle made with bc");
  if (!x_dev || !yfull_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: NULL array");
  if (overlaps(x_dev, h->nin * h->G, yfull_dev, h->nout * h->N)) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: yfull may not overlap x");
  int rc = opfun_run(h, x_dev, h->hz->z, (hipStream_t)stream); if (rc) return rc;
  return bc_extend(h->hz, h->nout, h->hz->z, nullptr, yfull_dev, (hipStream_t)stream);
}
#undef BC_LAUNCH
