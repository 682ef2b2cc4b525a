// dealias.hip -- dealiased products and advection terms on the Chebyshev-Gauss-Lobatto grids (cheb_dealias_*, include/chebhip.h):
//   multiply   out[f] = Pi_N (u[f] v[f])
//   advect     out[f] = Pi_N (sum_k vel[k] d_k c[f])
// for `nfields` stacked full-grid fields (field-major, row-major, all nodes: the layout of cheb_modal_*), Pi_N the truncation to
// degree N_k = n_k - 1 per direction of the polynomial product.  Per direction (diffmat.cpp: dealias_matrix_host) R interpolates
// the n coarse values to m >= n fine nodes, G = R D differentiates and interpolates, P = B_n T_m[0:n, :] takes fine values back to
// the coarse nodes keeping the modes 0 .. N; with m > 3 (n - 1) / 2 + 1 (the default m = ceil(3n/2)) nothing aliases.
// A periodic direction (cheb_dealias_create_basis) brings its own R, G = R D_F and P (diffmat.cpp:
// fourier_dealias_matrix_host: the trigonometric interpolant and the cut at the wavenumbers |k| <= floor(n/2)) and its own default
// m = 3 floor(n/2) + 1; nothing below knows the difference.
//
// Schedule.  No operand ever exists at the fine size.  The direction l with the largest m_l / n_l (the last one on a tie) runs
// last on the way up: every operand is first taken to the fine grid in all the OTHER directions by plain line products
// (line_chain of linegemm.hip, fields as the outer extent, shrinking ratios first), which leaves images of prod(m) n_l / m_l
// values per field.
// cheb_pair_kernel below then runs direction l for two images at once, multiplies the two results in registers, adds such
// products over a run-time list of pairs and stores that one array of prod(m) values per field.  multiply has one pair
// (R u, R v); advect has d pairs (R vel_k, G_k c): G sits in direction k of the second operand, so for k != l it is one of the
// plain line products and for k == l it is the pair kernel's second matrix.  The way down is P per direction as plain line
// products, direction l first (it shrinks most), the last one into `out`.
#include "../../include/chebhip.h"
#include "sweep.h"
#include "ops.h"
#include "linetile.h"
#include <algorithm>
#include <map>
#include <new>
#include <utility>
#include <vector>

using namespace chebhip;

namespace {

constexpr int MD = 10;               // directions
constexpr int PR_BM = 64;            // output points per workgroup of the pair kernel

struct PairOp { const double *Ra, *Rb, *xa, *xb; };

struct PairDir {
  double *y;
  unsigned O, K, M, Q, L;            // as ResampleDir, for operand b and the output
  unsigned La;                       // lines of operand a: L, or L / nfields when a is shared by the fields (line % La)
  int npairs;
  PairOp op[MD];
};

// y = sum over the pairs of (Ra xa) o (Rb xb) along one direction.  The tiling, the LDS layout and the order of the MFMA chain are
// those of cheb_resample_kernel (linegemm.hip; linetile.h describes them) with BM = 64, run for two line images side by side:
// three accumulator sets (a, b and
// the sum of products) of 2 x 2 C/D tiles each are 96 registers a lane: 206 .. 232 VGPRs in all, two waves per SIMD (which the launch
// bounds ask for); with BM = 128 the sets are 192 registers, the kernel 464 .. 493, one wave per SIMD.  SAME: every pair has Ra == Rb (multiply): one matrix chunk is loaded, staged and read.  Otherwise both
// copies exist and a pair whose two matrices are the same pointer stages and reads the first one only.
template <bool LINES_A, bool SAME>
__global__ __launch_bounds__(256, 2) void cheb_pair_kernel(const PairDir p) {
  constexpr int BM = PR_BM;
  __shared__ double sRa[BM * RS_RP];
  __shared__ double sRb[SAME ? 1 : BM * RS_RP];
  __shared__ double sXa[RS_KC * RS_XP];
  __shared__ double sXb[RS_KC * RS_XP];
  constexpr int MT = BM / 32;                    // m-tiles of 16 points per wave
  constexpr int XN = RS_KC * RS_BN / 256;        // line-image elements a thread loads per chunk and image
  constexpr int RN = BM * RS_KC / 256;           // matrix elements a thread loads per chunk and matrix
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kq = lane >> 4, l16 = lane & 15;
  const int pw = (w >> 1) * (BM / 2), lw = (w & 1) * 32;     // this wave's first point / line within the tile
  const unsigned K = p.K, M = p.M, Q = p.Q, L = p.L;
  const unsigned l0 = blockIdx.x * RS_BN, i0 = blockIdx.y * BM;

  // what this thread loads: (point, line) of the images and (row, point) of the matrices, the same in every chunk and pair
  unsigned xbb[XN], xba[XN]; int xk[XN], xo[XN]; bool xl[XN];
#pragma unroll
  for (int e = 0; e < XN; e++) {
    const int t = tid + 256 * e;
    int kk, ll;
    if (LINES_A) { ll = t / RS_KC; kk = t % RS_KC; } else { kk = t / RS_BN; ll = t % RS_BN; }
    const unsigned line = l0 + ll, o = line / Q;
    xl[e] = line < L; xk[e] = kk; xo[e] = lds_x(kk, ll);
    xbb[e] = o * K * Q + (line - o * Q);
    const unsigned la = line % p.La, oa = la / Q;
    xba[e] = oa * K * Q + (la - oa * Q);
  }
  int rk[RN], ro[RN]; bool rl[RN]; unsigned rb[RN];
#pragma unroll
  for (int e = 0; e < RN; e++) {
    const int t = tid + 256 * e, ii = t / RS_KC, kk = t % RS_KC;
    rl[e] = i0 + ii < M; rk[e] = kk; ro[e] = lds_r(ii, kk); rb[e] = (i0 + ii) * K;
  }

  v4d sum[MT][2];
#pragma unroll
  for (int u = 0; u < MT; u++)
#pragma unroll
    for (int t = 0; t < 2; t++) sum[u][t] = (v4d){0.0, 0.0, 0.0, 0.0};

  for (int pi = 0; pi < p.npairs; pi++) {
    const double *__restrict__ Ra = p.op[pi].Ra, *__restrict__ Rb = p.op[pi].Rb;
    const double *__restrict__ xa = p.op[pi].xa, *__restrict__ xb = p.op[pi].xb;
    const bool two = !SAME && Ra != Rb;          // (uniform over the workgroup)
    const double *sRb2 = two ? sRb : sRa;

    double xva[XN], xvb[XN], rva[RN], rvb[SAME ? 1 : RN];
    auto load = [&](unsigned k0) {
#pragma unroll
      for (int e = 0; e < XN; e++) {
        const unsigned k = k0 + xk[e];
        const bool ok = xl[e] && k < K;
        xva[e] = ok ? xa[xba[e] + k * Q] : 0.0;
        xvb[e] = ok ? xb[xbb[e] + k * Q] : 0.0;
      }
#pragma unroll
      for (int e = 0; e < RN; e++) {
        const unsigned k = k0 + rk[e];
        const bool ok = rl[e] && k < K;
        rva[e] = ok ? Ra[rb[e] + k] : 0.0;
        if constexpr (!SAME) rvb[e] = (ok && two) ? Rb[rb[e] + k] : 0.0;
      }
    };

    v4d acca[MT][2], accb[MT][2];
#pragma unroll
    for (int u = 0; u < MT; u++)
#pragma unroll
      for (int t = 0; t < 2; t++) acca[u][t] = accb[u][t] = (v4d){0.0, 0.0, 0.0, 0.0};

    load(0);
    for (unsigned k0 = 0; k0 < K; k0 += RS_KC) {
      __syncthreads();                           // (the previous chunk, or the previous pair's last one, has been read)
#pragma unroll
      for (int e = 0; e < XN; e++) { sXa[xo[e]] = xva[e]; sXb[xo[e]] = xvb[e]; }
#pragma unroll
      for (int e = 0; e < RN; e++) {
        sRa[ro[e]] = rva[e];
        if constexpr (!SAME) { if (two) sRb[ro[e]] = rvb[e]; }
      }
      __syncthreads();
      if (k0 + RS_KC < K) load(k0 + RS_KC);      // next chunk in flight during the products
#pragma unroll
      for (int ks = 0; ks < RS_KC / 4; ks++) {
        double aa[MT], ab[MT], ba[2], bb[2];
#pragma unroll
        for (int u = 0; u < MT; u++) {
          aa[u] = sRa[lds_r(pw + 16 * u + l16, 4 * ks + kq)];
          ab[u] = SAME ? aa[u] : sRb2[lds_r(pw + 16 * u + l16, 4 * ks + kq)];
        }
#pragma unroll
        for (int t = 0; t < 2; t++) {
          ba[t] = sXa[lds_x(4 * ks + kq, lw + 16 * t + l16)];
          bb[t] = sXb[lds_x(4 * ks + kq, lw + 16 * t + l16)];
        }
#pragma unroll
        for (int u = 0; u < MT; u++)
#pragma unroll
          for (int t = 0; t < 2; t++) {
            acca[u][t] = line_mfma<LINES_A>(aa[u], ba[t], acca[u][t]);
            accb[u][t] = line_mfma<LINES_A>(ab[u], bb[t], accb[u][t]);
          }
      }
    }
#pragma unroll
    for (int u = 0; u < MT; u++)
#pragma unroll
      for (int t = 0; t < 2; t++) sum[u][t] += acca[u][t] * accb[u][t];
  }

  // C/D element r of a lane: row (lane >> 4) + 4 r, column lane & 15
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const unsigned line = l0 + lw + 16 * t + (LINES_A ? 4 * r + kq : l16);
      if (line >= L) continue;
      const unsigned o = line / Q, ob = o * M * Q + (line - o * Q);
#pragma unroll
      for (int u = 0; u < MT; u++) {
        const unsigned i = i0 + pw + 16 * u + (LINES_A ? l16 : 4 * r + kq);
        if (i < M) p.y[ob + i * Q] = sum[u][t][r];
      }
    }
}

template <bool LINES_A, bool SAME>
hipError_t pair_launch_t(const PairDir &p, hipStream_t st) {
  const dim3 grid((p.L + RS_BN - 1) / RS_BN, (p.M + PR_BM - 1) / PR_BM);
  hipLaunchKernelGGL((cheb_pair_kernel<LINES_A, SAME>), grid, dim3(256), 0, st, p);
  sweep_note_launch();
  return hipGetLastError();
}

hipError_t pair_launch(const PairDir &p, hipStream_t st) {
  bool same = true;
  for (int i = 0; i < p.npairs; i++) same = same && p.op[i].Ra == p.op[i].Rb;
  const bool la = p.Q <= 4;
  if (same) return la ? pair_launch_t<true, true>(p, st) : pair_launch_t<false, true>(p, st);
  return la ? pair_launch_t<true, false>(p, st) : pair_launch_t<false, false>(p, st);
}

}  // namespace

struct cheb_dealias {
  int d = 0, nf = 1, l = 0;                  // l: the direction run last on the way up
  int n[MD] = {0}, m[MD] = {0};
  long coarse = 0, fine = 0, img = 0;        // values per field: prod(n), prod(m), prod(m) n_l / m_l
  std::vector<int> up, down;                 // the other directions on the way up; all directions with m != n on the way down
  int basis[MD] = {0};                       // CHEB_BASIS_* per direction (cheb_dealias_create_basis; all CGL otherwise)
  std::map<std::pair<std::pair<int, int>, int>, double *> mats;   // device: R (m n), P (n m), G (m n) of a distinct ((n, m), basis), one allocation
  double *prod = nullptr;                    // nf * fine: the product on the fine grid
  double *image = nullptr;                   // image_fields * img: the operands before direction l; the way down's intermediates
  double *tmp[2] = {nullptr, nullptr};       // tmp_fields * tmp_len[b]: an operand's intermediates before its image
  long image_fields = 0, tmp_fields = 0, tmp_len[2] = {0, 0};
  bool advect_ready = false;
  size_t mat_bytes = 0;

  const double *mat(int k, int which) const {
    const double *base = mats.at({{n[k], m[k]}, basis[k]});
    return base + (size_t)which * n[k] * m[k];
  }
  size_t work_bytes() const {
    return sizeof(double) * ((size_t)nf * fine + (size_t)image_fields * img + (size_t)tmp_fields * (tmp_len[0] + tmp_len[1])) + mat_bytes;
  }
};

extern "C" int cheb_dealias_fine_size(int n) {
  return check_extent(n) ? -1 : dealias_fine_size(n);
}

namespace {

int check_basis_value(int basis) {
  if (basis != CHEB_BASIS_CGL && basis != CHEB_BASIS_FOURIER) return chebhip_fail(CHEBHIP_ERR_ARG, "basis = %d is neither 0 (CGL) nor 1 (Fourier)", basis);
  return 0;
}

// the coarse extent of one direction: check_extent, or the range of a periodic direction
int check_coarse(int n, int basis) {
  if (basis != CHEB_BASIS_FOURIER) return check_extent(n);
  if (n < 2) return chebhip_fail(CHEBHIP_ERR_SIZE, "n = %d: a periodic direction needs at least 2 points", n);
  if (n > 256) return chebhip_fail(CHEBHIP_ERR_ARG, "n = %d: a periodic direction supports at most 256 points", n);
  return 0;
}

}  // namespace

extern "C" int cheb_dealias_fine_size_basis(int n, int basis) {
  if (check_basis_value(basis) || check_coarse(n, basis)) return -1;
  return basis == CHEB_BASIS_FOURIER ? fourier_dealias_fine_size(n) : dealias_fine_size(n);
}

extern "C" int cheb_dealias_matrix_host(int n, int m, int which, double *A) {
  int rc;
  if ((rc = check_extent(n)) || (rc = check_extent(m))) return rc;
  if (m < n) return chebhip_fail(CHEBHIP_ERR_ARG, "m = %d is smaller than n = %d", m, n);
  if (which < 0 || which > 2) return chebhip_fail(CHEBHIP_ERR_ARG, "which = %d is none of 0 (R), 1 (P), 2 (G)", which);
  if (!A) return chebhip_fail(CHEBHIP_ERR_ARG, "matrix is NULL");
  dealias_matrix_host(n, m, which, A);
  return 0;
}

extern "C" int cheb_dealias_matrix_basis_host(int n, int m, int which, int basis, double *A) {
  int rc;
  if ((rc = check_basis_value(basis))) return rc;
  if (basis == CHEB_BASIS_CGL) return cheb_dealias_matrix_host(n, m, which, A);
  if ((rc = check_coarse(n, basis)) || (rc = check_extent(m))) return rc;
  if (m < n) return chebhip_fail(CHEBHIP_ERR_ARG, "m = %d is smaller than n = %d", m, n);
  if (which < 0 || which > 2) return chebhip_fail(CHEBHIP_ERR_ARG, "which = %d is none of 0 (R), 1 (P), 2 (G)", which);
  if (!A) return chebhip_fail(CHEBHIP_ERR_ARG, "matrix is NULL");
  fourier_dealias_matrix_host(n, m, which, A);
  return 0;
}

extern "C" int cheb_dealias_destroy(cheb_dealias *h) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  for (auto &mm : h->mats) if (mm.second) (void)hipFree(mm.second);
  if (h->prod) (void)hipFree(h->prod);
  if (h->image) (void)hipFree(h->image);
  for (double *b : h->tmp) if (b) (void)hipFree(b);
  delete h;
  return 0;
}

namespace {

// (re)allocates the image and the intermediates for operands of `fields` fields in all and `job` fields at a time
int dealias_reserve(cheb_dealias *h, long fields, long job) {
  if (h->d == 1) return 0;                                     // direction l is the only one: the operands are their own images
  if (fields * h->img >= 0x80000000L) return chebhip_fail(CHEBHIP_ERR_DIMS, "operand images of 2^31 values or more");
  if (fields > h->image_fields) {
    if (h->image) { (void)hipFree(h->image); h->image = nullptr; h->image_fields = 0; }
    if (hipMalloc(&h->image, (size_t)fields * h->img * sizeof(double)) != hipSuccess)
      return chebhip_fail(CHEBHIP_ERR_MEMORY, "dealias operand images of %ld doubles", fields * h->img);
    h->image_fields = fields;
  }
  if (job > h->tmp_fields) {
    for (int b = 0; b < 2; b++) {
      if (h->tmp[b]) { (void)hipFree(h->tmp[b]); h->tmp[b] = nullptr; }
      if (h->tmp_len[b] && hipMalloc(&h->tmp[b], (size_t)job * h->tmp_len[b] * sizeof(double)) != hipSuccess) {
        h->tmp_fields = 0;
        return chebhip_fail(CHEBHIP_ERR_MEMORY, "dealias work buffer of %ld doubles", job * h->tmp_len[b]);
      }
    }
    h->tmp_fields = job;
  }
  return 0;
}

}  // namespace

// basis null: cheb_dealias_create.  A Fourier direction brings its own three matrices and its own default fine size; the schedule,
// the buffers and the launches do not know the difference.
static int dealias_create(int d, const int *dims, const int *dims_fine, const int *basis, int nfields, cheb_dealias **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  int rc, mk[MD];
  if ((rc = check_field_count(d, dims, nfields))) return rc;
  // (not check_field_extents: a direction's faults have this module's texts, shared with *_basis_host, and the bound is the fine grid's)
  long coarse = 1, fine = 1;
  for (int k = 0; k < d; k++) {
    const int bk = basis ? basis[k] : CHEB_BASIS_CGL;
    if ((rc = check_basis_value(bk)) || (rc = check_coarse(dims[k], bk))) return rc;
    mk[k] = dims_fine ? dims_fine[k] : bk == CHEB_BASIS_FOURIER ? fourier_dealias_fine_size(dims[k]) : dealias_fine_size(dims[k]);
    if (mk[k] < dims[k]) return chebhip_fail(CHEBHIP_ERR_ARG, "direction %d: fine size %d is smaller than %d", k, mk[k], dims[k]);
    if (mk[k] > 1024)
      return chebhip_fail(CHEBHIP_ERR_ARG, "direction %d: fine size %d: at most 1024 points per direction%s", k, mk[k],
                          dims_fine ? "" : " (the 3/2 rule takes n <= 682)");
    coarse *= dims[k]; fine *= mk[k];
    if (nfields * fine >= 0x80000000L) return chebhip_fail(CHEBHIP_ERR_DIMS, "2^31 values or more on the fine grid");
  }
  if ((rc = require_device())) return rc;
  cheb_dealias *h = new (std::nothrow) cheb_dealias;
  if (!h) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  h->d = d; h->nf = nfields; h->coarse = coarse; h->fine = fine;
  int l = 0;
  for (int k = 0; k < d; k++) {
    h->n[k] = dims[k]; h->m[k] = mk[k]; h->basis[k] = basis ? basis[k] : CHEB_BASIS_CGL;
    if ((long)mk[k] * dims[l] >= (long)mk[l] * dims[k]) l = k;            // the largest m / n, the last one on a tie
  }
  h->l = l;
  h->img = fine / mk[l] * dims[l];
  for (int k = 0; k < d; k++) if (k != l) h->up.push_back(k);
  order_by_ratio(h->up.data(), h->up.data() + h->up.size(), h->m, h->n);           // growing least first: small intermediates
  for (int k = 0; k < d; k++) if (k != l && mk[k] != dims[k]) h->down.push_back(k);
  order_by_ratio(h->down.data(), h->down.data() + h->down.size(), h->n, h->m);     // shrinking most first
  if (mk[l] != dims[l]) h->down.insert(h->down.begin(), l);
  // an operand's intermediates: stage s of its line products writes tmp[s & 1], the last one its image.  An operand may skip
  // directions with m == n, which shifts the stages: both buffers take the largest intermediate.
  {
    long cur = coarse, len = 0;
    for (size_t s = 0; s + 1 < h->up.size(); s++) {
      const int k = h->up[s];
      cur = cur / dims[k] * mk[k];
      len = std::max(len, cur);
    }
    if (h->up.size() >= 2) h->tmp_len[0] = len;
    if (h->up.size() >= 3) h->tmp_len[1] = len;
  }

  std::vector<double> buf;
  for (int k = 0; k < d && !rc; k++) {
    const std::pair<std::pair<int, int>, int> key{{dims[k], mk[k]}, h->basis[k]};
    if (h->mats.count(key)) continue;
    const size_t nm = (size_t)dims[k] * mk[k];
    buf.resize(3 * nm);
    for (int which = 0; which < 3; which++) {
      if (h->basis[k] == CHEB_BASIS_FOURIER) fourier_dealias_matrix_host(dims[k], mk[k], which, buf.data() + which * nm);
      else dealias_matrix_host(dims[k], mk[k], which, buf.data() + which * nm);
    }
    double *dev = nullptr;
    if ((rc = device_array(&dev, 3 * nm, buf.data(), "dealias matrices"))) break;
    h->mats[key] = dev;
    h->mat_bytes += 3 * nm * sizeof(double);
  }
  if (!rc) rc = device_array(&h->prod, (size_t)nfields * fine, nullptr, "dealias product buffer");
  if (!rc) rc = dealias_reserve(h, 2L * nfields, nfields);
  if (rc) { cheb_dealias_destroy(h); return rc; }
  *out = h;
  return 0;
}

extern "C" int cheb_dealias_create(int d, const int *dims, const int *dims_fine, int nfields, cheb_dealias **out) {
  return dealias_create(d, dims, dims_fine, nullptr, nfields, out);
}

extern "C" int cheb_dealias_create_basis(int d, const int *dims, const int *dims_fine, const int *basis, int nfields, cheb_dealias **out) {
  if (out) *out = nullptr;
  if (!basis) return chebhip_fail(CHEBHIP_ERR_ARG, "basis is NULL");
  return dealias_create(d, dims, dims_fine, basis, nfields, out);
}

extern "C" int cheb_dealias_reserve_advect(cheb_dealias *h) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (h->advect_ready) return 0;
  int rc;
  if ((rc = dealias_reserve(h, (long)h->d * (1 + h->nf), std::max(h->d, h->nf)))) return rc;
  h->advect_ready = true;
  return 0;
}

extern "C" int cheb_dealias_fine_dims(const cheb_dealias *h, int *dims_fine) {
  if (!h || !dims_fine) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  for (int k = 0; k < h->d; k++) dims_fine[k] = h->m[k];
  return 0;
}

extern "C" long cheb_dealias_size(const cheb_dealias *h) { return h ? h->nf * h->coarse : -1; }
extern "C" long cheb_dealias_work_bytes(const cheb_dealias *h) { return h ? (long)h->work_bytes() : -1; }

namespace {

// `fields` coarse fields at x to the fine grid in every direction but l, direction g (-1: none) through G instead of R: the
// result is written to `image` (fields * img values), or IS x when no direction is left to run
int dealias_lift(cheb_dealias *h, const double *x, long fields, int g, double *image, const double **res, hipStream_t st) {
  long cur[MD];
  for (int k = 0; k < h->d; k++) cur[k] = h->n[k];
  LineStep run[MD];
  int nr = 0;
  for (int k : h->up) if (k == g || h->m[k] != h->n[k]) run[nr++] = LineStep{k, h->mat(k, k == g ? 2 : 0), h->m[k]};
  hipError_t e = line_chain(h->d, cur, fields, 1, nr, run, x, image, h->tmp, st);
  if (e != hipSuccess) return chebhip_fail(CHEBHIP_ERR_DEVICE, "dealias launch: %s", hipGetErrorString(e));
  *res = nr ? image : x;
  return 0;
}

// direction l of the pairs in p (op[] and npairs set by the caller), then P down every direction into out
int dealias_finish(cheb_dealias *h, PairDir &p, bool a_shared, double *out, hipStream_t st) {
  const int l = h->l;
  long O = h->nf, Q = 1;
  for (int j = 0; j < l; j++) O *= h->m[j];
  for (int j = l + 1; j < h->d; j++) Q *= h->m[j];
  const int nd = (int)h->down.size();
  p.y = nd ? h->prod : out;
  p.O = (unsigned)O; p.K = (unsigned)h->n[l]; p.M = (unsigned)h->m[l]; p.Q = (unsigned)Q; p.L = (unsigned)(O * Q);
  p.La = a_shared ? p.L / (unsigned)h->nf : p.L;
  hipError_t e = pair_launch(p, st);
  if (e != hipSuccess) return chebhip_fail(CHEBHIP_ERR_DEVICE, "dealias pair launch: %s", hipGetErrorString(e));
  // the way down: stage s writes half s & 1 of the image buffer (nf * img values each: stage 0 shrinks direction l or something smaller)
  long cur[MD];
  for (int k = 0; k < h->d; k++) cur[k] = h->m[k];
  LineStep down[MD];
  for (int s = 0; s < nd; s++) down[s] = LineStep{h->down[s], h->mat(h->down[s], 1), h->n[h->down[s]]};
  double *const halves[2] = {h->image, h->image ? h->image + (size_t)h->nf * h->img : nullptr};
  e = line_chain(h->d, cur, h->nf, 1, nd, down, h->prod, out, halves, st);
  return e == hipSuccess ? 0 : chebhip_fail(CHEBHIP_ERR_DEVICE, "dealias launch: %s", hipGetErrorString(e));
}

}  // namespace

extern "C" int cheb_dealias_multiply(cheb_dealias *h, const double *u, const double *v, double *out, void *stream) {
  if (!h || !u || !v || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  const long N = h->nf * h->coarse;
  if (overlap(u, N, out, N) || overlap(v, N, out, N)) return chebhip_fail(CHEBHIP_ERR_ARG, "multiply: out must not overlap u or v");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  PairDir p{};
  p.npairs = 1;
  const double *ia, *ib;
  if ((rc = dealias_lift(h, u, h->nf, -1, h->image, &ia, st))) return rc;
  ib = ia;
  if (v != u && (rc = dealias_lift(h, v, h->nf, -1, h->image + (size_t)h->nf * h->img, &ib, st))) return rc;
  p.op[0] = PairOp{h->mat(h->l, 0), h->mat(h->l, 0), ia, ib};
  return dealias_finish(h, p, false, out, st);
}

extern "C" int cheb_dealias_advect(cheb_dealias *h, const double *vel, const double *c, double *out, void *stream) {
  if (!h || !vel || !c || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (!h->advect_ready) return chebhip_fail(CHEBHIP_ERR_ARG, "advect: call cheb_dealias_reserve_advect first");
  const long N = h->nf * h->coarse, NV = h->d * h->coarse;
  if (overlap(vel, NV, out, N) || overlap(c, N, out, N)) return chebhip_fail(CHEBHIP_ERR_ARG, "advect: out must not overlap vel or c");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  PairDir p{};
  p.npairs = h->d;
  // images: the d velocity components (one operand of d fields), then c with G in direction k, k = 0 .. d-1 (k == l: R everywhere,
  // G is the pair kernel's second matrix)
  const double *iv;
  if ((rc = dealias_lift(h, vel, h->d, -1, h->image, &iv, st))) return rc;
  for (int k = 0; k < h->d; k++) {
    const double *ic;
    double *slot = h->image ? h->image + ((size_t)h->d + (size_t)k * h->nf) * h->img : nullptr;
    if ((rc = dealias_lift(h, c, h->nf, k == h->l ? -1 : k, slot, &ic, st))) return rc;
    p.op[k] = PairOp{h->mat(h->l, 0), h->mat(h->l, k == h->l ? 2 : 0), iv + (size_t)k * h->img, ic};
  }
  return dealias_finish(h, p, true, out, st);
}
