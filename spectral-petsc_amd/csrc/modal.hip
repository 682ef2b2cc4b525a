// modal.hip -- the modal side of the Chebyshev-Gauss-Lobatto grids (cheb_modal_*, include/chebhip.h): values <-> Chebyshev
// coefficients, modal filters, per-direction energy spectra and Clenshaw-Curtis quadrature of `nfields` stacked full-grid fields
// (field-major, row-major, all nodes: the layout of cheb_helmholtz_solve_bc's full-grid arrays).
//
// forward / backward / filter are tensor products of n x n matrices (diffmat.cpp: T, B, F = B diag(sigma) T): one launch of the
// line product of linegemm.hip per direction (line_chain), the fields as one more outer extent, intermediates in the handle's two ping-pong buffers.
//
// integrate and spectrum are one pass over the data each.  Both see a field as rpf = prod_{k < d-1} n_k rows of n = n_{d-1}
// contiguous values.  A row is walked by LPR lanes (the power of two >= ceil(n / 2), at most 64), each lane taking the pairs
// (j, j + 1), j = 2 l, 2 l + 2 LPR, ...: one 16-byte load where the row starts on a 16-byte boundary, two 8-byte loads where it
// does not (an odd n puts every other row, and an odd field size every other field, on an 8-byte boundary).  A wave takes
// 64 / LPR rows at a time.  Neither kernel uses atomics: a workgroup writes its partial sums to the handle's scratch array and
// k_modal_fold adds the workgroups' partials in a fixed order, so results are bit-reproducible from run to run.
#include "../../include/chebhip.h"
#include "sweep.h"
#include "ops.h"
#include "rowpass.h"
#include <algorithm>
#include <map>
#include <new>
#include <utility>
#include <vector>

using namespace chebhip;

namespace {

constexpr int MD = 10;               // directions
constexpr unsigned SPEC_CR = 8;      // k_modal_spectrum: rows per wave and step (at least; 64 / LPR if that is more)

struct ModalGeo {
  int d, lg;                         // directions; log2 LPR
  int n[MD], off[MD];                // extents; offset of direction k in the concatenated weight / spectrum arrays
  unsigned rpf, N, S;                // rows per field, values per field, sum of the extents
};

// indices (i_0 .. i_{d-2}) of row r of a field (DC: d known at compile time, 0: any d up to MD)
template <int DC>
__device__ __forceinline__ void row_index(const ModalGeo &g, unsigned r, int *i) {
  if (DC == 1) return;
  if (DC == 2) { i[0] = (int)r; return; }
  if (DC == 3) { const unsigned n1 = (unsigned)g.n[1]; i[0] = (int)(r / n1); i[1] = (int)(r - (r / n1) * n1); return; }
  for (int m = g.d - 2; m > 0; m--) { const unsigned nm = (unsigned)g.n[m]; i[m] = (int)(r % nm); r /= nm; }
  if (g.d > 1) i[0] = (int)r;
}

// partial[field][workgroup] = sum over the workgroup's rows of W u (v): field = blockIdx.y; workgroup b takes the rows
// (4 b + wave) RPW + group, then every gridDim.x 4 RPW-th.  The last direction's weights sit in LDS, a row's weight is the product
// of the other directions' (read through the cache: a wave's rows share all but the last of them).
template <int DC>
__global__ __launch_bounds__(256) void k_modal_integrate(const ModalGeo g, const double *__restrict__ w, const double *__restrict__ u,
                                                         const double *__restrict__ v, double *__restrict__ partial) {
  __shared__ double swl[1024];
  __shared__ double red[4];
  const int d = DC ? DC : g.d;
  const unsigned n = (unsigned)g.n[d - 1];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (unsigned j = tid; j < n; j += 256) swl[j] = w[g.off[d - 1] + j];
  __syncthreads();
  const unsigned lpr = 1u << g.lg, rpw = 64u >> g.lg, grp = (unsigned)lane >> g.lg, l = (unsigned)lane & (lpr - 1);
  const unsigned fo = blockIdx.y * g.N;
  double acc = 0.0;
  for (unsigned r = (blockIdx.x * 4 + wv) * rpw + grp; r < g.rpf; r += gridDim.x * 4 * rpw) {
    int i[MD];
    row_index<DC>(g, r, i);
    double wr = 1.0;
    for (int m = 0; m < (DC ? DC : MD) - 1; m++) if (m < d - 1) wr *= w[g.off[m] + i[m]];
    const double *pu = u + fo + r * n, *pv = v ? v + fo + r * n : nullptr;
    const bool au = ((size_t)pu & 15) == 0, av = ((size_t)pv & 15) == 0;
    double s = 0.0;
    for (unsigned j = 2 * l; j < n; j += 2 * lpr) {
      d2 a = load_pair(pu, au, j, n);
      if (pv) { const d2 b = load_pair(pv, av, j, n); a.x *= b.x; a.y *= b.y; }
      s += swl[j] * a.x + (j + 1 < n ? swl[j + 1] : 0.0) * a.y;
    }
    acc += wr * s;
  }
  acc = wave_sum(acc);
  if (lane == 0) red[wv] = acc;
  __syncthreads();
  if (tid == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// partial[field][workgroup][bin]: the workgroup's share of E[k][m] = sum of a^2 over every index but i_k = m, all k.  A step of
// the workgroup is 4 CR consecutive rows, CR = max(64 / LPR, 8) per wave.  A wave has 8, 8, 4, 2 rows in flight at a time for NIT = 1, 2, 4, 8, the
// pairs a lane takes of one row (1, 2, 4, 8 for rows of up to 128, 256, 512, 1024 points): all their loads are issued before the
// first square -- row after row, a wave would sit out one memory round trip per row.  Last direction: a lane adds the squares of
// its own points j in registers over all its rows; at the end the lane groups of a wave meet by shuffles and the four waves add
// into LDS one after the other.  Other directions: the sum of each row goes to LDS (rs) next to the row's indices (si); after a
// barrier the thread that owns bin m of direction k adds the rows with i_k = m in slot order.
template <int NIT>
__global__ __launch_bounds__(256) void k_modal_spectrum(const ModalGeo g, const double *__restrict__ a, unsigned nsteps, double *__restrict__ partial) {
  extern __shared__ double sm[];
  constexpr int RB = NIT == 1 ? 8 : 16 / NIT;
  const int d = g.d;
  double *bins = sm, *rs = sm + g.S;
  unsigned short *si = reinterpret_cast<unsigned short *>(rs + 256);     // [d - 1][256]
  const unsigned n = (unsigned)g.n[d - 1];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned lpr = 1u << g.lg, rpw = 64u >> g.lg, grp = (unsigned)lane >> g.lg, l = (unsigned)lane & (lpr - 1);
  const unsigned cr = rpw > SPEC_CR ? rpw : SPEC_CR, sr = 4 * cr, nq = cr / rpw;
  const unsigned fo = blockIdx.y * g.N;
  for (unsigned b = tid; b < g.S; b += 256) bins[b] = 0.0;
  double al[NIT][2];
#pragma unroll
  for (int it = 0; it < NIT; it++) al[it][0] = al[it][1] = 0.0;
  __syncthreads();

  for (unsigned step = blockIdx.x; step < nsteps; step += gridDim.x) {
    const unsigned r0 = step * sr;
    if ((unsigned)tid < sr) {
      const unsigned r = r0 + tid;
      int i[MD];
      if (r < g.rpf) row_index<0>(g, r, i);
      for (int m = 0; m < d - 1; m++) si[m * 256 + tid] = r < g.rpf ? (unsigned short)i[m] : (unsigned short)0xffff;
    }
    for (unsigned q0 = 0; q0 < nq; q0 += RB) {
      d2 x[RB][NIT];
#pragma unroll
      for (int b = 0; b < RB; b++) {
        const unsigned r = r0 + wv * cr + (q0 + b) * rpw + grp;
        const bool ok = q0 + b < nq && r < g.rpf;
        const double *pa = a + fo + (ok ? r * n : 0u);
        const bool aa = ((size_t)pa & 15) == 0;
#pragma unroll
        for (int it = 0; it < NIT; it++) {
          const unsigned j = 2 * l + 2 * lpr * it;
          x[b][it] = (d2){0.0, 0.0};
          if (ok && j < n) x[b][it] = load_pair(pa, aa, j, n);
        }
      }
#pragma unroll
      for (int b = 0; b < RB; b++) {
        double s = 0.0;
#pragma unroll
        for (int it = 0; it < NIT; it++) {
          const double e0 = x[b][it].x * x[b][it].x, e1 = x[b][it].y * x[b][it].y;
          al[it][0] += e0; al[it][1] += e1;
          s += e0 + e1;
        }
        for (unsigned m = 1; m < lpr; m <<= 1) s += __shfl_xor(s, (int)m);
        if (l == 0 && q0 + b < nq) rs[wv * cr + (q0 + b) * rpw + grp] = s;
      }
    }
    __syncthreads();
    for (int k = 0; k < d - 1; k++)
      for (unsigned m = tid; m < (unsigned)g.n[k]; m += 256) {
        double e = bins[g.off[k] + m];
#pragma unroll 8
        for (unsigned t = 0; t < sr; t++) e += si[k * 256 + t] == m ? rs[t] : 0.0;     // (no branch: the LDS reads of a group overlap)
        bins[g.off[k] + m] = e;
      }
    __syncthreads();
  }

  // last direction: lane groups of a wave by shuffles (masks LPR .. 32), then wave after wave
#pragma unroll
  for (int it = 0; it < NIT; it++)
    for (unsigned m = lpr; m < 64; m <<= 1) { al[it][0] += __shfl_xor(al[it][0], (int)m); al[it][1] += __shfl_xor(al[it][1], (int)m); }
  for (int q = 0; q < 4; q++) {
    if (wv == q && grp == 0) {
#pragma unroll
      for (int it = 0; it < NIT; it++) {
        const unsigned j = 2 * l + 2 * lpr * it;
        if (j < n) bins[g.off[d - 1] + j] += al[it][0];
        if (j + 1 < n) bins[g.off[d - 1] + j + 1] += al[it][1];
      }
    }
    __syncthreads();
  }
  double *out = partial + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * g.S;
  for (unsigned b = tid; b < g.S; b += 256) out[b] = bins[b];
}

// out[f][b] = sum over the gx workgroups of partial[f][workgroup][b], b < S: thread (part, b) adds the workgroups
// part, part + 64, ... in ascending order, then the 64 parts are added in ascending order.
__global__ __launch_bounds__(256) void k_modal_fold(const double *__restrict__ partial, unsigned gx, unsigned S, unsigned total, double *__restrict__ out) {
  __shared__ double sp[FOLD_PARTS][FOLD_OUT];
  const unsigned bl = threadIdx.x % FOLD_OUT, part = threadIdx.x / FOLD_OUT, t = blockIdx.x * FOLD_OUT + bl;
  double s = 0.0;
  if (t < total) {
    const unsigned f = t / S, b = t - f * S;
    const double *p = partial + (size_t)f * gx * S + b;
#pragma unroll 8
    for (unsigned x = part; x < gx; x += FOLD_PARTS) s += p[(size_t)x * S];
  }
  sp[part][bl] = s;
  __syncthreads();
  if (part == 0 && t < total) {
    s = sp[0][bl];
    for (int q = 1; q < FOLD_PARTS; q++) s += sp[q][bl];
    out[t] = s;
  }
}

}  // namespace

struct cheb_modal {
  int d = 0, nf = 1;
  long total = 0;                            // nf * prod(dims)
  ModalGeo geo{};
  int basis[MD] = {0};                       // BASIS_CGL / BASIS_FOURIER per direction (cheb_modal_create_basis)
  std::map<std::pair<int, int>, double *> mats;   // device: T then B (2 n^2 doubles) per distinct (extent, basis)
  double *F[MD] = {nullptr};                 // device filter matrix of a direction, or null: none set / all ones
  double *w = nullptr;                       // device: the directions' Clenshaw-Curtis weights, concatenated (geo.off)
  double *work[2] = {nullptr, nullptr};      // ping-pong intermediates
  double *partial = nullptr;                 // per-workgroup partial sums of integrate / spectrum
  unsigned gx_int = 1, gx_spec = 1, nsteps = 1;
  size_t lds_spec = 0;
};

extern "C" int cheb_modal_matrix_host(int n, int which, double *M) {
  int rc;
  if ((rc = check_extent(n))) return rc;
  if (which != 0 && which != 1) return chebhip_fail(CHEBHIP_ERR_ARG, "which = %d is neither 0 (forward) nor 1 (backward)", which);
  if (!M) return chebhip_fail(CHEBHIP_ERR_ARG, "M is NULL");
  modal_matrix_host(n, which, M);
  return 0;
}

extern "C" int cheb_modal_weights_host(int n, double *w) {
  int rc;
  if ((rc = check_extent(n))) return rc;
  if (!w) return chebhip_fail(CHEBHIP_ERR_ARG, "w is NULL");
  modal_weights_host(n, w);
  return 0;
}

extern "C" int cheb_modal_filter_matrix_host(int n, const double *sigma, double *F) {
  int rc;
  if ((rc = check_extent(n))) return rc;
  if (!sigma || !F) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  modal_filter_matrix_host(n, sigma, F);
  return 0;
}

extern "C" int cheb_modal_destroy(cheb_modal *h) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  for (auto &m : h->mats) if (m.second) (void)hipFree(m.second);
  for (double *f : h->F) if (f) (void)hipFree(f);
  for (double *b : h->work) if (b) (void)hipFree(b);
  if (h->w) (void)hipFree(h->w);
  if (h->partial) (void)hipFree(h->partial);
  delete h;
  return 0;
}

namespace {

// T (which = 0) / B (which = 1) of a periodic direction, long double rounded once (diffmat.cpp: fourier_modal_ld)
void fourier_modal_matrix(int n, int which, double *M) {
  std::vector<long double> A;
  fourier_modal_ld(n, which, A);
  for (size_t e = 0; e < A.size(); e++) M[e] = (double)A[e];
}

// F = B diag(sigma) T of a periodic direction, sigma per coefficient position, the sum in long double, rounded once.  (All ones never
// comes here: cheb_modal_set_filter drops such a direction from the filter, which is what makes it the identity exactly.)
void fourier_filter_matrix(int n, const double *sigma, double *F) {
  std::vector<long double> B, T;
  fourier_modal_ld(n, 1, B);
  fourier_modal_ld(n, 0, T);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      long double s = 0.0L;
      for (int p = 0; p < n; p++) if (sigma[p] != 0.0) s += B[(size_t)i * n + p] * (long double)sigma[p] * T[(size_t)p * n + j];
      F[(size_t)i * n + j] = (double)s;
    }
}

}  // namespace

// basis[k]: BASIS_CGL or BASIS_FOURIER (2 <= n <= 256; the coefficient layout is the parity mode layout of cheb_fourier_modes_host,
// the quadrature weight 2 / n at every node); null: CGL everywhere, which is cheb_modal_create
static int modal_create(int d, const int *dims, int nfields, const int *basis, cheb_modal **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  int rc;
  long N = 0, S = 0;
  if ((rc = check_field_grid(d, dims, basis, nfields, &N, &S))) return rc;
  if ((rc = require_device())) return rc;
  const long total = nfields * N;
  cheb_modal *h = new (std::nothrow) cheb_modal;
  if (!h) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  h->d = d; h->nf = nfields; h->total = total;
  ModalGeo &g = h->geo;
  g.d = d; g.S = (unsigned)S; g.N = (unsigned)N;
  const int n = dims[d - 1];
  g.rpf = g.N / (unsigned)n;
  g.lg = row_lanes_lg(n);
  table_offsets(d, dims, g.off);
  std::vector<double> w = weight_table(d, dims, g.off, S);
  for (int k = 0; k < d; k++) {
    g.n[k] = dims[k]; h->basis[k] = basis ? basis[k] : BASIS_CGL;
    if (h->basis[k] == BASIS_FOURIER) for (int j = 0; j < dims[k]; j++) w[g.off[k] + j] = (double)(2.0L / (long double)dims[k]);
  }

  // launch geometry of the two reductions, fixed per handle: results do not depend on anything but the shape
  const unsigned rpw = 64u >> g.lg, cr = rpw > SPEC_CR ? rpw : SPEC_CR, sr = 4 * cr, cap_int = 2048u / nfields, cap_spec = 1024u / nfields;
  h->gx_int = std::max(1u, std::min(cap_int, (g.rpf + 4 * rpw - 1) / (4 * rpw)));
  h->nsteps = (g.rpf + sr - 1) / sr;
  h->gx_spec = std::max(1u, std::min(cap_spec, h->nsteps));
  h->lds_spec = ((size_t)S + 256) * sizeof(double) + (size_t)(d > 1 ? d - 1 : 1) * 256 * sizeof(unsigned short);
  if (h->lds_spec > 64 * 1024) { delete h; return chebhip_fail(CHEBHIP_ERR_DIMS, "extents sum to %ld: the spectrum's bins do not fit in LDS", S); }
  const size_t npart = std::max((size_t)nfields * h->gx_int, (size_t)nfields * h->gx_spec * S);

  std::vector<double> m;
  for (int k = 0; k < d && !rc; k++) {
    const int nk = dims[k];
    const std::pair<int, int> key(nk, h->basis[k]);
    if (h->mats.count(key)) continue;
    const size_t nn = (size_t)nk * nk;
    m.resize(2 * nn);
    if (h->basis[k] == BASIS_FOURIER) { fourier_modal_matrix(nk, 0, m.data()); fourier_modal_matrix(nk, 1, m.data() + nn); }
    else { modal_matrix_host(nk, 0, m.data()); modal_matrix_host(nk, 1, m.data() + nn); }
    double *dev = nullptr;
    if (!(rc = device_array(&dev, 2 * nn, m.data(), "modal matrices"))) h->mats[key] = dev;
  }
  if (!rc) rc = device_array(&h->w, S, w.data(), "quadrature weights");
  for (int b = 0; b < 2 && b < d - 1 && !rc; b++) rc = device_array(&h->work[b], total, nullptr, "modal work buffer");
  if (!rc) rc = device_array(&h->partial, npart, nullptr, "modal partial sums");
  if (rc) { cheb_modal_destroy(h); return rc; }
  *out = h;
  return 0;
}

extern "C" int cheb_modal_create(int d, const int *dims, int nfields, cheb_modal **out) { return modal_create(d, dims, nfields, nullptr, out); }

extern "C" int cheb_modal_create_basis(int d, const int *dims, int nfields, const int *basis, cheb_modal **out) {
  if (out) *out = nullptr;
  if (!basis) return chebhip_fail(CHEBHIP_ERR_ARG, "basis is NULL");
  return modal_create(d, dims, nfields, basis, out);
}

extern "C" long cheb_modal_size(const cheb_modal *h) { return h ? h->total : -1; }
extern "C" long cheb_modal_spectrum_size(const cheb_modal *h) { return h ? (long)h->nf * h->geo.S : -1; }

namespace {

// y = (M_0 (x) ... (x) M_{d-1}) x over the directions with a matrix (null: identity), one launch each, the last one into y
int modal_product(cheb_modal *h, const double *const *M, const double *x, double *y, void *stream, const char *what) {
  if (!h || !x || !y) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (overlap(x, h->total, y, h->total)) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: input and output must not overlap", what);
  hipStream_t st = (hipStream_t)stream;
  LineStep steps[MD];
  long cur[MD];
  int nd = 0;
  for (int k = 0; k < h->d; k++) {
    cur[k] = h->geo.n[k];
    if (M[k]) steps[nd++] = LineStep{k, M[k], h->geo.n[k]};
  }
  if (nd == 0) {
    hipError_t e = hipMemcpyAsync(y, x, h->total * sizeof(double), hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? 0 : chebhip_fail(CHEBHIP_ERR_DEVICE, "%s copy: %s", what, hipGetErrorString(e));
  }
  hipError_t e = line_chain(h->d, cur, h->nf, 1, nd, steps, x, y, h->work, st);
  return e == hipSuccess ? 0 : chebhip_fail(CHEBHIP_ERR_DEVICE, "%s launch: %s", what, hipGetErrorString(e));
}

int modal_transform(cheb_modal *h, int which, const double *x, double *y, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  const double *M[MD];
  for (int k = 0; k < h->d; k++) M[k] = h->mats[std::make_pair(h->geo.n[k], h->basis[k])] + (which ? (size_t)h->geo.n[k] * h->geo.n[k] : 0);
  return modal_product(h, M, x, y, stream, which ? "backward" : "forward");
}

}  // namespace

extern "C" int cheb_modal_forward(cheb_modal *h, const double *u, double *a, void *stream) { return modal_transform(h, 0, u, a, stream); }
extern "C" int cheb_modal_backward(cheb_modal *h, const double *a, double *u, void *stream) { return modal_transform(h, 1, a, u, stream); }

extern "C" int cheb_modal_set_filter(cheb_modal *h, int k, const double *sigma) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (k < 0 || k >= h->d) return chebhip_fail(CHEBHIP_ERR_TDIM, "direction %d out of range 0..%d", k, h->d - 1);
  const int n = h->geo.n[k];
  bool ones = true;
  for (int m = 0; sigma && m < n; m++) ones = ones && sigma[m] == 1.0;
  if (ones) {                                                  // cleared or all ones: the direction drops out of filter
    if (h->F[k]) { (void)hipFree(h->F[k]); h->F[k] = nullptr; }
    return 0;
  }
  std::vector<double> F((size_t)n * n);
  if (h->basis[k] == BASIS_FOURIER) fourier_filter_matrix(n, sigma, F.data());
  else modal_filter_matrix_host(n, sigma, F.data());
  hipError_t e = h->F[k] ? hipSuccess : hipMalloc(&h->F[k], F.size() * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(h->F[k], F.data(), F.size() * sizeof(double), hipMemcpyHostToDevice);
  return e == hipSuccess ? 0 : chebhip_fail(CHEBHIP_ERR_MEMORY, "filter matrix: %s", hipGetErrorString(e));
}

extern "C" int cheb_modal_filter(cheb_modal *h, const double *u, double *v, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  return modal_product(h, h->F, u, v, stream, "filter");
}

static int modal_fold(cheb_modal *h, unsigned gx, unsigned S, double *out, hipStream_t st, const char *what) {
  const unsigned total = (unsigned)h->nf * S;
  hipLaunchKernelGGL(k_modal_fold, dim3((total + FOLD_OUT - 1) / FOLD_OUT), dim3(256), 0, st, h->partial, gx, S, total, out);
  return check_launch(what);
}

extern "C" int cheb_modal_integrate(cheb_modal *h, const double *u, const double *v, double *out, void *stream) {
  if (!h || !u || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(h->gx_int, (unsigned)h->nf);
#define MODAL_INT(DC) hipLaunchKernelGGL(k_modal_integrate<DC>, grid, dim3(256), 0, st, h->geo, h->w, u, v, h->partial)
  switch (h->d) { case 1: MODAL_INT(1); break; case 2: MODAL_INT(2); break; case 3: MODAL_INT(3); break; default: MODAL_INT(0); }
#undef MODAL_INT
  int rc;
  if ((rc = check_launch("integrate"))) return rc;
  return modal_fold(h, h->gx_int, 1, out, st, "integrate");
}

extern "C" int cheb_modal_spectrum(cheb_modal *h, const double *a, double *E, void *stream) {
  if (!h || !a || !E) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(h->gx_spec, (unsigned)h->nf);
#define MODAL_SPEC(NIT) hipLaunchKernelGGL(k_modal_spectrum<NIT>, grid, dim3(256), h->lds_spec, st, h->geo, a, h->nsteps, h->partial)
  const int n = h->geo.n[h->d - 1];                            // pairs of a row per lane: ceil(n / 2 LPR), LPR = 64 from n = 65 on
  if (n <= 128) MODAL_SPEC(1); else if (n <= 256) MODAL_SPEC(2); else if (n <= 512) MODAL_SPEC(4); else MODAL_SPEC(8);
#undef MODAL_SPEC
  int rc;
  if ((rc = check_launch("spectrum"))) return rc;
  return modal_fold(h, h->gx_spec, h->geo.S, E, st, "spectrum");
}
