// resample.hip -- moves a field between two Chebyshev-Gauss-Lobatto grids (cheb_resample_*, include/chebhip.h): the tensor-product
// Lagrange interpolation Y = (R_0 (x) R_1 (x) ... (x) R_{d-1}) X of a row-major tensor with `ncomp` components innermost.
//
// One launch per direction that is not the identity, a batched GEMM on the FP64 matrix cores: in a direction of n_in -> n_out
// points the tensor is (O outer, K = n_in, Q inner) and every one of the L = O Q lines (o, q) -- element k at o K Q + k Q + q --
// is multiplied by the n_out x n_in matrix R.  A workgroup computes BM output points x 64 lines; R and the line image are
// staged in LDS by chunks of 16 points of the contracted index (a 1024-point R does not fit), the next chunk's loads in flight
// while the current one is multiplied.  Two tilings, selected by the stride Q of the contracted index:
//   Q > 4 (COLFAST): R is the A operand, the lines the B operand -- the 16 lanes of a quarter-wave load and store 16 neighbouring
//                    lines at one point (contiguous for Q >= 16);
//   Q <= 4 (the last direction, stride = ncomp): the lines are the A operand, R^T the B operand -- the 16 lanes of a quarter-wave
//                    load and store 16 consecutive points of one line.
// Both read the same LDS fragments (R[i][k] and X[k][line]); only the operand order of the MFMA and the meaning of the C/D
// rows and columns change.  C/D of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 reg.
// The directions run in ascending order of n_out / n_in (shrinking ones first), which minimises the bytes of the intermediates;
// the handle owns the two ping-pong buffers they live in.
#include "../../include/chebhip.h"
#include "sweep.h"
#include "ops.h"
#include <algorithm>
#include <new>
#include <vector>

using namespace chebhip;

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int RS_BN = 64;            // lines per workgroup tile
constexpr int RS_KC = 16;            // points of the contracted index per LDS chunk (4 k-steps)
constexpr int RS_XP = RS_BN + 16;    // pitch (doubles) of a row of the line image: the 4 rows a wave reads at once sit 128 B apart
constexpr int RS_RP = RS_KC + 2;     // pitch (doubles) of a row of the matrix chunk: 16 rows x 2 k of a half-wave on distinct banks

struct ResampleDir {
  const double *R;                   // n_out x n_in, row-major
  const double *x;
  double *y;
  unsigned O, K, M, Q, L;            // outer extent, n_in, n_out, stride of the contracted index, lines O Q
};

// LINES_A: the lines are the A operand (Q <= 4); BM = 64 or 128 output points per workgroup (4 waves as 2 x 2: BM/2 points x 32 lines each)
template <bool LINES_A, int BM>
__global__ __launch_bounds__(256) void cheb_resample_kernel(const ResampleDir p) {
  __shared__ double sR[BM * RS_RP];
  __shared__ double sX[RS_KC * RS_XP];
  constexpr int MT = BM / 32;                    // m-tiles of 16 points per wave
  constexpr int XN = RS_KC * RS_BN / 256;        // line-image elements a thread loads per chunk
  constexpr int RN = BM * RS_KC / 256;           // matrix elements a thread loads per chunk
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kq = lane >> 4, l16 = lane & 15;
  const int pw = (w >> 1) * (BM / 2), lw = (w & 1) * 32;     // this wave's first point / line within the tile
  const unsigned K = p.K, M = p.M, Q = p.Q, L = p.L;
  const unsigned l0 = blockIdx.x * RS_BN, i0 = blockIdx.y * BM;

  // what this thread loads: (point, line) of the image and (row, point) of the matrix, the same in every chunk
  unsigned xb[XN]; int xk[XN], xo[XN]; bool xl[XN];
#pragma unroll
  for (int e = 0; e < XN; e++) {
    const int t = tid + 256 * e;
    int kk, ll;
    if (LINES_A) { ll = t / RS_KC; kk = t % RS_KC; } else { kk = t / RS_BN; ll = t % RS_BN; }
    const unsigned line = l0 + ll, o = line / Q;
    xl[e] = line < L; xk[e] = kk; xo[e] = kk * RS_XP + ll;
    xb[e] = o * K * Q + (line - o * Q);
  }
  int rk[RN], ro[RN]; bool rl[RN]; unsigned rb[RN];
#pragma unroll
  for (int e = 0; e < RN; e++) {
    const int t = tid + 256 * e, ii = t / RS_KC, kk = t % RS_KC;
    rl[e] = i0 + ii < M; rk[e] = kk; ro[e] = ii * RS_RP + kk; rb[e] = (i0 + ii) * K;
  }
  double xv[XN], rv[RN];
  auto load = [&](unsigned k0) {
#pragma unroll
    for (int e = 0; e < XN; e++) { const unsigned k = k0 + xk[e]; xv[e] = (xl[e] && k < K) ? p.x[xb[e] + k * Q] : 0.0; }
#pragma unroll
    for (int e = 0; e < RN; e++) { const unsigned k = k0 + rk[e]; rv[e] = (rl[e] && k < K) ? p.R[rb[e] + k] : 0.0; }
  };

  v4d acc[MT][2];
#pragma unroll
  for (int u = 0; u < MT; u++)
#pragma unroll
    for (int t = 0; t < 2; t++) acc[u][t] = (v4d){0.0, 0.0, 0.0, 0.0};

  load(0);
  for (unsigned k0 = 0; k0 < K; k0 += RS_KC) {
    __syncthreads();                             // (the previous chunk has been read)
#pragma unroll
    for (int e = 0; e < XN; e++) sX[xo[e]] = xv[e];
#pragma unroll
    for (int e = 0; e < RN; e++) sR[ro[e]] = rv[e];
    __syncthreads();
    if (k0 + RS_KC < K) load(k0 + RS_KC);        // next chunk in flight during the products
#pragma unroll
    for (int ks = 0; ks < RS_KC / 4; ks++) {
      double a[MT], b[2];
#pragma unroll
      for (int u = 0; u < MT; u++) a[u] = sR[(pw + 16 * u + l16) * RS_RP + 4 * ks + kq];      // R[point][k]
#pragma unroll
      for (int t = 0; t < 2; t++) b[t] = sX[(4 * ks + kq) * RS_XP + lw + 16 * t + l16];       // X[k][line]
#pragma unroll
      for (int u = 0; u < MT; u++)
#pragma unroll
        for (int t = 0; t < 2; t++)
          acc[u][t] = LINES_A ? __builtin_amdgcn_mfma_f64_16x16x4f64(b[t], a[u], acc[u][t], 0, 0, 0)   // (line x k) (k x point)
                              : __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[t], acc[u][t], 0, 0, 0);  // (point x k) (k x line)
    }
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
        if (i < M) p.y[ob + i * Q] = acc[u][t][r];
      }
    }
}

template <bool LINES_A, int BM>
hipError_t launch_t(const ResampleDir &p, hipStream_t st) {
  const dim3 grid((p.L + RS_BN - 1) / RS_BN, (p.M + BM - 1) / BM);
  hipLaunchKernelGGL((cheb_resample_kernel<LINES_A, BM>), grid, dim3(256), 0, st, p);
  sweep_note_launch();
  return hipGetLastError();
}

hipError_t resample_launch(const ResampleDir &p, hipStream_t st) {
  if (p.L == 0) return hipSuccess;
  const bool la = p.Q <= 4;
  if (p.M > 64) return la ? launch_t<true, 128>(p, st) : launch_t<false, 128>(p, st);
  return la ? launch_t<true, 64>(p, st) : launch_t<false, 64>(p, st);
}

int require_device_rs() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return chebhip_fail(CHEBHIP_ERR_DEVICE, "no usable HIP device (%s); libchebhip has no CPU fallback",
                        e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  return 0;
}

int check_nodes(int n, int nodes, const char *what) {
  if (nodes != CHEB_NODES_ALL && nodes != CHEB_NODES_INTERIOR) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: node set %d is neither ALL nor INTERIOR", what, nodes);
  const int lo = nodes == CHEB_NODES_INTERIOR ? 3 : 2;
  if (n < lo) return chebhip_fail(CHEBHIP_ERR_SIZE, "%s: n = %d but must be >= %d", what, n, lo);
  if (n > 1024) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: n = %d: at most 1024 points per direction", what, n);
  return 0;
}

}  // namespace

struct cheb_resample {
  int d = 0, ncomp = 1;
  long n_in = 0, n_out = 0;                  // stored values (components included)
  struct Dir { double *R = nullptr; unsigned O = 0, K = 0, M = 0, Q = 0; };
  std::vector<Dir> dirs;                     // non-identity directions in the order they run
  double *work[2] = {nullptr, nullptr};      // ping-pong intermediates
};

extern "C" int cheb_resample_matrix_host(int n_in, int nodes_in, int n_out, int nodes_out, double *R) {
  int rc;
  if ((rc = check_nodes(n_in, nodes_in, "input")) || (rc = check_nodes(n_out, nodes_out, "output"))) return rc;
  if (!R) return chebhip_fail(CHEBHIP_ERR_ARG, "R is NULL");
  resample_matrix_host(n_in, nodes_in, n_out, nodes_out, R);
  return 0;
}

extern "C" int cheb_resample_destroy(cheb_resample *r) {
  if (!r) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  for (auto &dr : r->dirs) if (dr.R) (void)hipFree(dr.R);
  for (double *w : r->work) if (w) (void)hipFree(w);
  delete r;
  return 0;
}

extern "C" int cheb_resample_create(int d, const int *dims_in, int nodes_in, const int *dims_out, int nodes_out, int ncomp,
                                    cheb_resample **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (!dims_in || !dims_out || d < 1 || d > 10) return chebhip_fail(CHEBHIP_ERR_DIMS, "d = %d must be in 1..10", d);
  if (ncomp < 1 || ncomp > 4) return chebhip_fail(CHEBHIP_ERR_ARG, "ncomp = %d must be in 1..4", ncomp);
  int rc;
  const int a_in = nodes_in == CHEB_NODES_INTERIOR, a_out = nodes_out == CHEB_NODES_INTERIOR;
  long nin = ncomp, nout = ncomp;
  std::vector<long> kin(d), kout(d);                       // stored points per direction
  for (int k = 0; k < d; k++) {
    if ((rc = check_nodes(dims_in[k], nodes_in, "input")) || (rc = check_nodes(dims_out[k], nodes_out, "output"))) return rc;
    kin[k] = dims_in[k] - 2 * a_in; kout[k] = dims_out[k] - 2 * a_out;
    nin *= kin[k]; nout *= kout[k];
    if (nin >= 0x80000000L || nout >= 0x80000000L) return chebhip_fail(CHEBHIP_ERR_DIMS, "a field of 2^31 values or more");
  }
  if ((rc = require_device_rs())) return rc;
  cheb_resample *r = new (std::nothrow) cheb_resample;
  if (!r) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  r->d = d; r->ncomp = ncomp; r->n_in = nin; r->n_out = nout;

  // matrices; identity directions (equal grids) are dropped
  std::vector<int> order;
  std::vector<std::vector<double>> mats(d);
  for (int k = 0; k < d; k++) {
    mats[k].resize((size_t)kout[k] * kin[k]);
    resample_matrix_host(dims_in[k], a_in, dims_out[k], a_out, mats[k].data());
    bool ident = kin[k] == kout[k];
    for (long i = 0; ident && i < kout[k]; i++) ident = mats[k][(size_t)i * kin[k] + i] == 1.0;   // (unit rows: the rest is 0)
    if (!ident) order.push_back(k);
  }
  // shrinking directions first: every prefix product of n_out / n_in, hence every intermediate, is then as small as it can be
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return kout[a] * kin[b] < kout[b] * kin[a]; });
  std::vector<long> cur(kin);
  long wsz[2] = {0, 0};
  for (size_t s = 0; s < order.size(); s++) {
    const int k = order[s];
    cheb_resample::Dir dr;
    long O = 1, Q = ncomp;
    for (int j = 0; j < k; j++) O *= cur[j];
    for (int j = k + 1; j < d; j++) Q *= cur[j];
    dr.O = (unsigned)O; dr.K = (unsigned)kin[k]; dr.M = (unsigned)kout[k]; dr.Q = (unsigned)Q;
    cur[k] = kout[k];
    if (s + 1 < order.size()) { long &ws = wsz[s & 1]; ws = std::max(ws, O * kout[k] * Q); }
    hipError_t e = hipMalloc(&dr.R, mats[k].size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(dr.R, mats[k].data(), mats[k].size() * sizeof(double), hipMemcpyHostToDevice);
    r->dirs.push_back(dr);
    if (e != hipSuccess) { cheb_resample_destroy(r); return chebhip_fail(CHEBHIP_ERR_MEMORY, "resample matrix: %s", hipGetErrorString(e)); }
  }
  for (int b = 0; b < 2; b++)
    if (wsz[b] && hipMalloc(&r->work[b], wsz[b] * sizeof(double)) != hipSuccess) {
      cheb_resample_destroy(r);
      return chebhip_fail(CHEBHIP_ERR_MEMORY, "resample work buffer of %ld doubles", wsz[b]);
    }
  *out = r;
  return 0;
}

extern "C" long cheb_resample_size(const cheb_resample *r, int which) {
  if (!r || which < 0 || which > 1) return -1;
  return which ? r->n_out : r->n_in;
}

extern "C" int cheb_resample_apply(cheb_resample *r, const double *x, double *y, void *stream) {
  if (!r || !x || !y) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (x < y + r->n_out && y < x + r->n_in) return chebhip_fail(CHEBHIP_ERR_ARG, "x and y must not overlap");
  hipStream_t st = (hipStream_t)stream;
  const size_t nd = r->dirs.size();
  if (nd == 0) {
    hipError_t e = hipMemcpyAsync(y, x, r->n_in * sizeof(double), hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? 0 : chebhip_fail(CHEBHIP_ERR_DEVICE, "resample copy: %s", hipGetErrorString(e));
  }
  const double *src = x;
  for (size_t s = 0; s < nd; s++) {
    const auto &dr = r->dirs[s];
    double *dst = s + 1 == nd ? y : r->work[s & 1];
    ResampleDir p{dr.R, src, dst, dr.O, dr.K, dr.M, dr.Q, dr.O * dr.Q};
    hipError_t e = resample_launch(p, st);
    if (e != hipSuccess) return chebhip_fail(CHEBHIP_ERR_DEVICE, "resample launch: %s", hipGetErrorString(e));
    src = dst;
  }
  return 0;
}
