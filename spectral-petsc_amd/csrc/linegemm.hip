// linegemm.hip -- the batched line product on the FP64 matrix cores that resample.hip (interpolation matrices), modal.hip
// (Chebyshev transform and filter matrices), points.hip (barycentric rows) and dealias.hip (the 3/2 rule's matrices) share, and
// the host driver of a chain of such products, one direction after the other.  The tiling is described in linetile.h; this is
// the only unit that compiles cheb_resample_kernel.
#include "sweep.h"
#include "linetile.h"

namespace chebhip {

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
    xl[e] = line < L; xk[e] = kk; xo[e] = lds_x(kk, ll);
    xb[e] = o * K * Q + (line - o * Q);
  }
  int rk[RN], ro[RN]; bool rl[RN]; unsigned rb[RN];
#pragma unroll
  for (int e = 0; e < RN; e++) {
    const int t = tid + 256 * e, ii = t / RS_KC, kk = t % RS_KC;
    rl[e] = i0 + ii < M; rk[e] = kk; ro[e] = lds_r(ii, kk); rb[e] = (i0 + ii) * K;
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
      for (int u = 0; u < MT; u++) a[u] = sR[lds_r(pw + 16 * u + l16, 4 * ks + kq)];
#pragma unroll
      for (int t = 0; t < 2; t++) b[t] = sX[lds_x(4 * ks + kq, lw + 16 * t + l16)];
#pragma unroll
      for (int u = 0; u < MT; u++)
#pragma unroll
        for (int t = 0; t < 2; t++) acc[u][t] = line_mfma<LINES_A>(a[u], b[t], acc[u][t]);
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
static hipError_t launch_t(const ResampleDir &p, hipStream_t st) {
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

hipError_t line_chain(int d, long *cur, long outer, long inner, int nsteps, const LineStep *steps, const double *src, double *dst,
                      double *const *work, hipStream_t st) {
  for (int s = 0; s < nsteps; s++) {
    const int k = steps[s].dir;
    long O = outer, Q = inner;
    for (int j = 0; j < k; j++) O *= cur[j];
    for (int j = k + 1; j < d; j++) Q *= cur[j];
    double *out = s + 1 == nsteps ? dst : work[s & 1];
    const ResampleDir p{steps[s].R, src, out, (unsigned)O, (unsigned)cur[k], (unsigned)steps[s].m, (unsigned)Q, (unsigned)(O * Q)};
    const hipError_t e = resample_launch(p, st);
    if (e != hipSuccess) return e;
    cur[k] = steps[s].m;
    src = out;
  }
  return hipSuccess;
}

}  // namespace chebhip
