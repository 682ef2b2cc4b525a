// linegemm.h -- the batched line product on the FP64 matrix cores that resample.hip (interpolation matrices) and modal.hip
// (Chebyshev transform and filter matrices) share: every line of a row-major tensor along one direction is multiplied by a
// dense M x K matrix R.
//
// In a direction of K -> M points the tensor is (O outer, K, Q inner) and every one of the L = O Q lines (o, q) -- element k at
// o K Q + k Q + q -- is multiplied by R.  A workgroup computes BM output points x 64 lines; R and the line image are
// staged in LDS by chunks of 16 points of the contracted index (a 1024-point R does not fit), the next chunk's loads in flight
// while the current one is multiplied.  Two tilings, selected by the stride Q of the contracted index:
//   Q > 4 (COLFAST): R is the A operand, the lines the B operand -- the 16 lanes of a quarter-wave load and store 16 neighbouring
//                    lines at one point (contiguous for Q >= 16);
//   Q <= 4 (the last direction, stride = ncomp): the lines are the A operand, R^T the B operand -- the 16 lanes of a quarter-wave
//                    load and store 16 consecutive points of one line.
// Both read the same LDS fragments (R[i][k] and X[k][line]); only the operand order of the MFMA and the meaning of the C/D
// rows and columns change.  C/D of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 reg.
//
// Everything here sits in an anonymous namespace: each translation unit that includes the header compiles its own copy of the
// kernel into its own code object (the library is built without relocatable device code), with internal linkage on both sides.
#pragma once
#include <hip/hip_runtime.h>
#include "sweep.h"

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
  chebhip::sweep_note_launch();
  return hipGetLastError();
}

[[maybe_unused]] hipError_t resample_launch(const ResampleDir &p, hipStream_t st) {
  if (p.L == 0) return hipSuccess;
  const bool la = p.Q <= 4;
  if (p.M > 64) return la ? launch_t<true, 128>(p, st) : launch_t<false, 128>(p, st);
  return la ? launch_t<true, 64>(p, st) : launch_t<false, 64>(p, st);
}

}  // namespace
