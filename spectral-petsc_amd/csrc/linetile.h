// linetile.h -- the workgroup tile of the batched line product on the FP64 matrix cores: what cheb_resample_kernel (linegemm.hip:
// one line image), cheb_pair_kernel (dealias.hip: two images side by side) and k_points_spread (points.hip: the image formed on
// chip, the contracted index a scattered point) share on the device.  Only those three units include it.
//
// In a direction of K -> M points the tensor is (O outer, K, Q inner) and every one of the L = O Q lines (o, q) -- element k at
// o K Q + k Q + q -- is multiplied by a dense M x K matrix R.  A workgroup computes BM output points x 64 lines; R and the line
// image are staged in LDS by chunks of 16 points of the contracted index (a 1024-point R does not fit), the next chunk's loads
// in flight while the current one is multiplied.  Two tilings, selected by the stride Q of the contracted index:
//   Q > 4 (COLFAST): R is the A operand, the lines the B operand -- the 16 lanes of a quarter-wave load and store 16 neighbouring
//                    lines at one point (contiguous for Q >= 16);
//   Q <= 4 (the last direction, stride = ncomp): the lines are the A operand, R^T the B operand -- the 16 lanes of a quarter-wave
//                    load and store 16 consecutive points of one line.
// Both read the same LDS fragments (R[i][k] and X[k][line]); only the operand order of the MFMA and the meaning of the C/D
// rows and columns change.  C/D of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 reg.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int RS_BN = 64;            // lines per workgroup tile
constexpr int RS_KC = 16;            // points of the contracted index per LDS chunk (4 k-steps)
constexpr int RS_XP = RS_BN + 16;    // pitch (doubles) of a row of the line image: the 4 rows a wave reads at once sit 128 B apart
constexpr int RS_RP = RS_KC + 2;     // pitch (doubles) of a row of the matrix chunk: 16 rows x 2 k of a half-wave on distinct banks

// LDS layout of a chunk: R[point][k] of a matrix chunk (BM * RS_RP doubles), X[k][line] of an image chunk (RS_KC * RS_XP doubles)
__device__ __forceinline__ int lds_r(int point, int k) { return point * RS_RP + k; }
__device__ __forceinline__ int lds_x(int k, int line) { return k * RS_XP + line; }

// one k-step of a 16 x 16 C/D tile from a lane's fragment elements r = R[point][k] and x = X[k][line]
template <bool LINES_A>
__device__ __forceinline__ v4d line_mfma(double r, double x, v4d acc) {
  return LINES_A ? __builtin_amdgcn_mfma_f64_16x16x4f64(x, r, acc, 0, 0, 0)    // (line x k) (k x point)
                 : __builtin_amdgcn_mfma_f64_16x16x4f64(r, x, acc, 0, 0, 0);   // (point x k) (k x line)
}

}  // namespace
