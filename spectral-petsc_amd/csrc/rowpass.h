// rowpass.h -- what the one-pass reductions over stacked full-grid fields share (modal.hip, reduce.hip, stats.hip, points.hip): a
// row of n = n_{d-1} contiguous values is walked by LPR lanes (the power of two >= ceil(n / 2), at most 64), each lane taking the
// pairs (j, j + 1), j = 2 l, 2 l + 2 LPR, ....  The modules' folds of per-workgroup partial sums share their tiling (FOLD_PARTS, FOLD_OUT).
#pragma once
#include <hip/hip_runtime.h>

namespace chebhip {

typedef double d2 __attribute__((ext_vector_type(2)));      // (tile.h declares the same type for the sweep kernels)

namespace {

constexpr int FOLD_PARTS = 64, FOLD_OUT = 4;   // a fold's workgroup adds 4 results from 64 parts of the terms each

// the pair (j, j + 1) of a row; the second value is 0 past the end of the row
__device__ __forceinline__ d2 load_pair(const double *row, bool aligned, unsigned j, unsigned n) {
  if (aligned && j + 1 < n) return *reinterpret_cast<const d2 *>(row + j);
  d2 v; v.x = row[j]; v.y = j + 1 < n ? row[j + 1] : 0.0;
  return v;
}

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
  return s;
}

// log2 LPR of a row of n values
inline int row_lanes_lg(int n) {
  int lg = 0;
  while (lg < 6 && (1 << lg) < (n + 1) / 2) lg++;
  return lg;
}

}  // namespace
}  // namespace chebhip
