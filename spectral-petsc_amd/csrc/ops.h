// ops.h -- what the preconditioner module (precond.hip) needs to see of the operator handles, and the plumbing that the
// handle modules share (chebhip.hip, resample.hip, modal.hip, points.hip, dealias.hip, reduce.hip).
#pragma once
#include "../../include/chebhip.h"
#include <hip/hip_runtime.h>
#include <algorithm>

namespace chebhip {

// Grid and coefficient state of an operator: everything FormJacobian (elliptic.C:537-590) / StokesPCSetUp0
// (stokes.C:1160-1241) read.  Pointers are device pointers owned by the operator; gradu may be null (Stokes).
struct FdView {
  int d = 0;
  const int *dims = nullptr;      // host, d extents of the local grid (boundary included)
  long N = 0, G = 0;              // local nodes, interior nodes
  const int *ixL = nullptr;       // device [N]: interior index or -1
  const double *eta = nullptr, *deta = nullptr;     // device [N]
  const double *gradu[10] = {nullptr};              // device [N] each, or null: no deta * du0 terms
};

}  // namespace chebhip

int ell_op_sync_coeffs(ell_op *op, void *stream);            // chebhip.hip: makes eta / deta current before the view's arrays are read
int ell_op_fd_view(ell_op *op, chebhip::FdView *v);          // chebhip.hip (allocates the coefficient state if needed)
// the same for slab-mode handles too (precond.hip's slab mode; *gP0: global extent of dimension 0, v->dims[0]: planes of the slab)
int ell_op_fd_view_any(ell_op *op, chebhip::FdView *v, int *gP0);
int stokes_op_fd_view_any(stokes_op *op, chebhip::FdView *v, int *gP0);
int stokes_op_fd_view(stokes_op *op, chebhip::FdView *v);    // stokes.hip
int chebhip_fail(int code, const char *fmt, ...);            // chebhip.hip

namespace chebhip {

inline int require_device() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return chebhip_fail(CHEBHIP_ERR_DEVICE, "no usable HIP device (%s); libchebhip has no CPU fallback",
                        e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  return 0;
}

// the extent of one direction of a full Chebyshev-Gauss-Lobatto grid
inline int check_extent(int n) {
  if (n < 2) return chebhip_fail(CHEBHIP_ERR_SIZE, "n = %d but must be >= 2", n);
  if (n > 1024) return chebhip_fail(CHEBHIP_ERR_ARG, "n = %d: at most 1024 points per direction", n);
  return 0;
}

inline bool overlap(const double *a, long na, const double *b, long nb) { return a < b + nb && b < a + na; }

// *dev = n doubles on the device, filled from `host` unless that is null; on failure *dev is null and the error is set
inline int device_array(double **dev, size_t n, const double *host, const char *what) {
  hipError_t e = hipMalloc(dev, n * sizeof(double));
  if (e != hipSuccess) *dev = nullptr;
  else if (host && (e = hipMemcpy(*dev, host, n * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) { (void)hipFree(*dev); *dev = nullptr; }
  return e == hipSuccess ? 0 : chebhip_fail(CHEBHIP_ERR_MEMORY, "%s: %s", what, hipGetErrorString(e));
}

// directions first..last in ascending order of out[k] / in[k], ties in their given order.  A chain of line products that runs its
// shrinking directions first keeps every prefix product of out / in, hence every intermediate, as small as it can be.
template <class Out, class In>
void order_by_ratio(int *first, int *last, const Out &out, const In &in) {
  std::stable_sort(first, last, [&](int a, int b) { return (long)out[a] * in[b] < (long)out[b] * in[a]; });
}

}  // namespace chebhip
