// ops.h -- the plumbing every module of the library shares: the error-return macros around HIP calls, the launch check, the grid-stride
// loop and the launch size of the pointwise kernels, the argument checks of the handle constructors (check_field_grid: the toolbox
// modules' stacked full-grid fields) and their concatenated per-direction weight table, BoxGrid (the local box of an operator handle and
// which of its nodes lie on the boundary of the global grid), and what the preconditioner module (precond.hip) needs to see of the operator handles.
#pragma once
#include "../../include/chebhip.h"
#include "sweep.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>

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
// grad.hip: out[v * d + k] = u[v * d + k] + alpha s_k d_k s[v], one accumulating sweep each; out may be u (project.hip)
int cheb_grad_axpy_grad(cheb_grad *h, int nvec, double alpha, const double *s_dev, const double *u_dev, double *out_dev, void *stream);
// precond.hip, for the owner of a boundary-condition Helmholtz handle (varhelm.hip): the full-grid extension u_B = Q u_I + B_BB^-1 g
// on the caller's arrays (the one solve_bc ends with; g may be null), and a new shift sigma for the same lines (synchronous)
int helmholtz_extend(const cheb_helmholtz *h, const double *z_dev, const double *g_dev, double *u_dev, void *stream);
int helmholtz_set_sigma(cheb_helmholtz *h, double sigma);
const double *varhelm_kappa(const cheb_varhelm *h);          // varhelm.hip: the handle's copy of kappa (the first of its stacked copies), device [N]
size_t helmholtz_work_bytes(const cheb_helmholtz *h);        // device bytes the handle holds: field buffers, line matrices, eigenvalues
int chebhip_fail(int code, const char *fmt, ...);            // chebhip.hip: sets chebhip_last_error(), returns code

// A failed HIP call ends the calling function: `cleanup` runs, the error text is the call as written plus HIP's reason.
#define HIP_TRY_AS(expr, text, code, cleanup)                                                           \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) { cleanup; return chebhip_fail(code, "%s: %s", text, hipGetErrorString(e_)); } \
  } while (0)
#define HIP_TRY(expr) HIP_TRY_AS(expr, #expr, CHEBHIP_ERR_DEVICE, (void)0)
#define HIP_TRY_OR(expr, cleanup) HIP_TRY_AS(expr, #expr, CHEBHIP_ERR_DEVICE, cleanup)     // constructors: destroy the half-built handle
#define HIP_TRY_MEM_OR(expr, cleanup) HIP_TRY_AS(expr, #expr, e_ == hipErrorOutOfMemory ? CHEBHIP_ERR_MEMORY : CHEBHIP_ERR_DEVICE, cleanup)

// pointwise kernels: grid-stride loop, and the blocks of a launch that gives each block `per_block` items, at most `cap` blocks
#define GS_LOOP(i, n) for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

namespace chebhip {

inline unsigned grid1d(long n, long per_block, long cap) { const long g = (n + per_block - 1) / per_block; return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g)); }

// The local box of an operator handle: d extents in row-major order, of which dimension 0 may be the planes [lo, lo + dims[0]) of a
// global grid with gP0 planes (slab mode; otherwise lo = 0 and dims[0] = gP0).  Host only.
struct BoxGrid {
  int d = 0;
  std::vector<int> dims;            // local extents, boundary included
  int gP0 = 0, lo = 0;
  long N = 0;                       // local nodes

  static int check_slab(int lo, int hi, int P0) {
    return 0 <= lo && lo < hi && hi <= P0 ? 0 : chebhip_fail(CHEBHIP_ERR_ARG, "slab planes [%d, %d) outside 0..%d", lo, hi, P0);
  }
  // the planes [lo_, hi_) of the grid gdims
  void set_box(int d_, const int *gdims, int lo_, int hi_) {
    d = d_; dims.assign(gdims, gdims + d_); dims[0] = hi_ - lo_; gP0 = gdims[0]; lo = lo_;
    N = 1; for (int n : dims) N *= n;
  }
  // is the node with local multi-index ind a boundary node of the GLOBAL grid?
  bool boundary(const int *ind) const {
    const int g0 = ind[0] + lo;
    if (g0 == 0 || g0 == gP0 - 1) return true;
    for (int j = 1; j < d; j++) if (ind[j] == 0 || ind[j] == dims[j] - 1) return true;
    return false;
  }
  // f(l, ind, is_boundary) for every local node l in row-major (BlockIt) order
  template <class F> void for_each_node(F f) const {
    std::vector<int> ind(d, 0);
    for (long l = 0; l < N; l++) {
      f(l, (const int *)ind.data(), boundary(ind.data()));
      for (int j = d - 1; j >= 0; j--) { if (++ind[j] < dims[j]) break; ind[j] = 0; }
    }
  }
  // ixL[l]: the number of node l among the interior nodes, or -1 on the boundary; returns the number of interior nodes
  long interior_index(std::vector<int> &ixL) const {
    long g = 0;
    ixL.resize((size_t)N);
    for_each_node([&](long l, const int *, bool bdy) { ixL[l] = bdy ? -1 : (int)g++; });
    return g;
  }
  // lines along direction k: the stride between their points, and how many there are
  unsigned inner(int k) const { unsigned in = 1; for (int r = k + 1; r < d; r++) in *= dims[r]; return in; }
  unsigned ncols(int k) const { return (unsigned)(N / dims[k]); }
};

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

// d and nfields of a toolbox handle over `nfields` stacked full-grid fields of d directions (d_code: what a bad d is answered with)
inline int check_field_count(int d, const int *dims, int nfields, int d_code = CHEBHIP_ERR_DIMS) {
  if (!dims || d < 1 || d > 10) return chebhip_fail(d_code, "d = %d must be in 1..10", d);
  if (nfields < 1 || nfields > 16) return chebhip_fail(CHEBHIP_ERR_ARG, "nfields = %d must be in 1..16", nfields);
  return 0;
}

// The directions of such a handle, d and nfields checked: per direction its basis code (basis null: CGL everywhere), its extent, the cap
// of a periodic direction and the running product nfields * prod n_k < 2^31.  *values_per_field = prod n_k, *S = sum n_k (or null).
inline int check_field_extents(int d, const int *dims, const int *basis, int nfields, long *values_per_field, long *S) {
  int rc;
  long total = nfields, sum = 0;
  for (int k = 0; k < d; k++) {
    if (basis && basis[k] != CHEB_BASIS_CGL && basis[k] != CHEB_BASIS_FOURIER)
      return chebhip_fail(CHEBHIP_ERR_ARG, "basis[%d] = %d is neither 0 (CGL) nor 1 (Fourier)", k, basis[k]);
    if ((rc = check_extent(dims[k]))) return rc;
    if (basis && basis[k] == CHEB_BASIS_FOURIER && dims[k] > 256)
      return chebhip_fail(CHEBHIP_ERR_ARG, "dims[%d] = %d: a periodic direction supports at most 256 points", k, dims[k]);
    total *= dims[k]; sum += dims[k];
    if (total >= 0x80000000L) return chebhip_fail(CHEBHIP_ERR_DIMS, "2^31 values or more");
  }
  if (values_per_field) *values_per_field = total / nfields;
  if (S) *S = sum;
  return 0;
}

// d, nfields, then the directions (cheb_reduce_create and cheb_stats_check call the halves, with a check of their own between them)
inline int check_field_grid(int d, const int *dims, const int *basis, int nfields, long *values_per_field, long *S) {
  int rc;
  if ((rc = check_field_count(d, dims, nfields))) return rc;
  return check_field_extents(d, dims, basis, nfields, values_per_field, S);
}

// The concatenated per-direction table of such a grid (weights, rates, spectrum bins): direction k's n_k entries start at off[k]
template <class Off> void table_offsets(int d, const int *dims, Off *off) {
  for (int k = 0, o = 0; k < d; o += dims[k], k++) off[k] = (Off)o;
}
template <class Off>      // ... filled with every direction's Clenshaw-Curtis weights
std::vector<double> weight_table(int d, const int *dims, const Off *off, long S) {
  std::vector<double> w(S);
  for (int k = 0; k < d; k++) modal_weights_host(dims[k], w.data() + off[k]);
  return w;
}

// direction k's n entries of a device table, from the host; null: back to the Clenshaw-Curtis weights.  Synchronous.
inline int set_direction_weights(double *table, long off, int n, const double *w_host, const char *what) {
  std::vector<double> def;
  if (!w_host) { def.resize(n); modal_weights_host(n, def.data()); w_host = def.data(); }
  hipError_t e = hipMemcpy(table + off, w_host, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
  return e == hipSuccess ? 0 : chebhip_fail(CHEBHIP_ERR_MEMORY, "%s: %s", what, hipGetErrorString(e));
}

// after a kernel launch: counts it, and fails with "<what> launch: <hip reason>" if it was refused
inline int check_launch(const char *what) {
  sweep_note_launch();
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : chebhip_fail(CHEBHIP_ERR_DEVICE, "%s launch: %s", what, hipGetErrorString(e));
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
