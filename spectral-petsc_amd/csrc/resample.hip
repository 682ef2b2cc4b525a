// resample.hip -- moves a field between two Chebyshev-Gauss-Lobatto grids (cheb_resample_*, include/chebhip.h): the tensor-product
// Lagrange interpolation Y = (R_0 (x) R_1 (x) ... (x) R_{d-1}) X of a row-major tensor with `ncomp` components innermost.
//
// One launch per direction that is not the identity, a batched GEMM on the FP64 matrix cores (linegemm.h, shared with modal.hip).
// The directions run in ascending order of n_out / n_in (shrinking ones first), which minimises the bytes of the intermediates;
// the handle owns the two ping-pong buffers they live in.
#include "../../include/chebhip.h"
#include "sweep.h"
#include "ops.h"
#include "linegemm.h"
#include <algorithm>
#include <new>
#include <vector>

using namespace chebhip;

namespace {

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
