// resample.hip -- moves a field between two Chebyshev-Gauss-Lobatto grids (cheb_resample_*, include/chebhip.h): the tensor-product
// Lagrange interpolation Y = (R_0 (x) R_1 (x) ... (x) R_{d-1}) X of a row-major tensor with `ncomp` components innermost.
//
// One launch per direction that is not the identity, a batched GEMM on the FP64 matrix cores (line_chain, linegemm.hip).
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
  std::vector<long> kin;                     // stored points per direction of the input
  std::vector<LineStep> steps;               // non-identity directions in the order they run; the handle owns their matrices
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
  for (auto &st : r->steps) if (st.R) (void)hipFree(const_cast<double *>(st.R));
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
  if ((rc = require_device())) return rc;
  cheb_resample *r = new (std::nothrow) cheb_resample;
  if (!r) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  r->d = d; r->ncomp = ncomp; r->n_in = nin; r->n_out = nout; r->kin = kin;

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
  order_by_ratio(order.data(), order.data() + order.size(), kout, kin);
  long len = nin, wsz[2] = {0, 0};           // stage s of a chain writes work[s & 1], the last one y
  for (size_t s = 0; s < order.size(); s++) {
    const int k = order[s];
    len = len / kin[k] * kout[k];
    if (s + 1 < order.size()) wsz[s & 1] = std::max(wsz[s & 1], len);
    double *R = nullptr;
    if ((rc = device_array(&R, mats[k].size(), mats[k].data(), "resample matrix"))) { cheb_resample_destroy(r); return rc; }
    r->steps.push_back(LineStep{k, R, (int)kout[k]});
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
  if (overlap(x, r->n_in, y, r->n_out)) return chebhip_fail(CHEBHIP_ERR_ARG, "x and y must not overlap");
  hipStream_t st = (hipStream_t)stream;
  if (r->steps.empty()) {
    hipError_t e = hipMemcpyAsync(y, x, r->n_in * sizeof(double), hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? 0 : chebhip_fail(CHEBHIP_ERR_DEVICE, "resample copy: %s", hipGetErrorString(e));
  }
  long cur[10];
  std::copy(r->kin.begin(), r->kin.end(), cur);
  hipError_t e = line_chain(r->d, cur, 1, r->ncomp, (int)r->steps.size(), r->steps.data(), x, y, r->work, st);
  return e == hipSuccess ? 0 : chebhip_fail(CHEBHIP_ERR_DEVICE, "resample launch: %s", hipGetErrorString(e));
}
