// layout.hip -- the way between the operators' vectors and the full-grid, field-major fields of the toolbox (cheb_layout_*,
// include/chebhip.h).  ell_op and stokes_op speak the reference's vectors: interior nodes only, node-major, the components of a node
// interleaved (stride si, first component at offset oi), with the Dirichlet values of the boundary nodes in a compact array of their
// own in BlockIt (row-major) order (stride sb, offset ob).  cheb_modal_*, cheb_points_*, cheb_reduce_*, cheb_grad_* want all nodes,
// one field after the other.  The handle owns one int per node: map[l] >= 0 is the node's number among the interior nodes, map[l] < 0
// is -1 - (its number among the boundary nodes); both counted row-major, by the node walk every operator handle uses (BoxGrid).
//
// Two grid-stride kernels, one node per lane, the components in a loop: the field side is coalesced, the interleaved side is read or
// written with the stride of its vector.  Values are moved, never computed: every bit arrives.
#include "../../include/chebhip.h"
#include "sweep.h"
#include "ops.h"
#include <new>
#include <vector>

using namespace chebhip;

namespace {

// out[c * N + l] = interior ? xi[m * si + oi + c] : xb[b * sb + ob + c]; a NULL source gives 0
__global__ __launch_bounds__(256) void k_layout_unpack(long N, const int *__restrict__ map, int ncomp, const double *__restrict__ xi, long si,
                                                       long oi, const double *__restrict__ xb, long sb, long ob, double *__restrict__ out) {
  GS_LOOP(l, N) {
    const int m = map[l];
    const double *src = m >= 0 ? xi : xb;
    const size_t base = m >= 0 ? (size_t)m * si + oi : (size_t)(-1 - m) * sb + ob;
    for (int c = 0; c < ncomp; c++) out[(size_t)c * N + l] = src ? src[base + c] : 0.0;
  }
}

// the inverse: a NULL target is skipped, entries of the targets that no (node, component) addresses are not touched
__global__ __launch_bounds__(256) void k_layout_pack(long N, const int *__restrict__ map, int ncomp, const double *__restrict__ fields,
                                                     double *__restrict__ xi, long si, long oi, double *__restrict__ xb, long sb, long ob) {
  GS_LOOP(l, N) {
    const int m = map[l];
    double *dst = m >= 0 ? xi : xb;
    if (!dst) continue;
    const size_t base = m >= 0 ? (size_t)m * si + oi : (size_t)(-1 - m) * sb + ob;
    for (int c = 0; c < ncomp; c++) dst[base + c] = fields[(size_t)c * N + l];
  }
}

int check_strides(const char *what, int ncomp, const void *pi, long si, long oi, const void *pb, long sb, long ob) {
  if (ncomp < 1) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: ncomp = %d must be >= 1", what, ncomp);
  if (pi && (oi < 0 || oi + ncomp > si)) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: interior offset %ld + %d components exceed the stride %ld", what, oi, ncomp, si);
  if (pb && (ob < 0 || ob + ncomp > sb)) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: boundary offset %ld + %d components exceed the stride %ld", what, ob, ncomp, sb);
  return 0;
}

int check_grid(int d, const int *dims, long *N_out) {
  if (!dims || d < 1 || d > 10) return chebhip_fail(CHEBHIP_ERR_DIMS, "d = %d must be in 1..10", d);
  long N = 1;
  for (int k = 0; k < d; k++) {
    if (dims[k] < 3) return chebhip_fail(CHEBHIP_ERR_SIZE, "dims[%d] = %d but must be >= 3: a line needs an interior node", k, dims[k]);
    if (dims[k] > 1024) return chebhip_fail(CHEBHIP_ERR_ARG, "dims[%d] = %d: at most 1024 points per direction", k, dims[k]);
    N *= dims[k];
    if (N >= 0x80000000L) return chebhip_fail(CHEBHIP_ERR_DIMS, "2^31 nodes or more");
  }
  *N_out = N;
  return 0;
}

}  // namespace

struct cheb_layout {
  long N = 0, I = 0;
  int *map = nullptr;      // device [N]
};

extern "C" int cheb_layout_destroy(cheb_layout *h) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (h->map) (void)hipFree(h->map);
  delete h;
  return 0;
}

// map[l] of every node of the grid, on the host (no device needed): the table cheb_layout_create uploads
extern "C" int cheb_layout_map_host(int d, const int *dims, int *map) {
  int rc; long N;
  if ((rc = check_grid(d, dims, &N))) return rc;
  if (!map) return chebhip_fail(CHEBHIP_ERR_ARG, "map is NULL");
  BoxGrid box;
  box.set_box(d, dims, 0, dims[0]);
  int g = 0, b = 0;
  box.for_each_node([&](long l, const int *, bool bdy) { map[l] = bdy ? -1 - b++ : g++; });
  return 0;
}

extern "C" int cheb_layout_create(int d, const int *dims, cheb_layout **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  int rc; long N;
  if ((rc = check_grid(d, dims, &N))) return rc;
  if ((rc = require_device())) return rc;
  std::vector<int> map((size_t)N);
  if ((rc = cheb_layout_map_host(d, dims, map.data()))) return rc;
  cheb_layout *h = new (std::nothrow) cheb_layout;
  if (!h) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  h->N = N;
  h->I = 1;
  for (int k = 0; k < d; k++) h->I *= dims[k] - 2;
  HIP_TRY_OR(hipMalloc((void **)&h->map, (size_t)N * sizeof(int)), cheb_layout_destroy(h));
  HIP_TRY_OR(hipMemcpy(h->map, map.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice), cheb_layout_destroy(h));
  *out = h;
  return 0;
}

extern "C" long cheb_layout_size(const cheb_layout *h, int which) {
  if (!h || which < 0 || which > 2) return -1;
  return which == 0 ? h->N : which == 1 ? h->I : h->N - h->I;
}

extern "C" int cheb_layout_unpack(cheb_layout *h, int ncomp, const double *xi_dev, long si, long oi, const double *xb_dev, long sb, long ob,
                                  double *out_dev, void *stream) {
  int rc;
  if ((rc = check_strides("unpack", ncomp, xi_dev, si, oi, xb_dev, sb, ob))) return rc;
  if (!h || !out_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "unpack: NULL handle or output");
  if ((long)ncomp * h->N >= 0x80000000L) return chebhip_fail(CHEBHIP_ERR_DIMS, "unpack: 2^31 values or more");
  const long nout = (long)ncomp * h->N;
  if ((xi_dev && overlap(out_dev, nout, xi_dev, h->I * si)) || (xb_dev && overlap(out_dev, nout, xb_dev, (h->N - h->I) * sb)))
    return chebhip_fail(CHEBHIP_ERR_ARG, "unpack: the output must not overlap a source");
  hipLaunchKernelGGL(k_layout_unpack, dim3(grid1d(h->N, 256, 4096)), dim3(256), 0, (hipStream_t)stream, h->N, h->map, ncomp, xi_dev, si, oi,
                     xb_dev, sb, ob, out_dev);
  sweep_note_launch();
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int cheb_layout_pack(cheb_layout *h, int ncomp, const double *fields_dev, double *xi_dev, long si, long oi, double *xb_dev, long sb,
                                long ob, void *stream) {
  int rc;
  if ((rc = check_strides("pack", ncomp, xi_dev, si, oi, xb_dev, sb, ob))) return rc;
  if (!h || !fields_dev) return chebhip_fail(CHEBHIP_ERR_ARG, "pack: NULL handle or fields");
  if ((long)ncomp * h->N >= 0x80000000L) return chebhip_fail(CHEBHIP_ERR_DIMS, "pack: 2^31 values or more");
  const long nin = (long)ncomp * h->N;
  if ((xi_dev && overlap(fields_dev, nin, xi_dev, h->I * si)) || (xb_dev && overlap(fields_dev, nin, xb_dev, (h->N - h->I) * sb)))
    return chebhip_fail(CHEBHIP_ERR_ARG, "pack: the fields must not overlap a target");
  hipLaunchKernelGGL(k_layout_pack, dim3(grid1d(h->N, 256, 4096)), dim3(256), 0, (hipStream_t)stream, h->N, h->map, ncomp, fields_dev, xi_dev,
                     si, oi, xb_dev, sb, ob);
  sweep_note_launch();
  HIP_TRY(hipGetLastError());
  return 0;
}
