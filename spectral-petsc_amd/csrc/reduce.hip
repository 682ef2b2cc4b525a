// reduce.hip -- partial contractions of `nfields` stacked full-grid fields (cheb_reduce_*, include/chebhip.h; field-major, row-major,
// all nodes: the layout of cheb_modal_*): a subset of the directions of u, or of the product u v, is summed against one weight
// vector per contracted direction, the other directions are kept:
//     out[f][kept indices] = sum over the contracted indices of prod_{k contracted} w_k[i_k] u[f][i] (v[f][i]).
// Mean profiles, plane-averaged fluxes, face values and wall fluxes (a row of D as the weights), marginals.
//
// The offset of a value splits into a part of the kept indices and a part of the contracted ones, so the general case (any mask
// over up to 10 directions) is two mixed-radix decodes: of the output index o into the kept GROUPS (neighbouring kept directions
// merged into one extent and one stride), and of the contracted index c into the contracted directions (one by one: each index
// also selects a weight).  Directions walked by c number at most 2 for d <= 3; 0, 1 and 2 are compiled in (NCT), 3 is the loop.
//
// Two kernels, by the status of the last (contiguous) direction:
//   k_reduce_rows   last direction contracted.  A row of n = n_{d-1} values is walked in pairs by LPR lanes as in modal.hip
//                   (16-byte loads where the row starts on a 16-byte boundary), its dot product with the last direction's weights
//                   (in LDS) is scaled by the product of the other contracted weights.  A TEAM of TL = LPR RT lanes owns one
//                   (output, slice): RT = 1 where direction d-2 is kept (neighbouring rows are neighbouring outputs: the teams of
//                   a wave read one contiguous stretch), RT = 64 / LPR where it is contracted (neighbouring rows belong to the same
//                   output: the wave is the team).  A lane adds its rows' products in registers, RB rows in flight before the first
//                   add; the team's lanes meet once, by shuffles, at the end.  At most MAX_WGS workgroups per launch stride over
//                   the teams: one that took a single row each would spend its time fetching the weights.
//   k_reduce_cols   last direction kept.  The trailing kept directions are one contiguous run of Lk values; a lane owns one pair
//                   (j, j + 1) of one run of the output and adds W_c u over the contracted indices c of its slice, RB loads in
//                   flight; the lanes of a wave read and store neighbouring pairs.
// An output whose terms are many, or a contraction with too few outputs to fill the device, is cut into `slices` equal ranges of
// c: slice s stores its partial sums at partial[s][output] and k_reduce_fold adds the slices in a fixed order.  With one slice
// the kernels store into `out` directly.
// No atomics; slices and the launch geometry depend on (dims, nfields, mask) alone; an output reads only the values it owns.
#include "../../include/chebhip.h"
#include "sweep.h"
#include "ops.h"
#include "rowpass.h"
#include <algorithm>
#include <new>
#include <vector>

using namespace chebhip;

static_assert(CHEB_W_INTEGRAL == REDUCE_W_INTEGRAL && CHEB_W_MEAN == REDUCE_W_MEAN && CHEB_W_NODE == REDUCE_W_NODE &&
              CHEB_W_DNODE == REDUCE_W_DNODE && CHEB_W_POINT == REDUCE_W_POINT && CHEB_W_DPOINT == REDUCE_W_DPOINT, "weight kinds");

namespace {

constexpr int MD = 10;                          // directions
constexpr unsigned TARGET_LANES = 1u << 18;     // lanes a launch should have before an output's terms stop being sliced
constexpr unsigned MAX_SLICES = 4096;
constexpr unsigned MAX_WGS = 4096;             // k_reduce_rows: workgroups of a launch, all fields together
constexpr unsigned MIN_ROWS = 4, MIN_TERMS = 8; // a slice has at least this many rows per lane group (rows) / terms (cols)

struct ReduceGeo {
  int nkg, ncd;                      // kept groups decoded from the output index (cols: without the trailing run); directions walked by c
  unsigned kn[MD], ks[MD];           // kept group: extent, stride
  unsigned cn[MD], cs[MD], cw[MD];   // contracted direction: extent, stride, offset of its weights
  unsigned n, wl;                    // rows: extent and weight offset of the last direction; cols: n = Lk
  int lg, lt;                        // rows: log2 LPR, log2 TL
  unsigned P, nunits;                // cols: pairs of a run; (run, pair) units of a field.  rows: nunits = outputs of a field
  unsigned nout, Tc, chunk, slices;  // outputs of a field; values of c; c per slice; slices
  unsigned nteams;                   // nunits * slices
  unsigned N, NT;                    // values of a field; nfields * nout
};

// offset of the kept indices of output (or run) r
__device__ __forceinline__ unsigned kept_offset(const ReduceGeo &g, unsigned r) {
  unsigned off = 0;
  for (int m = g.nkg - 1; m > 0; m--) { const unsigned i = r % g.kn[m]; r /= g.kn[m]; off += i * g.ks[m]; }
  if (g.nkg > 0) off += r * g.ks[0];
  return off;
}

// contracted index c < Tc: its offset is added to off, p = the product of its weights (NCT: directions, 3 = any number)
template <int NCT>
__device__ __forceinline__ void contracted(const ReduceGeo &g, const double *__restrict__ w, unsigned c, unsigned &off, double &p) {
  p = 1.0;
  if (NCT == 0) return;
  if (NCT == 1) { off += c * g.cs[0]; p = w[g.cw[0] + c]; return; }
  if (NCT == 2) {
    const unsigned i0 = c / g.cn[1], i1 = c - i0 * g.cn[1];
    off += i0 * g.cs[0] + i1 * g.cs[1];
    p = w[g.cw[0] + i0] * w[g.cw[1] + i1];
    return;
  }
  for (int m = g.ncd - 1; m > 0; m--) { const unsigned i = c % g.cn[m]; c /= g.cn[m]; off += i * g.cs[m]; p *= w[g.cw[m] + i]; }
  off += c * g.cs[0];
  p *= w[g.cw[0] + c];
}

// NIT: pairs of a row per lane (1, 2, 4, 8 for rows of up to 128, 256, 512, 1024 points); V: the product u v
template <int NIT, int NCT, bool V>
__global__ __launch_bounds__(256) void k_reduce_rows(const ReduceGeo g, const double *__restrict__ w, const double *__restrict__ u,
                                                     const double *__restrict__ v, double *__restrict__ dst) {
  __shared__ double swl[1024];
  constexpr int RB = NIT <= 2 ? 4 : NIT == 4 ? 2 : 1;
  const unsigned n = g.n, tid = threadIdx.x;
  for (unsigned j = tid; j < n; j += 256) swl[j] = w[g.wl + j];
  __syncthreads();
  const unsigned lpr = 1u << g.lg, tl = 1u << g.lt, rt = tl >> g.lg, per_wg = 256u >> g.lt;
  const unsigned l = tid & (lpr - 1), q = (tid & (tl - 1)) >> g.lg;
  for (unsigned t0 = blockIdx.x * per_wg; t0 < g.nteams; t0 += gridDim.x * per_wg) {      // (the same trips for the whole workgroup)
    const unsigned team = t0 + (tid >> g.lt);
    const bool live = team < g.nteams;
    const unsigned s = live ? team / g.nout : 0u, o = live ? team - s * g.nout : 0u;
    const unsigned base = blockIdx.y * g.N + kept_offset(g, o);
    const unsigned c0 = s * g.chunk, c1 = live ? min(g.Tc, c0 + g.chunk) : 0u;
    double acc = 0.0;
    for (unsigned cb = c0 + q; cb < c1; cb += rt * RB) {
      d2 x[RB][NIT], y[RB][NIT];
      double wr[RB];
#pragma unroll
      for (int b = 0; b < RB; b++) {
        const bool ok = cb + b * rt < c1;
        unsigned off = base;
        contracted<NCT>(g, w, ok ? cb + b * rt : c0, off, wr[b]);
        const double *pu = u + off, *pv = V ? v + off : nullptr;
        const bool au = ((size_t)pu & 15) == 0, av = ((size_t)pv & 15) == 0;
#pragma unroll
        for (int it = 0; it < NIT; it++) {
          const unsigned j = 2 * l + 2 * lpr * it;
          x[b][it] = (d2){0.0, 0.0};
          if (V) y[b][it] = (d2){0.0, 0.0};
          if (ok && j < n) {
            x[b][it] = load_pair(pu, au, j, n);
            if (V) y[b][it] = load_pair(pv, av, j, n);
          }
        }
      }
#pragma unroll
      for (int b = 0; b < RB; b++) {
        double sr = 0.0;
#pragma unroll
        for (int it = 0; it < NIT; it++) {
          const unsigned j = 2 * l + 2 * lpr * it;
          d2 a = x[b][it];
          if (V) { a.x *= y[b][it].x; a.y *= y[b][it].y; }
          if (j < n) sr += swl[j] * a.x + (j + 1 < n ? swl[j + 1] : 0.0) * a.y;
        }
        if (cb + b * rt < c1) acc += wr[b] * sr;
      }
    }
    for (unsigned m = 1; m < tl; m <<= 1) acc += __shfl_xor(acc, (int)m);
    if (live && (tid & (tl - 1)) == 0) dst[(size_t)s * g.NT + blockIdx.y * g.nout + o] = acc;
  }
}

template <int NCT, bool V>
__global__ __launch_bounds__(256) void k_reduce_cols(const ReduceGeo g, const double *__restrict__ w, const double *__restrict__ u,
                                                     const double *__restrict__ v, double *__restrict__ dst) {
  constexpr int RB = 4;
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;
  if (gid >= g.nteams) return;
  const unsigned s = gid / g.nunits, t = gid - s * g.nunits;
  const unsigned run = t / g.P, j = 2 * (t - run * g.P), left = g.n - j;      // left >= 1 values of the run from j on
  const unsigned base = blockIdx.y * g.N + kept_offset(g, run) + j;
  const unsigned c0 = s * g.chunk, c1 = min(g.Tc, c0 + g.chunk);
  d2 acc = (d2){0.0, 0.0};
  for (unsigned cb = c0; cb < c1; cb += RB) {
    d2 x[RB], y[RB];
    double wc[RB];
#pragma unroll
    for (int b = 0; b < RB; b++) {
      const bool ok = cb + b < c1;
      unsigned off = base;
      contracted<NCT>(g, w, ok ? cb + b : c0, off, wc[b]);
      const double *pu = u + off, *pv = V ? v + off : nullptr;
      x[b] = (d2){0.0, 0.0};
      if (V) y[b] = (d2){0.0, 0.0};
      if (ok) {
        x[b] = load_pair(pu, ((size_t)pu & 15) == 0, 0, left);
        if (V) y[b] = load_pair(pv, ((size_t)pv & 15) == 0, 0, left);
      }
    }
#pragma unroll
    for (int b = 0; b < RB; b++) {
      d2 a = x[b];
      if (V) { a.x *= y[b].x; a.y *= y[b].y; }
      if (cb + b < c1) { acc.x += wc[b] * a.x; acc.y += wc[b] * a.y; }
    }
  }
  double *po = dst + (size_t)s * g.NT + blockIdx.y * g.nout + run * g.n + j;
  po[0] = acc.x;
  if (left > 1) po[1] = acc.y;
}

// out[t] = sum over the slices of partial[slice][t], t < NT: thread (part, t) adds the slices part, part + 64, ... in ascending
// order, then the 64 parts are added in ascending order.  (The scheme of k_modal_fold; each file keeps its
// own kernel so that its code object stays what it was: with one shared kernel .text starts 256 bytes later and the rows route
// ran 0.6 .. 1.5 % slower with identical kernels, profiles/fieldpass/ab.txt.)
__global__ __launch_bounds__(256) void k_reduce_fold(const double *__restrict__ partial, unsigned slices, unsigned NT, double *__restrict__ out) {
  __shared__ double sp[FOLD_PARTS][FOLD_OUT];
  const unsigned bl = threadIdx.x % FOLD_OUT, part = threadIdx.x / FOLD_OUT, t = blockIdx.x * FOLD_OUT + bl;
  double s = 0.0;
  if (t < NT) {
#pragma unroll 8
    for (unsigned x = part; x < slices; x += FOLD_PARTS) s += partial[(size_t)x * NT + t];
  }
  sp[part][bl] = s;
  __syncthreads();
  if (part == 0 && t < NT) {
    s = sp[0][bl];
    for (int q = 1; q < FOLD_PARTS; q++) s += sp[q][bl];
    out[t] = s;
  }
}

template <int NIT, int NCT>
void launch_rows(const ReduceGeo &g, dim3 grid, hipStream_t st, const double *w, const double *u, const double *v, double *dst) {
  if (v) hipLaunchKernelGGL((k_reduce_rows<NIT, NCT, true>), grid, dim3(256), 0, st, g, w, u, v, dst);
  else hipLaunchKernelGGL((k_reduce_rows<NIT, NCT, false>), grid, dim3(256), 0, st, g, w, u, v, dst);
}

template <int NIT>
void launch_rows_nct(const ReduceGeo &g, dim3 grid, hipStream_t st, const double *w, const double *u, const double *v, double *dst) {
  switch (g.ncd) {
    case 0: launch_rows<NIT, 0>(g, grid, st, w, u, v, dst); break;
    case 1: launch_rows<NIT, 1>(g, grid, st, w, u, v, dst); break;
    case 2: launch_rows<NIT, 2>(g, grid, st, w, u, v, dst); break;
    default: launch_rows<NIT, 3>(g, grid, st, w, u, v, dst);
  }
}

template <int NCT>
void launch_cols(const ReduceGeo &g, dim3 grid, hipStream_t st, const double *w, const double *u, const double *v, double *dst) {
  if (v) hipLaunchKernelGGL((k_reduce_cols<NCT, true>), grid, dim3(256), 0, st, g, w, u, v, dst);
  else hipLaunchKernelGGL((k_reduce_cols<NCT, false>), grid, dim3(256), 0, st, g, w, u, v, dst);
}

}  // namespace

struct cheb_reduce {
  int d = 0, nf = 1;
  int n[MD] = {0}, off[MD] = {0}, contract[MD] = {0};
  long total = 0;                    // nf * prod(dims)
  bool rows = false;                 // the last direction is contracted
  ReduceGeo geo{};
  dim3 grid;
  double *w = nullptr;               // device: the directions' weights, concatenated (off); zeros for a kept direction
  double *partial = nullptr;         // slices x NT partial sums (slices > 1)
};

extern "C" int cheb_reduce_weights_host(int n, int kind, double arg, double *w) {
  int rc;
  if ((rc = check_extent(n))) return rc;
  if (!w) return chebhip_fail(CHEBHIP_ERR_ARG, "w is NULL");
  rc = reduce_weights_host(n, kind, arg, w);
  if (rc == 1) return chebhip_fail(CHEBHIP_ERR_ARG, "kind = %d is none of CHEB_W_*", kind);
  if (rc == 2) return chebhip_fail(CHEBHIP_ERR_ARG, "node %g is no index 0..%d", arg, n - 1);
  return 0;
}

extern "C" int cheb_reduce_destroy(cheb_reduce *h) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (h->w) (void)hipFree(h->w);
  if (h->partial) (void)hipFree(h->partial);
  delete h;
  return 0;
}

extern "C" int cheb_reduce_create(int d, const int *dims, int nfields, const int *contract, cheb_reduce **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  int rc, nc = 0;
  long N = 0, S = 0;
  if ((rc = check_field_count(d, dims, nfields))) return rc;
  if (!contract) return chebhip_fail(CHEBHIP_ERR_ARG, "contract is NULL");
  if ((rc = check_field_extents(d, dims, nullptr, nfields, &N, &S))) return rc;
  for (int k = 0; k < d; k++) nc += contract[k] != 0;
  if (nc == 0) return chebhip_fail(CHEBHIP_ERR_ARG, "no direction is contracted");
  if ((rc = require_device())) return rc;
  cheb_reduce *h = new (std::nothrow) cheb_reduce;
  if (!h) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  h->d = d; h->nf = nfields; h->total = nfields * N;
  h->rows = contract[d - 1] != 0;
  ReduceGeo &g = h->geo;
  g.N = (unsigned)N;
  unsigned stride[MD];
  stride[d - 1] = 1;
  for (int k = d - 2; k >= 0; k--) stride[k] = stride[k + 1] * (unsigned)dims[k + 1];
  table_offsets(d, dims, h->off);
  std::vector<double> w = weight_table(d, dims, h->off, S);
  for (int k = 0; k < d; k++) {
    h->n[k] = dims[k]; h->contract[k] = contract[k] != 0;
    if (!contract[k]) std::fill_n(w.begin() + h->off[k], dims[k], 0.0);      // a kept direction takes no weights
  }

  // the directions c walks (rows: all contracted ones but the last), and the kept groups (cols: all but the trailing run)
  int last_kept = d;                                   // cols: first direction of the trailing kept run
  if (!h->rows) while (last_kept > 0 && !contract[last_kept - 1]) last_kept--;
  g.nkg = g.ncd = 0;
  g.Tc = 1; g.nout = 1;
  unsigned nko = 1;
  for (int k = 0; k < d; k++) {
    if (contract[k]) {
      if (h->rows && k == d - 1) continue;
      g.cn[g.ncd] = (unsigned)dims[k]; g.cs[g.ncd] = stride[k]; g.cw[g.ncd] = (unsigned)h->off[k]; g.ncd++;
      g.Tc *= (unsigned)dims[k];
    } else {
      g.nout *= (unsigned)dims[k];
      if (k >= last_kept) continue;
      nko *= (unsigned)dims[k];
      if (k > 0 && !contract[k - 1]) { g.kn[g.nkg - 1] *= (unsigned)dims[k]; g.ks[g.nkg - 1] = stride[k]; }
      else { g.kn[g.nkg] = (unsigned)dims[k]; g.ks[g.nkg] = stride[k]; g.nkg++; }
    }
  }
  g.NT = (unsigned)nfields * g.nout;

  // launch geometry, fixed per handle: a function of the shape alone
  unsigned lanes_per_unit, min_terms;
  if (h->rows) {
    const int n = dims[d - 1];
    g.n = (unsigned)n; g.wl = (unsigned)h->off[d - 1];
    g.lg = row_lanes_lg(n);
    g.lt = (d >= 2 && contract[d - 2]) ? 6 : g.lg;
    g.P = 0; g.nunits = g.nout;
    lanes_per_unit = 1u << g.lt;
    min_terms = (1u << (g.lt - g.lg)) * MIN_ROWS;
  } else {
    g.n = g.nout / nko;                                // Lk
    g.wl = 0; g.lg = g.lt = 0;
    g.P = (g.n + 1) / 2; g.nunits = nko * g.P;
    lanes_per_unit = 1;
    min_terms = MIN_TERMS;
  }
  const unsigned long lanes = (unsigned long)nfields * g.nunits * lanes_per_unit;
  const unsigned want = (unsigned)((TARGET_LANES + lanes - 1) / lanes), cap = std::max(1u, g.Tc / min_terms);
  g.slices = std::max(1u, std::min(std::min(want, cap), MAX_SLICES));
  g.chunk = (g.Tc + g.slices - 1) / g.slices;
  g.slices = (g.Tc + g.chunk - 1) / g.chunk;
  g.nteams = g.nunits * g.slices;
  const unsigned per_wg = h->rows ? 256u >> g.lt : 256u;
  unsigned gx = (g.nteams + per_wg - 1) / per_wg;
  if (h->rows) gx = std::min(gx, (MAX_WGS + nfields - 1) / nfields);
  h->grid = dim3(gx, (unsigned)nfields);

  rc = device_array(&h->w, S, w.data(), "reduction weights");
  if (!rc && g.slices > 1) rc = device_array(&h->partial, (size_t)g.slices * g.NT, nullptr, "partial sums of the slices");
  if (rc) { cheb_reduce_destroy(h); return rc; }
  *out = h;
  return 0;
}

extern "C" long cheb_reduce_size(const cheb_reduce *h, int which) {
  if (!h || (which != 0 && which != 1)) return -1;
  return which ? (long)h->geo.NT : h->total;
}

extern "C" int cheb_reduce_slices(const cheb_reduce *h) { return h ? (int)h->geo.slices : -1; }

extern "C" int cheb_reduce_set_weights(cheb_reduce *h, int k, const double *w_host) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (k < 0 || k >= h->d) return chebhip_fail(CHEBHIP_ERR_TDIM, "direction %d out of range 0..%d", k, h->d - 1);
  if (!h->contract[k]) return chebhip_fail(CHEBHIP_ERR_ARG, "direction %d is kept: it takes no weights", k);
  return set_direction_weights(h->w, h->off[k], h->n[k], w_host, "reduction weights");
}

extern "C" int cheb_reduce_apply(cheb_reduce *h, const double *u, const double *v, double *out, void *stream) {
  if (!h || !u || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  const ReduceGeo &g = h->geo;
  if (overlap(out, g.NT, u, h->total) || (v && overlap(out, g.NT, v, h->total)))
    return chebhip_fail(CHEBHIP_ERR_ARG, "reduce: the output must not overlap the inputs");
  hipStream_t st = (hipStream_t)stream;
  double *dst = g.slices > 1 ? h->partial : out;
  if (h->rows) {
    if (g.n <= 128) launch_rows_nct<1>(g, h->grid, st, h->w, u, v, dst);
    else if (g.n <= 256) launch_rows_nct<2>(g, h->grid, st, h->w, u, v, dst);
    else if (g.n <= 512) launch_rows_nct<4>(g, h->grid, st, h->w, u, v, dst);
    else launch_rows_nct<8>(g, h->grid, st, h->w, u, v, dst);
  } else {
    switch (g.ncd) {
      case 1: launch_cols<1>(g, h->grid, st, h->w, u, v, dst); break;
      case 2: launch_cols<2>(g, h->grid, st, h->w, u, v, dst); break;
      default: launch_cols<3>(g, h->grid, st, h->w, u, v, dst);
    }
  }
  int rc;
  if ((rc = check_launch("reduce"))) return rc;
  if (g.slices > 1) {
    hipLaunchKernelGGL(k_reduce_fold, dim3((g.NT + FOLD_OUT - 1) / FOLD_OUT), dim3(256), 0, st, h->partial, g.slices, g.NT, out);
    return check_launch("reduce fold");
  }
  return 0;
}
