// stats.hip -- what a field is asked after every step and what is no weighted sum (cheb_stats_*, include/chebhip.h): extrema with
// their positions, the NaN count and the weighted moments (summary), volume-weighted histograms and conditional sums (histogram),
// the advective stability number (cfl).  `nfields` stacked full-grid fields, field-major, row-major, all nodes: the layout of
// cheb_modal_* and cheb_reduce_*.  The weight of a node is W_i = prod_k w_k[i_k], multiplied in ascending k.
//
//   k_stats_summary / k_stats_cfl   streaming reductions in the scheme of k_reduce_rows: a row of n = n_{d-1} values is walked in
//                   pairs by LPR lanes (16-byte loads where the row starts on a 16-byte boundary), the last direction's weights
//                   (cfl: rates) sit in LDS, the other directions' factors are looked up once per row.  A lane keeps its sums, its
//                   extrema and the index of the first element that attains them in registers; the lanes of a workgroup meet once,
//                   by shuffles and through LDS in ascending wave order; workgroup g of field f stores its results at
//                   partial[f][g], and k_stats_fold_summary / k_stats_fold_cfl combine the workgroups in ascending order (sums)
//                   or by the total order (value, index) (extrema: any order gives the same element).
//   k_stats_hist    a workgroup owns a contiguous range of a field, its four waves take the batches of 64 values of that range in
//                   turn.  Each wave has its own row of accumulators (mass, count) per slot in LDS.  A batch is walked with one
//                   step per distinct slot (a lane read, a compare into a lane mask).  Few lanes in a slot: `rank` of a lane = the
//                   lanes below it that go to the same slot (the count of the mask's bits below it), and round r adds the terms
//                   of the lanes of rank r: no two of them share a slot, so nothing conflicts, and a slot receives its terms in
//                   ascending lane order.  Eight lanes or more in a slot (sorted or smooth data): the group is added to the
//                   slot's accumulator in registers, in the same order, and stored once.  The waves' rows are added in
//                   ascending wave order, k_stats_fold_hist adds the workgroups in a fixed order.
// No atomics of any kind; the order of every addition and the launch geometry depend on (dims, nfields, nbins, mode) alone; a
// field's results read only that field's values.
#include "../../include/chebhip.h"
#include "sweep.h"
#include "ops.h"
#include "rowpass.h"
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

using namespace chebhip;

namespace {

constexpr int MD = 10;                          // directions
constexpr unsigned NONE = 0xffffffffu;          // no element yet
constexpr unsigned ROW_WGS = 2048;              // summary, cfl: workgroups of a launch, all fields together
constexpr unsigned ROW_MIN = 8192;              // ... each of at least this many values
constexpr unsigned HIST_WGS = 2048;             // histogram: workgroups of a launch, all fields together
constexpr unsigned HIST_MIN = 8192;             // ... each of at least this many values
constexpr int SUMMARY_OUT = 9, SUMMARY_PART = 9;
constexpr unsigned SERIAL_MIN = 8;              // k_stats_hist: lanes of a batch in one slot from which they are added in registers

struct StatsGeo {
  int d;
  unsigned n[MD], off[MD];          // extent of a direction, offset of its weights (rates) in the concatenated table
  unsigned T, R, nlast;             // values of a field, rows of a field, extent of the last direction
  int lg;                           // log2 of the lanes per row
  unsigned G;                       // workgroups per field (summary, cfl)
};

// is the element (a, ia) ahead of (b, ib) as a minimum (SGN = +1) or as a maximum (SGN = -1)?  NONE loses against every element.
template <int SGN>
__device__ __forceinline__ bool ahead(double a, unsigned ia, double b, unsigned ib) {
  if (ia == NONE) return false;
  if (ib == NONE) return true;
  return (SGN > 0 ? a < b : a > b) || (a == b && ia < ib);
}

// cfl: NaN is ahead of every number, the first NaN ahead of a later one
__device__ __forceinline__ bool ahead_cfl(double a, unsigned ia, double b, unsigned ib) {
  if (ia == NONE) return false;
  if (ib == NONE) return true;
  const bool na = a != a, nb = b != b;
  if (na != nb) return na;
  if (na) return ia < ib;
  return a > b || (a == b && ia < ib);
}

__device__ __forceinline__ unsigned shfl_u(unsigned v, int m) { return (unsigned)__shfl_xor((int)v, m); }

struct Summary {
  double m[4], mn, mx;
  unsigned imn, imx, nan;
};

__device__ __forceinline__ void summary_take(Summary &a, const Summary &b) {       // a = a (+) b, a's sums first
  for (int p = 0; p < 4; p++) a.m[p] += b.m[p];
  if (ahead<1>(b.mn, b.imn, a.mn, a.imn)) { a.mn = b.mn; a.imn = b.imn; }
  if (ahead<-1>(b.mx, b.imx, a.mx, a.imx)) { a.mx = b.mx; a.imx = b.imx; }
  a.nan += b.nan;
}

// every lane of the wave ends with the wave's result: a + b on both sides of each exchange gives both the same bits
__device__ __forceinline__ void summary_wave(Summary &s) {
  for (int m = 1; m < 64; m <<= 1) {
    Summary o;
    for (int p = 0; p < 4; p++) o.m[p] = __shfl_xor(s.m[p], m);
    o.mn = __shfl_xor(s.mn, m); o.mx = __shfl_xor(s.mx, m);
    o.imn = shfl_u(s.imn, m); o.imx = shfl_u(s.imx, m); o.nan = shfl_u(s.nan, m);
    summary_take(s, o);
  }
}

__device__ __forceinline__ void summary_add(Summary &s, double u, double W, double c, unsigned idx) {
  const double x = u - c, x2 = x * x, x3 = x2 * x, x4 = x3 * x;
  s.m[0] += W * x; s.m[1] += W * x2; s.m[2] += W * x3; s.m[3] += W * x4;
  if (u != u) { s.nan++; return; }
  if (s.imn == NONE || u < s.mn) { s.mn = u; s.imn = idx; }
  if (s.imx == NONE || u > s.mx) { s.mx = u; s.imx = idx; }
}

// row r of a field: the product of the weights of the directions before the last, in ascending direction
__device__ __forceinline__ double row_weight(const StatsGeo &g, const double *__restrict__ w, unsigned r) {
  unsigned idx[MD];
#pragma unroll
  for (int k = MD - 2; k >= 0; k--) {
    idx[k] = 0;
    if (k < g.d - 1) { idx[k] = r % g.n[k]; r /= g.n[k]; }
  }
  double p = 1.0;
  bool first = true;
#pragma unroll
  for (int k = 0; k < MD - 1; k++)
    if (k < g.d - 1) { const double wk = w[g.off[k] + idx[k]]; p = first ? wk : p * wk; first = false; }
  return p;
}

// partial[(f * G + wg) * 9 ..]: M_1..M_4, min, max, their indices, the NaN count (the integers as doubles: they are below 2^31)
__global__ __launch_bounds__(256) void k_stats_summary(const StatsGeo g, const double *__restrict__ w, const double *__restrict__ u,
                                                       const double *__restrict__ center, double *__restrict__ partial) {
  __shared__ double swl[1024];
  __shared__ Summary sw[4];
  const unsigned n = g.nlast, tid = threadIdx.x, f = blockIdx.y;
  for (unsigned j = tid; j < n; j += 256) swl[j] = w[g.off[g.d - 1] + j];
  __syncthreads();
  const double c = center ? center[f] : 0.0;
  const unsigned lpr = 1u << g.lg, per_wg = 256u >> g.lg, l = tid & (lpr - 1);
  const double *uf = u + (size_t)f * g.T;
  Summary s;
  for (int p = 0; p < 4; p++) s.m[p] = 0.0;
  s.mn = INFINITY; s.mx = -INFINITY; s.imn = s.imx = NONE; s.nan = 0;
  for (unsigned r = blockIdx.x * per_wg + (tid >> g.lg); r < g.R; r += gridDim.x * per_wg) {
    const double wr = g.d > 1 ? row_weight(g, w, r) : 1.0;
    const double *row = uf + (size_t)r * n;
    const bool al = ((size_t)row & 15) == 0;
    for (unsigned j = 2 * l; j < n; j += 2 * lpr) {
      const d2 x = load_pair(row, al, j, n);
      summary_add(s, x.x, g.d > 1 ? wr * swl[j] : swl[j], c, r * n + j);
      if (j + 1 < n) summary_add(s, x.y, g.d > 1 ? wr * swl[j + 1] : swl[j + 1], c, r * n + j + 1);
    }
  }
  summary_wave(s);
  if ((tid & 63) == 0) sw[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    s = sw[0];
    for (int q = 1; q < 4; q++) summary_take(s, sw[q]);
    double *po = partial + ((size_t)f * gridDim.x + blockIdx.x) * SUMMARY_PART;
    for (int p = 0; p < 4; p++) po[p] = s.m[p];
    po[4] = s.mn; po[5] = s.mx;
    po[6] = s.imn == NONE ? -1.0 : (double)s.imn; po[7] = s.imx == NONE ? -1.0 : (double)s.imx;
    po[8] = (double)s.nan;
  }
}

// one workgroup per field: thread t takes the workgroups t, t + 256, .. in ascending order, then the threads meet as the lanes of
// k_stats_summary do: by shuffles, and the four waves in ascending order
__global__ __launch_bounds__(256) void k_stats_fold_summary(const double *__restrict__ partial, unsigned G, double *__restrict__ out) {
  __shared__ Summary sw[4];
  const unsigned tid = threadIdx.x, f = blockIdx.x;
  Summary s;
  for (int p = 0; p < 4; p++) s.m[p] = 0.0;
  s.mn = INFINITY; s.mx = -INFINITY; s.imn = s.imx = NONE; s.nan = 0;
  for (unsigned x = tid; x < G; x += 256) {
    const double *pi = partial + ((size_t)f * G + x) * SUMMARY_PART;
    Summary o;
    for (int p = 0; p < 4; p++) o.m[p] = pi[p];
    o.mn = pi[4]; o.mx = pi[5];
    o.imn = pi[6] < 0.0 ? NONE : (unsigned)pi[6]; o.imx = pi[7] < 0.0 ? NONE : (unsigned)pi[7];
    o.nan = (unsigned)pi[8];
    summary_take(s, o);
  }
  summary_wave(s);
  if ((tid & 63) == 0) sw[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    s = sw[0];
    for (int q = 1; q < 4; q++) summary_take(s, sw[q]);
    double *po = out + (size_t)f * SUMMARY_OUT;
    po[0] = s.mn; po[1] = s.mx;
    po[2] = s.imn == NONE ? -1.0 : (double)s.imn; po[3] = s.imx == NONE ? -1.0 : (double)s.imx;
    po[4] = (double)s.nan;
    for (int p = 0; p < 4; p++) po[5 + p] = s.m[p];
  }
}

// vel: d fields; rate: the concatenated r_k.  partial[wg * 2 ..]: the value (NaN where a component is NaN), the index or -1
__global__ __launch_bounds__(256) void k_stats_cfl(const StatsGeo g, const double *__restrict__ rate, const double *__restrict__ vel,
                                                   double *__restrict__ partial) {
#pragma clang fp contract(off)      // every product is rounded, then added in ascending k: a plain double restatement has the same bits
  __shared__ double swl[1024];
  __shared__ double sv[4];
  __shared__ unsigned si[4];
  const unsigned n = g.nlast, tid = threadIdx.x;
  for (unsigned j = tid; j < n; j += 256) swl[j] = rate[g.off[g.d - 1] + j];
  __syncthreads();
  const unsigned lpr = 1u << g.lg, per_wg = 256u >> g.lg, l = tid & (lpr - 1);
  double best = 0.0;
  unsigned ibest = NONE;
  for (unsigned r = blockIdx.x * per_wg + (tid >> g.lg); r < g.R; r += gridDim.x * per_wg) {
    double rk[MD - 1];
    {
      unsigned q = r;
#pragma unroll
      for (int k = MD - 2; k >= 0; k--) {
        rk[k] = 0.0;
        if (k < g.d - 1) { const unsigned i = q % g.n[k]; q /= g.n[k]; rk[k] = rate[g.off[k] + i]; }
      }
    }
    const size_t ro = (size_t)r * n;
    for (unsigned j = 2 * l; j < n; j += 2 * lpr) {
      d2 a = (d2){0.0, 0.0};
#pragma unroll
      for (int k = 0; k < MD - 1; k++)
        if (k < g.d - 1) {
          const double *row = vel + (size_t)k * g.T + ro;
          const d2 x = load_pair(row, ((size_t)row & 15) == 0, j, n);
          if (k == 0) { a.x = fabs(x.x) * rk[0]; a.y = fabs(x.y) * rk[0]; }
          else { a.x += fabs(x.x) * rk[k]; a.y += fabs(x.y) * rk[k]; }
        }
      {
        const double *row = vel + (size_t)(g.d - 1) * g.T + ro;
        const d2 x = load_pair(row, ((size_t)row & 15) == 0, j, n);
        const double w0 = swl[j], w1 = j + 1 < n ? swl[j + 1] : 0.0;
        if (g.d == 1) { a.x = fabs(x.x) * w0; a.y = fabs(x.y) * w1; }
        else { a.x += fabs(x.x) * w0; a.y += fabs(x.y) * w1; }
      }
      const unsigned idx = r * n + j;
      if (ahead_cfl(a.x, idx, best, ibest)) { best = a.x; ibest = idx; }
      if (j + 1 < n && ahead_cfl(a.y, idx + 1, best, ibest)) { best = a.y; ibest = idx + 1; }
    }
  }
  for (int m = 1; m < 64; m <<= 1) {
    const double ov = __shfl_xor(best, m);
    const unsigned oi = shfl_u(ibest, m);
    if (ahead_cfl(ov, oi, best, ibest)) { best = ov; ibest = oi; }
  }
  if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = ibest; }
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < 4; q++) if (ahead_cfl(sv[q], si[q], best, ibest)) { best = sv[q]; ibest = si[q]; }
    partial[2 * blockIdx.x] = best;
    partial[2 * blockIdx.x + 1] = ibest == NONE ? -1.0 : (double)ibest;
  }
}

__global__ __launch_bounds__(256) void k_stats_fold_cfl(const double *__restrict__ partial, unsigned G, double *__restrict__ out) {
  __shared__ double sv[4];
  __shared__ unsigned si[4];
  const unsigned tid = threadIdx.x;
  double best = 0.0;
  unsigned ibest = NONE;
  for (unsigned x = tid; x < G; x += 256) {
    const double v = partial[2 * x], di = partial[2 * x + 1];
    const unsigned i = di < 0.0 ? NONE : (unsigned)di;
    if (ahead_cfl(v, i, best, ibest)) { best = v; ibest = i; }
  }
  for (int m = 1; m < 64; m <<= 1) {
    const double ov = __shfl_xor(best, m);
    const unsigned oi = shfl_u(ibest, m);
    if (ahead_cfl(ov, oi, best, ibest)) { best = ov; ibest = oi; }
  }
  if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = ibest; }
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < 4; q++) if (ahead_cfl(sv[q], si[q], best, ibest)) { best = sv[q]; ibest = si[q]; }
    out[0] = best;
    out[1] = ibest == NONE ? -1.0 : (double)ibest;
  }
}

// the weight of the value with flat index i of a field
__device__ __forceinline__ double node_weight(const StatsGeo &g, const double *__restrict__ w, unsigned i) {
  unsigned idx[MD];
#pragma unroll
  for (int k = MD - 1; k >= 0; k--) {
    idx[k] = 0;
    if (k < g.d) { idx[k] = k > 0 ? i % g.n[k] : i; if (k > 0) i /= g.n[k]; }
  }
  double p = w[g.off[0] + idx[0]];
#pragma unroll
  for (int k = 1; k < MD; k++)
    if (k < g.d) p *= w[g.off[k] + idx[k]];
  return p;
}

// slots: 0 underflow, 1 .. nbins the bins, nbins + 1 overflow, nbins + 2 NaN.  UNIFORM: spec = (lo, hi).
__device__ __forceinline__ unsigned slot_uniform(double u, double lo, double inv, bool good, unsigned nbins) {
  if (u != u) return nbins + 2;
  if (!good) return nbins + 1;
  if (u < lo) return 0;
  const double t = (u - lo) * inv;
  if (!(t < (double)nbins)) return nbins + 1;     // t >= nbins, or a t that is NaN (hi - lo overflowed)
  return 1 + (unsigned)t;                          // 0 <= t < nbins: the conversion truncates = floor
}

// EDGES: e[0 .. nbins] non-decreasing; the bin is the last b with e[b] <= u
__device__ __forceinline__ unsigned slot_edges(double u, const double *e, unsigned nbins) {
  if (u != u) return nbins + 2;
  if (u < e[0]) return 0;
  if (!(u < e[nbins])) return nbins + 1;
  unsigned a = 0, b = nbins;                       // e[a] <= u < e[b]
  while (b - a > 1) { const unsigned m = (a + b) >> 1; if (e[m] <= u) a = m; else b = m; }
  return 1 + a;
}

// pm[(f * G + wg) * slots + s], pc[...]: mass and count of workgroup wg.  chunk: values of a workgroup's range, a multiple of 256.
template <bool EDGES, bool COND>
__global__ __launch_bounds__(256) void k_stats_hist(const StatsGeo g, const double *__restrict__ w, const double *__restrict__ u,
                                                    const double *__restrict__ cond, const double *__restrict__ spec, unsigned nbins,
                                                    unsigned chunk, double *__restrict__ pm, unsigned *__restrict__ pc) {
  extern __shared__ double lds[];
  const unsigned slots = nbins + 3, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.y;
  double *se = lds;                                                 // EDGES: nbins + 1 edges
  double *sm = lds + (EDGES ? nbins + 1 : 0);                       // [4][slots] masses
  unsigned *sc = reinterpret_cast<unsigned *>(sm + 4 * slots);      // [4][slots] counts
  if (EDGES) for (unsigned j = tid; j <= nbins; j += 256) se[j] = spec[(size_t)f * (nbins + 1) + j];
  for (unsigned j = tid; j < 4 * slots; j += 256) { sm[j] = 0.0; sc[j] = 0; }
  __syncthreads();
  double lo = 0.0, inv = 0.0;
  bool good = false;
  if (!EDGES) {
    lo = spec[2 * f];
    const double hi = spec[2 * f + 1];
    good = lo < hi && fabs(lo) < INFINITY && fabs(hi) < INFINITY;
    inv = (double)nbins / (hi - lo);
  }
  double *wm = sm + wave * slots;
  unsigned *wc = sc + wave * slots;
  const double *uf = u + (size_t)f * g.T, *cf = COND ? cond + (size_t)f * g.T : nullptr;
  const unsigned i0 = blockIdx.x * chunk, i1 = min(g.T, i0 + chunk);      // (chunk * gridDim.x < 2^32: T < 2^31, chunk <= T + 255)
  for (unsigned ib = i0 + 64 * wave; ib < i1; ib += 256) {
    const unsigned i = ib + lane;
    const bool live = i < i1;
    unsigned s = NONE;
    double term = 0.0;
    if (live) {
      const double x = uf[i];
      s = EDGES ? slot_edges(x, se, nbins) : slot_uniform(x, lo, inv, good, nbins);
      term = node_weight(g, w, i);
      if (COND) term *= cf[i];
    }
    // One step per DISTINCT slot of the batch: the lanes that share the slot of the first lane not yet ranked form a group (a
    // lane mask), and each of them gets its `rank` = the lanes of the group below it.  Round r adds the terms of the lanes of
    // rank r.  A group of SERIAL_MIN lanes or more (sorted or smooth data; rare in noise) is taken out of the rounds and added
    // at once, in registers: every lane reads the slot's accumulator and adds the group's terms in ascending lane order (lane
    // reads: the chain is the same in every lane), the group's first lane stores the result.  Either way a slot receives
    // (((acc + t_a) + t_b) + ..), a < b < ..
    // The accesses are volatile (one load and one store each, never merged over the rounds), and a wave-scope release /
    // acquire pair stands after every store that another lane reads later.
    volatile double *vm = wm;
    volatile unsigned *vc = wc;
    unsigned rank = 0, rounds = 0;
    for (unsigned long long todo = __ballot(live); todo != 0;) {
      const unsigned sq = (unsigned)__builtin_amdgcn_readlane((int)s, __builtin_ctzll(todo));
      const unsigned long long grp = __ballot(live && s == sq);
      const unsigned cnt = (unsigned)__builtin_popcountll(grp);
      if (s == sq) rank = __builtin_amdgcn_mbcnt_hi((unsigned)(grp >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)grp, 0u));
      rounds = max(rounds, cnt < SERIAL_MIN ? cnt : 0u);
      todo &= ~grp;
    }
    // a group of SERIAL_MIN lanes or more has exactly one lane of rank SERIAL_MIN - 1: one step per such group
    for (unsigned long long heads = __ballot(live && rank == SERIAL_MIN - 1); heads != 0; heads &= heads - 1) {
      const unsigned sq = (unsigned)__builtin_amdgcn_readlane((int)s, __builtin_ctzll(heads));
      const unsigned long long grp = __ballot(live && s == sq);
      double acc = vm[sq];
      for (unsigned long long g2 = grp; g2 != 0; g2 &= g2 - 1) {
        const int l = __builtin_ctzll(g2);
        acc += __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(term), l), __builtin_amdgcn_readlane(__double2loint(term), l));
      }
      if (live && s == sq) {
        if (rank == 0) { vm[sq] = acc; vc[sq] = vc[sq] + (unsigned)__builtin_popcountll(grp); }
        rank = NONE;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    for (unsigned r = 0; r < rounds; r++) {
      if (live && rank == r) { vm[s] = vm[s] + term; vc[s] = vc[s] + 1; }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  __syncthreads();
  const size_t po = ((size_t)f * gridDim.x + blockIdx.x) * slots;
  for (unsigned j = tid; j < slots; j += 256) {
    pm[po + j] = ((sm[j] + sm[slots + j]) + sm[2 * slots + j]) + sm[3 * slots + j];
    pc[po + j] = sc[j] + sc[slots + j] + sc[2 * slots + j] + sc[3 * slots + j];
  }
}

// out[f][0][s] = the sum over the workgroups of their masses, out[f][1][s] of their counts: thread (part, t) adds the workgroups
// part, part + 64, .. in ascending order, then the parts are added in ascending order: the tiling of k_modal_fold and k_reduce_fold, but not
// their sum: a part starts from its first term, not from 0.0, and a part without a term is left out, so that a sum of -0.0 terms
// keeps its sign, and the integer counts ride along.  Those are other bits, on purpose.
__global__ __launch_bounds__(256) void k_stats_fold_hist(const double *__restrict__ pm, const unsigned *__restrict__ pc, unsigned G,
                                                         unsigned slots, unsigned nf, double *__restrict__ out) {
  __shared__ double spm[FOLD_PARTS][FOLD_OUT];
  __shared__ unsigned long spc[FOLD_PARTS][FOLD_OUT];
  const unsigned bl = threadIdx.x % FOLD_OUT, part = threadIdx.x / FOLD_OUT, t = blockIdx.x * FOLD_OUT + bl, NT = nf * slots;
  const unsigned f = t < NT ? t / slots : 0u, s = t - f * slots;
  double m = 0.0;
  unsigned long c = 0;
  if (t < NT) {
    const size_t base = (size_t)f * G * slots + s;
    if (part < G) m = pm[base + (size_t)part * slots];          // (stored, not added to 0.0: a sum of -0.0 terms keeps its sign)
    if (part < G) c = pc[base + (size_t)part * slots];
    for (unsigned x = part + FOLD_PARTS; x < G; x += FOLD_PARTS) { m += pm[base + (size_t)x * slots]; c += pc[base + (size_t)x * slots]; }
  }
  spm[part][bl] = m; spc[part][bl] = c;
  __syncthreads();
  if (part == 0 && t < NT) {
    const unsigned live = G < (unsigned)FOLD_PARTS ? G : (unsigned)FOLD_PARTS;
    for (unsigned q = 1; q < live; q++) { m += spm[q][bl]; c += spc[q][bl]; }
    out[(size_t)f * 2 * slots + s] = m;
    out[(size_t)f * 2 * slots + slots + s] = (double)c;
  }
}

}  // namespace

struct cheb_stats {
  int d = 0, nf = 1, max_bins = 1;
  long total = 0;                    // nf * prod(dims)
  StatsGeo geo{};
  unsigned Gh = 1, chunk = 0;        // histogram: workgroups per field, values of a workgroup
  int S = 0;                         // sum of dims
  double *w = nullptr;               // device: the directions' weights, concatenated
  double *rate = nullptr;            // device: the directions' r_k of the last scale, concatenated
  double *partial = nullptr;         // summary: nf * G * 9; cfl: G * 2
  double *pm = nullptr;              // histogram: nf * Gh * (max_bins + 3) masses
  unsigned *pc = nullptr;            // ... and counts
  std::vector<double> scale;         // the scale `rate` was built for (empty: none yet)
  std::vector<double> rate_host;
};

extern "C" int cheb_stats_spacing_host(int n, double *h) {
  int rc;
  if ((rc = check_extent(n))) return rc;
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "h is NULL");
  stats_spacing_host(n, h);
  return 0;
}

extern "C" int cheb_stats_rate_host(int n, double s, double *r) {
  int rc;
  if ((rc = check_extent(n))) return rc;
  if (!r) return chebhip_fail(CHEBHIP_ERR_ARG, "r is NULL");
  if (!(s == s)) return chebhip_fail(CHEBHIP_ERR_ARG, "the scale is NaN");
  stats_rate_host(n, s, r);
  return 0;
}

extern "C" int cheb_stats_check(int d, const int *dims, int nfields, int max_bins, int nbins) {
  int rc;
  // (this module answers a bad d with CHEBHIP_ERR_ARG where every other module says CHEBHIP_ERR_DIMS: kept)
  if ((rc = check_field_count(d, dims, nfields, CHEBHIP_ERR_ARG))) return rc;
  if (max_bins < 1 || max_bins > 1024) return chebhip_fail(CHEBHIP_ERR_ARG, "max_bins = %d must be in 1..1024", max_bins);
  if (nbins < 1 || nbins > max_bins) return chebhip_fail(CHEBHIP_ERR_ARG, "nbins = %d must be in 1..max_bins = %d", nbins, max_bins);
  return check_field_extents(d, dims, nullptr, nfields, nullptr, nullptr);
}

extern "C" int cheb_stats_destroy(cheb_stats *h) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (h->w) (void)hipFree(h->w);
  if (h->rate) (void)hipFree(h->rate);
  if (h->partial) (void)hipFree(h->partial);
  if (h->pm) (void)hipFree(h->pm);
  if (h->pc) (void)hipFree(h->pc);
  delete h;
  return 0;
}

extern "C" int cheb_stats_create(int d, const int *dims, int nfields, int max_bins, cheb_stats **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  int rc;
  if ((rc = cheb_stats_check(d, dims, nfields, max_bins, max_bins))) return rc;
  if ((rc = require_device())) return rc;
  cheb_stats *h = new (std::nothrow) cheb_stats;
  if (!h) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  h->d = d; h->nf = nfields; h->max_bins = max_bins;
  StatsGeo &g = h->geo;
  g.d = d;
  long T = 1;
  int S = 0;
  for (int k = 0; k < d; k++) { g.n[k] = (unsigned)dims[k]; S += dims[k]; T *= dims[k]; }
  table_offsets(d, dims, g.off);
  h->S = S; h->total = T * nfields;
  g.T = (unsigned)T; g.nlast = (unsigned)dims[d - 1]; g.R = g.T / g.nlast;
  g.lg = row_lanes_lg(dims[d - 1]);
  // launch geometry, fixed per handle: a function of the shape alone
  const unsigned per_wg = 256u >> g.lg, passes = (g.R + per_wg - 1) / per_wg;
  g.G = std::max(1u, std::min(std::min((g.T + ROW_MIN - 1) / ROW_MIN, passes), ROW_WGS / (unsigned)nfields));
  h->Gh = std::max(1u, std::min((g.T + HIST_MIN - 1) / HIST_MIN, HIST_WGS / (unsigned)nfields));
  h->chunk = ((g.T + h->Gh - 1) / h->Gh + 255u) / 256u * 256u;
  h->Gh = (g.T + h->chunk - 1) / h->chunk;

  const std::vector<double> w = weight_table(d, dims, g.off, S);
  const size_t slots = (size_t)max_bins + 3;
  rc = device_array(&h->w, S, w.data(), "stats weights");
  if (!rc) rc = device_array(&h->rate, S, nullptr, "stats rates");
  if (!rc) rc = device_array(&h->partial, (size_t)nfields * g.G * SUMMARY_PART, nullptr, "stats partial results");
  if (!rc) rc = device_array(&h->pm, (size_t)nfields * h->Gh * slots, nullptr, "histogram partial masses");
  if (!rc) {
    hipError_t e = hipMalloc(&h->pc, (size_t)nfields * h->Gh * slots * sizeof(unsigned));
    if (e != hipSuccess) { h->pc = nullptr; rc = chebhip_fail(CHEBHIP_ERR_MEMORY, "histogram partial counts: %s", hipGetErrorString(e)); }
  }
  if (rc) { cheb_stats_destroy(h); return rc; }
  *out = h;
  return 0;
}

extern "C" long cheb_stats_size(const cheb_stats *h, int which) {
  if (!h) return -1;
  switch (which) {
    case 0: return h->total;                                  // input values
    case 1: return (long)h->nf * SUMMARY_OUT;                 // values of a summary
    case 2: return h->max_bins;
    case 3: return (long)h->geo.G;                            // workgroups per field of summary and cfl
    case 4: return (long)h->Gh;                               // ... of histogram
    default: return -1;
  }
}

extern "C" int cheb_stats_set_weights(cheb_stats *h, int k, const double *w_host) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (k < 0 || k >= h->d) return chebhip_fail(CHEBHIP_ERR_TDIM, "direction %d out of range 0..%d", k, h->d - 1);
  return set_direction_weights(h->w, h->geo.off[k], (int)h->geo.n[k], w_host, "stats weights");
}

extern "C" int cheb_stats_summary(cheb_stats *h, const double *u, const double *center, double *out, void *stream) {
  if (!h || !u || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  const StatsGeo &g = h->geo;
  if (overlap(out, (long)h->nf * SUMMARY_OUT, u, h->total)) return chebhip_fail(CHEBHIP_ERR_ARG, "summary: the output must not overlap the input");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  hipLaunchKernelGGL(k_stats_summary, dim3(g.G, (unsigned)h->nf), dim3(256), 0, st, g, h->w, u, center, h->partial);
  if ((rc = check_launch("summary"))) return rc;
  hipLaunchKernelGGL(k_stats_fold_summary, dim3((unsigned)h->nf), dim3(256), 0, st, h->partial, g.G, out);
  return check_launch("summary fold");
}

extern "C" int cheb_stats_histogram(cheb_stats *h, const double *u, const double *cond, int mode, int nbins, const double *spec,
                                    double *out, void *stream) {
  if (!h || !u || !spec || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (nbins < 1 || nbins > h->max_bins) return chebhip_fail(CHEBHIP_ERR_ARG, "nbins = %d must be in 1..max_bins = %d", nbins, h->max_bins);
  if (mode != CHEB_STATS_UNIFORM && mode != CHEB_STATS_EDGES) return chebhip_fail(CHEBHIP_ERR_ARG, "mode = %d is none of CHEB_STATS_*", mode);
  const StatsGeo &g = h->geo;
  const unsigned slots = (unsigned)nbins + 3;
  const long nout = (long)h->nf * 2 * slots;
  if (overlap(out, nout, u, h->total) || (cond && overlap(out, nout, cond, h->total)))
    return chebhip_fail(CHEBHIP_ERR_ARG, "histogram: the output must not overlap the inputs");
  hipStream_t st = (hipStream_t)stream;
  const bool edges = mode == CHEB_STATS_EDGES;
  const size_t lds = ((edges ? (size_t)nbins + 1 : 0) + 4 * (size_t)slots) * sizeof(double) + 4 * (size_t)slots * sizeof(unsigned);
  const dim3 grid(h->Gh, (unsigned)h->nf);
  const unsigned nb = (unsigned)nbins;
  if (edges) {
    if (cond) hipLaunchKernelGGL((k_stats_hist<true, true>), grid, dim3(256), lds, st, g, h->w, u, cond, spec, nb, h->chunk, h->pm, h->pc);
    else hipLaunchKernelGGL((k_stats_hist<true, false>), grid, dim3(256), lds, st, g, h->w, u, cond, spec, nb, h->chunk, h->pm, h->pc);
  } else {
    if (cond) hipLaunchKernelGGL((k_stats_hist<false, true>), grid, dim3(256), lds, st, g, h->w, u, cond, spec, nb, h->chunk, h->pm, h->pc);
    else hipLaunchKernelGGL((k_stats_hist<false, false>), grid, dim3(256), lds, st, g, h->w, u, cond, spec, nb, h->chunk, h->pm, h->pc);
  }
  int rc;
  if ((rc = check_launch("histogram"))) return rc;
  hipLaunchKernelGGL(k_stats_fold_hist, dim3(((unsigned)h->nf * slots + FOLD_OUT - 1) / FOLD_OUT), dim3(256), 0, st, h->pm, h->pc, h->Gh, slots,
                     (unsigned)h->nf, out);
  return check_launch("histogram fold");
}

extern "C" int cheb_stats_cfl(cheb_stats *h, const double *vel, const double *scale_host, double *out, void *stream) {
  if (!h || !vel || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  const StatsGeo &g = h->geo;
  std::vector<double> s(h->d, 1.0);
  if (scale_host)
    for (int k = 0; k < h->d; k++) {
      if (!(std::fabs(scale_host[k]) < INFINITY)) return chebhip_fail(CHEBHIP_ERR_ARG, "cfl: scale[%d] is not finite", k);
      s[k] = scale_host[k];
    }
  hipStream_t st = (hipStream_t)stream;
  if (s != h->scale) {                                   // a new scale: r is formed again and goes ahead of the kernel on `stream`
    h->rate_host.resize(h->S);
    for (int k = 0; k < h->d; k++) stats_rate_host((int)g.n[k], s[k], h->rate_host.data() + g.off[k]);
    h->scale.clear();
    HIP_TRY(hipMemcpyAsync(h->rate, h->rate_host.data(), (size_t)h->S * sizeof(double), hipMemcpyHostToDevice, st));
    h->scale = s;
  }
  int rc;
  hipLaunchKernelGGL(k_stats_cfl, dim3(g.G), dim3(256), 0, st, g, h->rate, vel, h->partial);
  if ((rc = check_launch("cfl"))) return rc;
  hipLaunchKernelGGL(k_stats_fold_cfl, dim3(1), dim3(256), 0, st, h->partial, g.G, out);
  return check_launch("cfl fold");
}
