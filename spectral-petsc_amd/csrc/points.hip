// points.hip -- values of `nfields` stacked full-grid Chebyshev-Gauss-Lobatto fields (field-major, row-major, all nodes: the
// layout of cheb_modal_* and cheb_helmholtz_solve_bc) at arbitrary points of the reference cube (cheb_points_*,
// include/chebhip.h): scattered points whose coordinates live on the device, and tensor grids of arbitrary coordinates (plane
// and line cuts, uniform plotting grids).
//
// Per direction of n points the interpolant is evaluated in barycentric form with the weights w_j = (-1)^j, halved at both ends.
// The row of a coordinate x is built on the device (k_points_rows) in the nearest-node form, which cannot overflow:
//   s = the node nearest to x,  d_j = x - x_j,  r_s = 1,  r_j = (w_j / w_s) (d_s / d_j),  l = r / sum r
// from the node table the handle uploaded at create (long double, rounded once, diffmat.cpp).  d_s == 0 gives the exact unit row,
// a NaN or infinite coordinate a row of NaN, |x| > 1 is extrapolated by the same formula.  A row is built by G lanes (the power
// of two >= n, at most 64), lane l taking j = l, l + G, ...; the lanes' sums meet by a butterfly of shuffles, so the order of the
// sum depends on n alone and rows repeat bit for bit.
//
// Scattered points run in chunks of C points (cheb_points_chunk), three launches a chunk:
//   1. k_points_rows: the C x n_k rows of every direction;
//   2. direction 0 on the FP64 matrix cores: the line product of linegemm.hip with R = the chunk's C x n_0 rows, O = nfields,
//      Q = n_1 .. n_{d-1} -- the fields are read once per chunk; the result is [field][point][i_1 .. i_{d-1}];
//   3. k_points_contract: one workgroup per (field, point) contracts the point's contiguous block with the product of the other
//      directions' rows: the last direction's row in LDS, 16-byte loads where a block row starts on a 16-byte boundary, no
//      atomics, a fixed order of additions.
// Tensor grids take the same rows and one line product per direction (line_chain), shrinking directions first, as resample.hip does.
//
// cheb_points_spread is the transpose of the scattered evaluation: one number per (field, point) goes onto the grid,
//   g[f][i_0 .. i_{d-1}] = sum_p s[f][p] l_0,p[i_0] l_1,p[i_1] .. l_{d-1},p[i_{d-1}]
// in passes of cheb_points_spread_pass points, two launches a pass: k_points_rows into the handle's work memory, then
// k_points_spread, a product on the FP64 matrix cores with the workgroup tile of linetile.h whose contracted index is the point:
//   matrix operand  R[i_0][p] = rows_0[p][i_0]: the rows of direction 0 as k_points_rows stores them, read along i_0;
//   image operand   X[p][line] = ((s[f][p] l_1,p[i_1]) l_2,p[i_2] ..) l_{d-1},p[i_{d-1}], line = (f, i_1 .. i_{d-1}): formed in
//                   registers by the threads that fill the LDS chunk, in exactly this association; d = 1: X[p][f] = s[f][p].
// A workgroup owns BM points of direction 0 x 64 lines and walks the pass in LDS chunks of RS_KC points; slots past the last point
// are zeros in both operands, written by a select and never read from memory (a stale NaN row times 0 would be NaN).  The epilogue stores, or adds
// to what `out` holds (later passes, CHEB_SPREAD_ACCUMULATE), after multiplying by the inverse Clenshaw-Curtis weights
// (v iw_0[i_0]) (iw_1[i_1] (.. iw_{d-1}[i_{d-1}])) under CHEB_SPREAD_DELTA.  No atomics: every element of `out` belongs to one lane,
// and the order of its additions depends on (dims, nfields, npts, pass size) alone.
//
// First derivatives are another row per direction (k_points_rows writes value rows, derivative rows or both, as its job says: the
// derivative of the same rational function, by a formula that never divides by d_s).  cheb_points_eval_deriv / _spread_deriv /
// _eval_grid_deriv run the pipelines above with the flagged directions' rows exchanged; the plain calls are these with no direction
// flagged.  cheb_points_eval_grad takes every first derivative of a chunk of C / 2 points from ONE direction-0 line product over the
// stacked value and derivative rows, [field][2 cnt][i_1 .. i_{d-1}], and one launch of k_points_contract<DC, true>, the same
// contraction with an accumulator per component, over the blocks it writes.
//
// A periodic direction (cheb_points_create_basis) takes its rows, value and derivative, from k_points_frows: the
// trigonometric interpolant in the same nearest-node form, coordinates wrapped into the period.  Everything downstream takes rows.
// One rows job holds the entries of both bases; launch_rows runs the CGL ones, then the periodic ones.
#include "../../include/chebhip.h"
#include "sweep.h"
#include "ops.h"
#include "rowpass.h"
#include "linetile.h"
#include <algorithm>
#include <cmath>
#include <map>
#include <new>
#include <type_traits>
#include <vector>

using namespace chebhip;

namespace {

constexpr int MD = 10;               // directions
constexpr long WORK_MIN = 32L << 20; // bytes of work memory a handle may always take

// one entry of a rows job: m coordinates x[i stride] of a direction of n points, m rows of n values each
struct RowsEntry {
  int n, lg;                         // extent; log2 of the lanes that share a row
  int what;                          // 1 the value rows into R, 2 the derivative rows into D, 3 both
  int periodic;                      // the rows of k_points_frows (nodes: its table), not of k_points_rows
  unsigned m;
  long stride;
  const double *x, *nodes;
  double *R, *D;
};

// the rows of a chunk, pass or grid: entry blockIdx.y of a launch.  A launch holds entries of one basis (launch_rows)
struct RowsJob {
  int nd;
  RowsEntry e[MD];
};

struct PtGeo {
  int d, lg;                         // directions; log2 of the lanes per block row in k_points_contract
  int n[MD];
  unsigned off[MD];                  // sum of the extents before direction k: its rows start at rows + C off[k]
  unsigned rpb, B;                   // rows of n_{d-1} values per block; values per block, n_1 .. n_{d-1}
};

// A row is built by the G = 2^lg lanes of a group, lane l of it taking the nodes l, l + G, ..: 64 / G rows a wave, four waves.
// ok: the row exists (the lanes of a missing one take x = 0 through the shuffles and store nothing)
struct RowLanes {
  int n, G, l;
  unsigned row;
  bool ok;
  double x;
};

__device__ __forceinline__ RowLanes row_lanes(const RowsEntry &e) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int G = 1 << e.lg, rpw = 64 >> e.lg, grp = lane >> e.lg;
  const unsigned row = (blockIdx.x * 4u + (unsigned)wv) * (unsigned)rpw + (unsigned)grp;
  const bool ok = row < e.m;
  return RowLanes{e.n, G, lane & (G - 1), row, ok, ok ? e.x[(size_t)row * (size_t)e.stride] : 0.0};
}

// the sums over a row's lane group, by a butterfly: every lane gets them, in an order that depends on G alone (sums that are
// ready together go through one call: their shuffles overlap)
template <class... T>
__device__ __forceinline__ void group_sum(int G, T &...v) {
  for (int mm = 1; mm < G; mm <<= 1) ((v += __shfl_xor(v, mm)), ...);
}

// entry j of a value row from its unnormalised entry e: a row of NaN for a coordinate that is not finite, the exact unit row on node s
__device__ __forceinline__ double row_value(bool fin, double ds, bool self, double e, double sum) {
  return !fin ? __builtin_nan("") : ds == 0.0 ? (self ? 1.0 : 0.0) : e / sum;
}

// The rows of a CGL direction, values and derivatives l'_j(x) = d l_j / dx.  With c_j = w_j / w_s, q_j = c_j / d_j (j != s),
// R = 1 + sum r_j (the value rows' normalising sum), Q2 = sum q_k / d_k and T = sum q_k ((x_s - x_k) / d_k), all sums over k != s:
//   l'_j = (q_j / R) ((1 + d_s^2 Q2) / R - d_s / d_j)   (j != s),     l'_s = -T / R^2
// Nothing divides by d_s; d_s == 0 gives R = 1, (x_s - x_k) / d_k = 1 exactly and the row l'_j = q_j, l'_s = -sum q_k of the
// differentiation matrix by the same instructions.  The value rows do not depend on whether the derivative rows are asked for.
__global__ __launch_bounds__(256) void k_points_rows(const RowsJob g) {
  const RowsEntry &e = g.e[blockIdx.y];
  const RowLanes r = row_lanes(e);
  const int n = r.n, N = n - 1, G = r.G, l = r.l, what = e.what;
  const double *__restrict__ xn = e.nodes;
  const double x = r.x;

  // the nearest node, the lowest index on a tie
  double best = INFINITY;
  int s = 0x7fffffff;
  for (int j = l; j < n; j += G) { const double a = fabs(x - xn[j]); if (a < best) { best = a; s = j; } }
  for (int mm = 1; mm < G; mm <<= 1) {
    const double ob = __shfl_xor(best, mm);
    const int os = __shfl_xor(s, mm);
    if (ob < best || (ob == best && os < s)) { best = ob; s = os; }
  }
  const bool fin = fabs(x) < INFINITY;                     // (false for a NaN as well)
  if (!fin) s = 0;
  const double xs = xn[s], ds = x - xs, ihs = (s == 0 || s == N) ? 2.0 : 1.0;
  auto coef = [&](int j) -> double {                       // w_j / w_s
    const double hj = (j == 0 || j == N) ? 0.5 : 1.0;
    return (((j - s) & 1) ? -hj : hj) * ihs;
  };
  auto entry = [&](int j) -> double {
    if (j == s) return 1.0;
    return coef(j) * (ds / (x - xn[j]));
  };
  double sum = 0.0;
  for (int j = l; j < n; j += G) sum += entry(j);
  group_sum(G, sum);
  double q2 = 0.0, t = 0.0;
  if (what & 2) {
    for (int j = l; j < n; j += G)
      if (j != s) {
        const double dj = x - xn[j], q = coef(j) / dj;
        q2 += q / dj;
        t += q * ((xs - xn[j]) / dj);
      }
    group_sum(G, q2, t);
  }
  if (!r.ok) return;
  if (what & 1) {
    double *__restrict__ out = e.R + (size_t)r.row * (size_t)n;
    for (int j = l; j < n; j += G) out[j] = row_value(fin, ds, j == s, entry(j), sum);
  }
  if (what & 2) {
    double *__restrict__ out = e.D + (size_t)r.row * (size_t)n;
    const double g0 = (1.0 + ds * ds * q2) / sum, ls = -t / (sum * sum);
    for (int j = l; j < n; j += G) {
      double v = ls;
      if (j != s) { const double dj = x - xn[j]; v = (coef(j) / dj) / sum * (g0 - ds / dj); }
      out[j] = fin ? v : __builtin_nan("");
    }
  }
}

// The rows of a PERIODIC direction (cheb_points_create_basis): n nodes x_j = -1 + 2 j / n, period 2, the trigonometric
// interpolant in its barycentric form r_j ~ (-1)^j cot(pi (x - x_j) / 2) (n even), (-1)^j / sin(pi (x - x_j) / 2) (n odd), in the
// nearest-node form of k_points_rows: entries relative to node s, one normalising sum over the row's lane group, the same butterflies.
// The arithmetic is this kernel's own; the lane groups, the group sums and the value-row store are k_points_rows' helpers.  An
// entry's `nodes` is the table of fourier_points_table_host.
//   wrapping   any finite x is wrapped, never extrapolated: xr = x - 2 rint(x / 2) in [-1, 1], exact in double;
//   s          by arithmetic, no search: the candidates rint((xr + 1) n / 2) and its two neighbours, the smallest |distance|, the
//              lowest index on a tie; the candidate n is node 0 one period on (it serves x ~ +1);
//   d_s        = xr - x_s with x_s the DOUBLE node of the table (xr - 1 for the candidate n): exact (Sterbenz: |d_s| <= 1 / n <=
//              |x_s| / 2, or x_s = 0).  The rows are those of the point x_s(exact) + d_s, which is x moved by the rounding of the
//              node, at most 2^-54: so the doubles fourier_nodes(n), and their images a period away, give the exact unit row;
//   entries    with a = pi d_s / 2 and b = pi m / n, m = (s - j) mod n, from the table (sinpi / cospi of d_s / 2 for a):
//              S = sin a cos b + cos a sin b = sin(pi (x - x_j) / 2) up to the sign both parities carry in (-1)^m; the two terms are
//              within a factor 3 of their sum (|tan a / tan b| <= 1/2), so nothing is lost half a period away, where a rounded
//              x - x_j would leave the small sine without relative accuracy.  C = cos a cos b - sin a sin b.
//              n odd: e_j = (-1)^m sin a / S;  n even: e_j = (-1)^m tan a (C / S);  e_s = 1;  r = e / sum e.
//              Nothing divides by d_s; d_s == 0 is the exact unit row; NaN or +-Inf a row of NaN.
//   derivative of the same rational function, h = pi / 2, sums over j != s:
//              n odd:  p_j = h (-1)^m cos a / S,          f_j = -h (-1)^m sin a C / S^2
//              n even: p_j = h (-1)^m (C / S) / cos^2 a,  f_j = -h (-1)^m tan a / S^2
//              r'_j = (f_j R + p_j - e_j F) / R^2,  r'_s = -(P + F) / R^2,  R = sum e, F = sum f, P = sum p.
//              d_s == 0: e = f = 0, R = 1 and r'_j = p_j, r'_s = -P: row s of D_F by the same instructions.
__global__ __launch_bounds__(256) void k_points_frows(const RowsJob g) {
  const RowsEntry &en = g.e[blockIdx.y];
  const RowLanes r = row_lanes(en);
  const int n = r.n, G = r.G, l = r.l, what = en.what;
  const double *__restrict__ tab = en.nodes;
  const double x = r.x;
  const bool fin = fabs(x) < INFINITY;                     // (false for a NaN as well)
  const double xf = fin ? x : 0.0;
  const double xr = xf - 2.0 * rint(0.5 * xf);

  int s = 0;
  double ds = 0.0, best = INFINITY;
  const int c0 = (int)rint((xr + 1.0) * (0.5 * (double)n));
  for (int c = c0 - 1; c <= c0 + 1; c++) {
    if (c < 0 || c > n) continue;
    const int j = c == n ? 0 : c;
    const double dd = c == n ? xr - 1.0 : xr - tab[j];
    const double a = fabs(dd);
    if (a < best || (a == best && j < s)) { best = a; s = j; ds = dd; }
  }
  const double sa = sinpi(0.5 * ds), ca = cospi(0.5 * ds), ta = sa / ca, h = 1.5707963267948966;
  const bool odd = n & 1;
  // (e, p, f) of node j != s
  auto parts = [&](int j, double &e, double &p, double &f) {
    int m = s - j;
    if (m < 0) m += n;
    const double sb = tab[n + m], cb = tab[2 * n + m], sg = (m & 1) ? -1.0 : 1.0;
    const double S = sa * cb + ca * sb, C = ca * cb - sa * sb;
    if (odd) { e = sg * (sa / S); p = h * sg * (ca / S); f = -h * sg * (sa * C / (S * S)); }
    else { const double cs = C / S; e = sg * (ta * cs); p = h * sg * (cs / (ca * ca)); f = -h * sg * (ta / (S * S)); }
  };
  double R = 0.0, F = 0.0, P = 0.0;
  for (int j = l; j < n; j += G) {
    if (j == s) { R += 1.0; continue; }
    double e, p, f;
    parts(j, e, p, f);
    R += e;
    if (what & 2) { F += f; P += p; }
  }
  group_sum(G, R);
  if (what & 2) group_sum(G, F, P);
  if (!r.ok) return;
  double *__restrict__ outv = (what & 1) ? en.R + (size_t)r.row * (size_t)n : nullptr;
  double *__restrict__ outd = (what & 2) ? en.D + (size_t)r.row * (size_t)n : nullptr;
  const double R2 = R * R;
  for (int j = l; j < n; j += G) {
    double e = 1.0, p = 0.0, f = 0.0;
    if (j != s) parts(j, e, p, f);
    if (outv) outv[j] = row_value(fin, ds, j == s, e, R);
    if (outd) outd[j] = !fin ? __builtin_nan("") : j == s ? -(P + F) / R2 : (f * R + p - e * F) / R2;
  }
}

// The indices (i_1 .. i_{end-1}) of the flat index q over the directions 1 .. end - 1, the last one fastest: f(k, i_k) from
// k = end - 1 down to 1.  DC: an upper bound of `end` known at compile time (the loop is unrolled, so f may keep per-direction
// state in registers), 0: none.  k_points_spread keeps its two walks written out: through this helper the compiler schedules
// them otherwise, and that kernel's listing is held to the instruction (profiles/points/unify_isa.txt).
template <int DC, class F>
__device__ __forceinline__ void unflatten(unsigned q, const int *n, int end, F f) {
  auto step = [&](int k) {
    const unsigned nk = (unsigned)n[k], i = k > 1 ? q % nk : q;
    q /= nk;
    f(k, i);
  };
  if (DC) {
#pragma unroll
    for (int k = DC - 1; k >= 1; k--)
      if (k < end) step(k);
  } else {
    for (int k = end - 1; k >= 1; k--) step(k);
  }
}

struct ConArgs {
  const double *rows;                // direction k's value rows at rows + P off[k], its derivative rows H n_k values further
  unsigned P, H;
  const double *V, *D;               // direction 0's value and derivative blocks, (f, p) at ((f bs) + p) B; D null: none
  unsigned bs;                       // blocks per field
  double *out;                       // component c of (f, p) at out[(f nc + c) npts + p]
  size_t npts;
  int nc;                            // components per field
  unsigned mask;                     // sums to store: bit k < d the derivative along k (GRAD), bit d the value sum of V
  int vdst;                          // the component the value sum of V goes to
  double scale[MD + 1];              // per component, multiplied at the store
};

// Workgroup (p, f), 1 or 4 waves (blockDim.x), contracts the point's block W[f][p][i_1 .. i_{d-1}] with the rows of directions
// 1 .. d - 1.  The block is rpb rows of n = n_{d-1} values, the last direction's row is in LDS; LPR lanes walk a block row by pairs,
// a wave takes 64 / LPR rows at a time, a row's weight w is the product of the middle directions' entries (DC: d known at compile
// time, 0: any d up to MD).  No atomics, a fixed order of additions.
//   GRAD false  one sum, sum_rows w sum_j l_{d-1}[j] v over V, stored as component vdst (bit d of the mask, D null): the scattered
//               evaluation, out[f][p], and eval_grad's chunk of one point, a component a launch.  No derivative row in LDS, no
//               derivative weights, one accumulator.
//   GRAD true   the gradient of that sum: workgroup (p, f, 0) walks V once, forming per block row s = sum_j l_{d-1}[j] v and
//               s' = sum_j l'_{d-1}[j] v; the value takes w s, the last direction's derivative w s', a middle direction's w_k s with
//               w_k the product w with direction k's derivative entry.  Workgroup (p, f, 1) walks the derivative block D once for
//               direction 0's derivative, w sum_j l_{d-1}[j] v: the value sum of that block (two workgroups a point: at 256^3 a
//               chunk of 64 points is 64 MiB of blocks, which 64 workgroups read at half the rate 128 do).
// The value sum is formed by the same instructions in the same order in both.
template <int DC, bool GRAD>
__global__ __launch_bounds__(256) void k_points_contract(const PtGeo g, const ConArgs a) {
  constexpr int DM = DC ? DC : MD;
  constexpr int NA = GRAD ? DM + 1 : 1;                    // accumulators: the value sum in the last, the derivative along c in acc[c]
  __shared__ double swl[1024], swd[GRAD ? 1024 : 1];
  __shared__ double red[4][NA];
  const int d = DC ? DC : g.d;
  const unsigned n = (unsigned)g.n[d - 1];
  const unsigned p = blockIdx.x, f = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
  const bool second = GRAD && blockIdx.z != 0;
  const unsigned mask = second ? (a.mask & 1u) << d : (GRAD && a.D) ? a.mask & ~1u : a.mask;
  const int vdst = second ? 0 : a.vdst;
  const bool derivs = GRAD && (mask & ((1u << d) - 2u)) != 0;  // any of directions 1 .. d - 1
  const double *rl = a.rows + (size_t)a.P * g.off[d - 1] + (size_t)p * n;
  for (unsigned j = tid; j < n; j += blockDim.x) {
    swl[j] = rl[j];
    if (GRAD) swd[j] = derivs ? rl[(size_t)a.H * n + j] : 0.0;
  }
  __syncthreads();
  const unsigned lpr = 1u << g.lg, rpw = 64u >> g.lg, grp = (unsigned)lane >> g.lg, l = (unsigned)lane & (lpr - 1);
  const double *bv = (second ? a.D : a.V) + ((size_t)f * a.bs + p) * g.B;
  double acc[NA];
#pragma unroll
  for (int c = 0; c < NA; c++) acc[c] = 0.0;
  for (unsigned r = (unsigned)wv * rpw + grp; r < g.rpb; r += (unsigned)nw * rpw) {
    double wr = 1.0, wk[NA];                               // wk[m]: the weight with direction m's derivative entry, 1 <= m <= d - 2
#pragma unroll
    for (int c = 0; c < NA; c++) wk[c] = 1.0;
    unflatten<DC>(r, g.n, d - 1, [&](int m, unsigned i) {
      const unsigned nm = (unsigned)g.n[m];
      const size_t e = (size_t)a.P * g.off[m] + (size_t)p * nm + i;
      const double lv = a.rows[e];
      wr *= lv;
      if (GRAD) {
        const double ld = derivs ? a.rows[e + (size_t)a.H * nm] : 0.0;
#pragma unroll
        for (int c = 1; c < NA - 2; c++)
          if (c < d - 1) wk[c] *= c == m ? ld : lv;
      }
    });
    const double *pr = bv + (size_t)r * n;
    const bool al = ((size_t)pr & 15) == 0;
    double s = 0.0, sd = 0.0;
    for (unsigned j = 2 * l; j < n; j += 2 * lpr) {
      const d2 v = load_pair(pr, al, j, n);
      s += swl[j] * v.x + (j + 1 < n ? swl[j + 1] : 0.0) * v.y;
      if (GRAD) sd += swd[j] * v.x + (j + 1 < n ? swd[j + 1] : 0.0) * v.y;
    }
    acc[NA - 1] += wr * s;
#pragma unroll
    for (int c = 1; c < NA - 1; c++)
      if (c < d) acc[c] += c == d - 1 ? wr * sd : wk[c] * s;
  }
#pragma unroll
  for (int c = 0; c < NA; c++) {
    const double s = wave_sum(acc[c]);
    if (lane == 0) red[wv][c] = s;
  }
  __syncthreads();
  if (tid <= d && ((mask >> tid) & 1u)) {
    const int slot = tid == d ? NA - 1 : tid, c = tid == d ? vdst : tid;
    double s = red[0][slot];
    for (int q = 1; q < nw; q++) s += red[q][slot];
    a.out[((size_t)f * a.nc + c) * a.npts + p] = s * a.scale[c];
  }
}

// d = 1: the line product's two outputs are the result; W[f][p] the values, W[f][cnt + p] the derivatives of a chunk
__global__ __launch_bounds__(256) void k_points_grad1(const double *__restrict__ W, unsigned cnt, unsigned nf, int value, double s0,
                                                      double *__restrict__ out, size_t npts) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= cnt * nf) return;
  const unsigned f = i / cnt, p = i - f * cnt;
  const int nc = value ? 2 : 1;
  out[((size_t)f * nc) * npts + p] = W[(size_t)f * 2 * cnt + cnt + p] * s0;
  if (value) out[((size_t)f * nc + 1) * npts + p] = W[(size_t)f * 2 * cnt + p];
}

// LDS layout of k_points_spread's matrix chunk: Rt[k][point], the way the rows arrive (contiguous in the point of direction 0);
// the pitch keeps the 4 k a wave reads at once 128 B apart, as RS_XP does for the image
__device__ __forceinline__ int lds_rt(int k, int point, int bm) { return k * (bm + 16) + point; }

struct SpreadArgs {
  const double *rows;                // direction k's rows of this pass at rows + P off[k]
  const double *s;                   // s[f][p] of this pass at s[f npts + p]
  const double *iw;                  // inverse quadrature weights, direction k at off[k]; null: no scaling
  double *out;
  size_t npts;
  unsigned P, cnt, L, Q;             // row capacity of the pass, its points, lines nf Q, Q = n_1 .. n_{d-1}
  int accumulate;
};

// out[f][i_0][q] (+)= sum over the pass's points of rows_0[p][i_0] X[p][(f, q)]: workgroup (line tile, point tile), 4 waves as
// 2 x 2 of BM/2 points x 32 lines.  DC: d known at compile time (1 .. 3), 0: any d up to MD.
template <int DC, int BM>
__global__ __launch_bounds__(256) void k_points_spread(const PtGeo g, const SpreadArgs a) {
  __shared__ double sR[RS_KC * (BM + 16)];
  __shared__ double sX[RS_KC * RS_XP];
  constexpr int MT = BM / 32;                    // m-tiles of 16 points per wave
  constexpr int XN = RS_KC * RS_BN / 256;        // image elements a thread forms per chunk
  constexpr int RN = BM * RS_KC / 256;           // matrix elements a thread loads per chunk
  constexpr int DM = DC ? DC : MD;
  const int d = DC ? DC : g.d;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kq = lane >> 4, l16 = lane & 15;
  const int pw = (w >> 1) * (BM / 2), lw = (w & 1) * 32;     // this wave's first point / line within the tile
  const unsigned M = (unsigned)g.n[0], Q = a.Q, L = a.L, cnt = a.cnt;
  const unsigned l0 = blockIdx.x * RS_BN, i0 = blockIdx.y * BM;

  // the weight of a line under CHEB_SPREAD_DELTA: iw_1[i_1] (.. iw_{d-1}[i_{d-1}]), built from the last direction down
  auto line_weight = [&](unsigned line) -> double {
    unsigned q = line % Q;
    double wq = 1.0;
#pragma unroll
    for (int k = DM - 1; k >= 1; k--)
      if (k < d) {
        const unsigned nk = (unsigned)g.n[k], i = k > 1 ? q % nk : q;
        q /= nk;
        wq = k == d - 1 ? a.iw[g.off[k] + i] : a.iw[g.off[k] + i] * wq;
      }
    return wq;
  };

  // a thread forms the image of one line at XN points of a chunk, and loads RN matrix elements, the same places in every chunk
  const unsigned xline = l0 + (unsigned)(tid & (RS_BN - 1));
  const bool xl = xline < L;
  const int xk = tid / RS_BN;                    // + 4 e
  unsigned ro[DM];                               // direction k's entry of the line at point p: rows[ro[k] + p n_k]
  size_t sb = 0;
  {
    const unsigned line = xl ? xline : 0u;
    unsigned q = line % Q;
    sb = (size_t)(line / Q) * a.npts;
#pragma unroll
    for (int k = DM - 1; k >= 1; k--) {
      ro[k] = 0;
      if (k < d) {
        const unsigned nk = (unsigned)g.n[k], i = k > 1 ? q % nk : q;
        q /= nk;
        ro[k] = a.P * g.off[k] + i;
      }
    }
  }
  // Loads carry no branch: an index past the pass's last point (or the grid's last node, or the last line) is clamped to it and
  // the value dropped by a select where the LDS slot is written, so the loads of the next chunk stay in flight during the products
  // and a padding slot is an exact zero whatever its clamped source holds.  d <= 3 keeps the factors and multiplies at the store.
  constexpr int XF = DC ? DC : 1;                // values kept per image element: s and the entries of directions 1 .. DC - 1
  double xv[XN][XF], rv[RN];
  auto load = [&](unsigned k0) {
#pragma unroll
    for (int e = 0; e < XN; e++) {
      const unsigned p = min(k0 + (unsigned)(xk + (256 / RS_BN) * e), cnt - 1);
      xv[e][0] = a.s[sb + p];
#pragma unroll
      for (int k = 1; k < DM; k++)
        if (k < d) {
          const double l = a.rows[ro[k] + p * (unsigned)g.n[k]];
          if (DC) xv[e][k < XF ? k : 0] = l; else xv[e][0] = xv[e][0] * l;
        }
    }
#pragma unroll
    for (int e = 0; e < RN; e++) {
      const int t = tid + 256 * e;
      rv[e] = a.rows[min(k0 + (unsigned)(t / BM), cnt - 1) * M + min(i0 + (unsigned)(t % BM), M - 1)];
    }
  };

  v4d acc[MT][2];
#pragma unroll
  for (int u = 0; u < MT; u++)
#pragma unroll
    for (int t = 0; t < 2; t++) acc[u][t] = (v4d){0.0, 0.0, 0.0, 0.0};

  load(0);
  for (unsigned k0 = 0; k0 < cnt; k0 += RS_KC) {
    __syncthreads();                             // (the previous chunk has been read)
#pragma unroll
    for (int e = 0; e < XN; e++) {
      const int kk = xk + (256 / RS_BN) * e;
      double x = xv[e][0];
#pragma unroll
      for (int k = 1; k < XF; k++) x = x * xv[e][k];
      sX[lds_x(kk, tid & (RS_BN - 1))] = (xl && k0 + (unsigned)kk < cnt) ? x : 0.0;
    }
#pragma unroll
    for (int e = 0; e < RN; e++) {
      const int t = tid + 256 * e;
      sR[lds_rt(t / BM, t % BM, BM)] = (i0 + (unsigned)(t % BM) < M && k0 + (unsigned)(t / BM) < cnt) ? rv[e] : 0.0;
    }
    __syncthreads();
    load(k0 + RS_KC);                            // next chunk in flight during the products (clamped past the end)
#pragma unroll
    for (int ks = 0; ks < RS_KC / 4; ks++) {
      double ra[MT], xb[2];
#pragma unroll
      for (int u = 0; u < MT; u++) ra[u] = sR[lds_rt(4 * ks + kq, pw + 16 * u + l16, BM)];
#pragma unroll
      for (int t = 0; t < 2; t++) xb[t] = sX[lds_x(4 * ks + kq, lw + 16 * t + l16)];
#pragma unroll
      for (int u = 0; u < MT; u++)
#pragma unroll
        for (int t = 0; t < 2; t++) acc[u][t] = line_mfma<false>(ra[u], xb[t], acc[u][t]);
    }
  }

  // C/D element r of a lane: point (lane >> 4) + 4 r, line lane & 15
#pragma unroll
  for (int t = 0; t < 2; t++) {
    const unsigned line = l0 + lw + 16 * t + l16;
    if (line >= L) continue;
    const unsigned f = line / Q, ob = f * M * Q + (line - f * Q);
    double wl = 1.0;
    if (a.iw && d > 1) wl = line_weight(line);
#pragma unroll
    for (int u = 0; u < MT; u++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const unsigned i = i0 + pw + 16 * u + 4 * r + kq;
        if (i >= M) continue;
        double v = acc[u][t][r];
        if (a.iw) { v = v * a.iw[i]; if (d > 1) v = v * wl; }
        double *o = a.out + ((size_t)ob + (size_t)i * Q);
        *o = a.accumulate ? *o + v : v;
      }
  }
}

int rows_lg(int n) {                 // log2 of the power of two >= n, at most 6
  int lg = 0;
  while (lg < 6 && (1 << lg) < n) lg++;
  return lg;
}

// The rows of a job: its CGL entries as one launch of k_points_rows, then its periodic ones as one launch of k_points_frows.  An
// entry is self-contained, so a launch takes the entries of its basis, in their order, as a job of their own; a basis with no
// entry, or with no coordinate, launches nothing.
int launch_rows(const RowsJob &job, hipStream_t st, const char *what) {
  for (int periodic = 0; periodic < 2; periodic++) {
    RowsJob part{};
    unsigned gx = 0;
    for (int i = 0; i < job.nd; i++) {
      const RowsEntry &e = job.e[i];
      if ((e.periodic != 0) != (periodic != 0)) continue;
      part.e[part.nd++] = e;
      const unsigned rpb = 4u * (64u >> e.lg);
      gx = std::max(gx, (e.m + rpb - 1) / rpb);
    }
    if (gx == 0) continue;
    void (*const kernel)(const RowsJob) = periodic ? k_points_frows : k_points_rows;
    hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)part.nd), dim3(256), 0, st, part);
    sweep_note_launch();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)      // (two-part name: not check_launch)
      return chebhip_fail(CHEBHIP_ERR_DEVICE, "%s %srows launch: %s", what, periodic ? "periodic " : "", hipGetErrorString(e));
  }
  return 0;
}

// a multi-index of first derivatives: d host ints, each 0 or 1; NULL = all zero
int check_deriv(int d, const int *deriv, const char *what) {
  for (int k = 0; deriv && k < d; k++)
    if (deriv[k] != 0 && deriv[k] != 1) return chebhip_fail(CHEBHIP_ERR_ARG, "%s: deriv[%d] = %d must be 0 or 1", what, k, deriv[k]);
  return 0;
}

// fn(std::integral_constant<int, DC>) for the kernels' template argument DC: d where a kernel is built for it (1 .. 3), 0 above
template <class F>
void dispatch_dc(int d, F fn) {
  switch (d) {
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 3: fn(std::integral_constant<int, 3>{}); break;
    default: fn(std::integral_constant<int, 0>{});
  }
}

// one launch of the contraction (d >= 2: at d = 1 the line product's output is the result); the caller checks it (check_launch)
template <bool GRAD>
void contract_launch(int d, dim3 grid, dim3 block, hipStream_t st, const PtGeo &g, const ConArgs &a) {
  dispatch_dc(d, [&](auto dc) {
    constexpr int DC = decltype(dc)::value > 1 ? decltype(dc)::value : 0;
    hipLaunchKernelGGL((k_points_contract<DC, GRAD>), grid, block, 0, st, g, a);
  });
}

// what the three *_matrix_host entries check after n, and their work: fill() writes the m rows
template <class F>
int matrix_host(int m, int deriv, const double *x, const double *R, F fill) {
  if (m < 0) return chebhip_fail(CHEBHIP_ERR_ARG, "m = %d is negative", m);
  if (deriv != 0 && deriv != 1) return chebhip_fail(CHEBHIP_ERR_ARG, "deriv = %d must be 0 or 1", deriv);
  if (m == 0) return 0;
  if (!x || !R) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  fill();
  return 0;
}

}  // namespace

struct cheb_points {
  int d = 0, nf = 1;
  long total = 0;                            // nf * prod(dims)
  unsigned C = 0;                            // points per chunk
  PtGeo geo{};
  int basis[MD] = {0};                       // CHEB_BASIS_* per direction (cheb_points_create_basis; all CGL otherwise)
  std::map<int, double *> nodes;             // device node table per distinct extent of a CGL direction
  std::map<int, double *> ftab;              // device table of fourier_points_table_host per distinct extent of a periodic direction
  const double *table(int k) const { return basis[k] ? ftab.at(geo.n[k]) : nodes.at(geo.n[k]); }
  double *rows = nullptr;                    // C x n_k rows of every direction, direction k at C geo.off[k]
  double *W = nullptr;                       // nf x C x B: direction 0's output
  double *iw = nullptr;                      // spread's CHEB_SPREAD_DELTA: 1 / Clenshaw-Curtis weight, direction k at geo.off[k]; made at first use
  // tensor grids (cheb_points_grid_reserve)
  int mmax[MD] = {0};
  size_t goff[MD] = {0};                     // direction k's rows in grows
  double *grows = nullptr;
  double *gwork[2] = {nullptr, nullptr};     // ping-pong intermediates
};

namespace {
// direction k's entry of a rows job: the value rows of the m coordinates x[i stride] into R
RowsEntry rows_entry(const cheb_points *h, int k, const double *x, long stride, unsigned m, double *R) {
  const int n = h->geo.n[k];
  return RowsEntry{n, rows_lg(n), 1, h->basis[k] != CHEB_BASIS_CGL, m, stride, x, h->table(k), R, R};
}

// the rows job of a chunk of cnt scattered points xi[p][k]: direction k's rows at base + cap off[k]
RowsJob chunk_job(const cheb_points *h, const double *xi, unsigned cnt, double *base, size_t cap) {
  RowsJob job{};
  job.nd = h->d;
  for (int k = 0; k < h->d; k++) job.e[k] = rows_entry(h, k, xi + k, h->d, cnt, base + cap * h->geo.off[k]);
  return job;
}

// a flagged direction's derivative rows where its value rows would go (deriv null: none flagged)
void job_deriv(RowsJob &job, const int *deriv) {
  for (int k = 0; deriv && k < job.nd; k++)
    if (deriv[k]) { job.e[k].what = 2; job.e[k].D = job.e[k].R; }
}
}  // namespace

extern "C" int cheb_nodes_host(int n, double *x) {
  int rc;
  if ((rc = check_extent(n))) return rc;
  if (!x) return chebhip_fail(CHEBHIP_ERR_ARG, "x is NULL");
  points_nodes_host(n, x);
  return 0;
}

extern "C" int cheb_points_matrix_host(int n, int m, const double *x, double *R) {
  int rc;
  if ((rc = check_extent(n))) return rc;
  return matrix_host(m, 0, x, R, [&] { points_matrix_host(n, m, x, R); });
}

namespace {
void free_grid(cheb_points *h) {
  if (h->grows) (void)hipFree(h->grows);
  for (double *&b : h->gwork) { if (b) (void)hipFree(b); b = nullptr; }
  h->grows = nullptr;
  for (int k = 0; k < MD; k++) h->mmax[k] = 0;
}
}  // namespace

extern "C" int cheb_points_destroy(cheb_points *h) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  for (auto &t : h->nodes) if (t.second) (void)hipFree(t.second);
  for (auto &t : h->ftab) if (t.second) (void)hipFree(t.second);
  if (h->rows) (void)hipFree(h->rows);
  if (h->W) (void)hipFree(h->W);
  if (h->iw) (void)hipFree(h->iw);
  free_grid(h);
  delete h;
  return 0;
}

// basis null: cheb_points_create
static int points_create(int d, const int *dims, int nfields, const int *basis, cheb_points **out) {
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  int rc;
  long N = 0, S = 0;
  if ((rc = check_field_grid(d, dims, basis, nfields, &N, &S))) return rc;
  if ((rc = require_device())) return rc;
  const long total = nfields * N;
  cheb_points *h = new (std::nothrow) cheb_points;
  if (!h) return chebhip_fail(CHEBHIP_ERR_MEMORY, "out of host memory");
  h->d = d; h->nf = nfields; h->total = total;
  for (int k = 0; k < d; k++) h->basis[k] = basis ? basis[k] : CHEB_BASIS_CGL;
  PtGeo &g = h->geo;
  g.d = d;
  for (int k = 0; k < d; k++) g.n[k] = dims[k];
  table_offsets(d, dims, g.off);
  g.B = (unsigned)(N / dims[0]);
  g.rpb = g.B / (unsigned)dims[d - 1];
  g.lg = row_lanes_lg(dims[d - 1]);

  // the chunk: rows and direction 0's output within max(bytes of the fields, 32 MiB); a multiple of 128 (the line product's
  // tile of output points), of 64 below that, whatever fits below 64
  const long cap = std::max(total * (long)sizeof(double), WORK_MIN) / (long)sizeof(double);
  const long per = S + (long)nfields * g.B;
  long C = std::min(1024L, cap / per);
  if (C >= 128) C -= C % 128; else if (C >= 64) C = 64;
  if (C < 1) { delete h; return chebhip_fail(CHEBHIP_ERR_DIMS, "no room for one point's work memory"); }
  h->C = (unsigned)C;

  std::vector<double> x;
  for (int k = 0; k < d && !rc; k++) {
    const int nk = dims[k];
    if (h->basis[k] == CHEB_BASIS_FOURIER) {
      if (h->ftab.count(nk)) continue;
      x.resize((size_t)3 * nk);
      fourier_points_table_host(nk, x.data());
      double *dev = nullptr;
      if (!(rc = device_array(&dev, (size_t)3 * nk, x.data(), "periodic node table"))) h->ftab[nk] = dev;
      continue;
    }
    if (h->nodes.count(nk)) continue;
    x.resize(nk);
    points_nodes_host(nk, x.data());
    double *dev = nullptr;
    if (!(rc = device_array(&dev, nk, x.data(), "node table"))) h->nodes[nk] = dev;
  }
  if (!rc) rc = device_array(&h->rows, (size_t)C * S, nullptr, "interpolation rows");
  if (!rc) rc = device_array(&h->W, (size_t)C * nfields * g.B, nullptr, "points work buffer");
  if (rc) { cheb_points_destroy(h); return rc; }
  *out = h;
  return 0;
}

extern "C" int cheb_points_create(int d, const int *dims, int nfields, cheb_points **out) {
  return points_create(d, dims, nfields, nullptr, out);
}

extern "C" int cheb_points_create_basis(int d, const int *dims, int nfields, const int *basis, cheb_points **out) {
  if (out) *out = nullptr;
  if (!basis) return chebhip_fail(CHEBHIP_ERR_ARG, "basis is NULL");
  return points_create(d, dims, nfields, basis, out);
}

extern "C" int cheb_points_fourier_matrix_host(int n, int m, const double *x, int deriv, double *R) {
  if (n < 2) return chebhip_fail(CHEBHIP_ERR_SIZE, "n = %d: a periodic direction needs at least 2 points", n);
  if (n > 256) return chebhip_fail(CHEBHIP_ERR_ARG, "n = %d: a periodic direction supports at most 256 points", n);
  return matrix_host(m, deriv, x, R, [&] { fourier_points_matrix_host(n, m, x, deriv, R); });
}

extern "C" long cheb_points_chunk(const cheb_points *h) { return h ? (long)h->C : -1; }

// cheb_points_rows (deriv 0) and cheb_points_drows (deriv 1): the m rows of direction k into R
static int rows_run(cheb_points *h, int k, const double *x, long m, int deriv, double *R, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (k < 0 || k >= h->d) return chebhip_fail(CHEBHIP_ERR_TDIM, "direction %d out of range 0..%d", k, h->d - 1);
  if (m < 0 || m >= 0x80000000L) return chebhip_fail(CHEBHIP_ERR_ARG, "m = %ld must be in 0..2^31-1", m);
  if (m == 0) return 0;
  if (!x || !R) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  RowsJob job{};
  job.nd = 1;
  job.e[0] = rows_entry(h, k, x, 1, (unsigned)m, R);
  job_deriv(job, &deriv);
  return launch_rows(job, (hipStream_t)stream, "points");
}

extern "C" int cheb_points_rows(cheb_points *h, int k, const double *x, long m, double *R, void *stream) {
  return rows_run(h, k, x, m, 0, R, stream);
}

extern "C" int cheb_points_drows(cheb_points *h, int k, const double *x, long m, double *R, void *stream) {
  return rows_run(h, k, x, m, 1, R, stream);
}

extern "C" int cheb_points_dmatrix_host(int n, int m, const double *x, double *R) {
  int rc;
  if ((rc = check_extent(n))) return rc;
  return matrix_host(m, 0, x, R, [&] { points_dmatrix_host(n, m, x, R); });
}

namespace {
int eval_run(cheb_points *h, const double *u, const double *xi, long npts, const int *deriv, double *out, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (npts < 0) return chebhip_fail(CHEBHIP_ERR_ARG, "npts = %ld is negative", npts);
  if (npts == 0) return 0;
  if (!u || !xi || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (overlap(u, h->total, out, h->nf * npts)) return chebhip_fail(CHEBHIP_ERR_ARG, "eval: fields and output must not overlap");
  hipStream_t st = (hipStream_t)stream;
  const PtGeo &g = h->geo;
  const int d = h->d;
  const long C = h->C;
  int rc;
  ConArgs a{};                                             // the contraction's one sum, out[f][p]
  a.rows = h->rows; a.P = (unsigned)C; a.V = h->W; a.npts = (size_t)npts; a.nc = 1; a.mask = 1u << d;
  for (double &s : a.scale) s = 1.0;
  for (long p0 = 0; p0 < npts; p0 += C) {
    const unsigned cnt = (unsigned)std::min(C, npts - p0);
    RowsJob job = chunk_job(h, xi + (size_t)p0 * d, cnt, h->rows, (size_t)C);
    job_deriv(job, deriv);
    if ((rc = launch_rows(job, st, "eval"))) return rc;
    // d == 1: the line product's [field][point] is the result where it is one chunk or one field
    const bool direct = d == 1 && (h->nf == 1 || cnt == npts);
    ResampleDir p{h->rows, u, direct ? out + p0 : h->W, (unsigned)h->nf, (unsigned)g.n[0], cnt, g.B, (unsigned)h->nf * g.B};
    hipError_t e = resample_launch(p, st);
    if (e != hipSuccess) return chebhip_fail(CHEBHIP_ERR_DEVICE, "eval line product launch: %s", hipGetErrorString(e));
    if (d == 1) {
      if (!direct) {
        e = hipMemcpy2DAsync(out + p0, (size_t)npts * sizeof(double), h->W, (size_t)cnt * sizeof(double), (size_t)cnt * sizeof(double),
                             (size_t)h->nf, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return chebhip_fail(CHEBHIP_ERR_DEVICE, "eval copy: %s", hipGetErrorString(e));
      }
      continue;
    }
    a.bs = cnt; a.out = out + p0;
    contract_launch<false>(d, dim3(cnt, (unsigned)h->nf), dim3(g.B <= 1024 ? 64 : 256), st, g, a);
    if ((rc = check_launch("eval contraction"))) return rc;
  }
  return 0;
}
}  // namespace

extern "C" int cheb_points_eval(cheb_points *h, const double *u, const double *xi, long npts, double *out, void *stream) {
  return eval_run(h, u, xi, npts, nullptr, out, stream);
}

extern "C" int cheb_points_eval_deriv(cheb_points *h, const double *u, const double *xi, long npts, const int *deriv, double *out,
                                      void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  int rc;
  if ((rc = check_deriv(h->d, deriv, "eval_deriv"))) return rc;
  return eval_run(h, u, xi, npts, deriv, out, stream);
}

extern "C" int cheb_points_eval_grad(cheb_points *h, const double *u, const double *xi, long npts, const double *scale, int flags,
                                     double *out, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (npts < 0) return chebhip_fail(CHEBHIP_ERR_ARG, "npts = %ld is negative", npts);
  if (flags & ~CHEB_POINTS_GRAD_VALUE) return chebhip_fail(CHEBHIP_ERR_ARG, "eval_grad: unknown flags %d", flags);
  const int d = h->d, value = (flags & CHEB_POINTS_GRAD_VALUE) ? 1 : 0, nc = d + value;
  for (int k = 0; scale && k < d; k++)
    if (!std::isfinite(scale[k])) return chebhip_fail(CHEBHIP_ERR_ARG, "eval_grad: scale[%d] is not finite", k);
  if (npts == 0) return 0;
  if (!u || !xi || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (overlap(u, h->total, out, (long)h->nf * nc * npts)) return chebhip_fail(CHEBHIP_ERR_ARG, "eval_grad: fields and output must not overlap");
  hipStream_t st = (hipStream_t)stream;
  const PtGeo &g = h->geo;
  const long C = h->C, H = C / 2;                          // a gradient chunk: half an eval chunk, two row sets and two blocks a point
  const unsigned nf = (unsigned)h->nf;
  int rc;
  ConArgs a{};
  a.rows = h->rows; a.out = out; a.npts = (size_t)npts; a.nc = nc;
  for (int k = 0; k <= MD; k++) a.scale[k] = (scale && k < d) ? scale[k] : 1.0;
  const dim3 block(g.B <= 1024 ? 64 : 256);

  if (H == 0) {
    // The work memory holds one point's value rows and one block (a first direction of two nodes under fields of 32 MiB or
    // more): a point takes one pass of the eval pipeline per component, the rows of direction c exchanged for its derivative
    // rows, and the contraction stores the value sum as component c.
    a.P = 1; a.H = 0; a.V = h->W; a.D = nullptr; a.bs = 1; a.mask = 1u << d;
    for (long p = 0; p < npts; p++)
      for (int c = 0; c < nc; c++) {
        RowsJob job = chunk_job(h, xi + (size_t)p * d, 1u, h->rows, 1);
        if (c < d) job.e[c].what = 2;
        if ((rc = launch_rows(job, st, "eval_grad"))) return rc;
        ResampleDir lp{h->rows, u, h->W, nf, (unsigned)g.n[0], 1u, g.B, nf * g.B};
        hipError_t e = resample_launch(lp, st);
        if (e != hipSuccess) return chebhip_fail(CHEBHIP_ERR_DEVICE, "eval_grad line product launch: %s", hipGetErrorString(e));
        a.out = out + p; a.vdst = c;
        contract_launch<false>(d, dim3(1, nf), block, st, g, a);
        if ((rc = check_launch("eval_grad contraction"))) return rc;
      }
    return 0;
  }

  a.P = (unsigned)(2 * H); a.H = (unsigned)H; a.mask = ((1u << d) - 1u) | (value ? 1u << d : 0u); a.vdst = d;
  for (long p0 = 0; p0 < npts; p0 += H) {
    const unsigned cnt = (unsigned)std::min(H, npts - p0);
    // direction 0: cnt value rows, then cnt derivative rows, one matrix of 2 cnt rows; direction k >= 1: its value rows at
    // rows + 2 H off[k], its derivative rows H n_k values further
    RowsJob job = chunk_job(h, xi + (size_t)p0 * d, cnt, h->rows, (size_t)(2 * H));
    for (int k = 0; k < d; k++) { job.e[k].what = 3; job.e[k].D = job.e[k].R + (size_t)(k == 0 ? cnt : H) * g.n[k]; }
    if ((rc = launch_rows(job, st, "eval_grad"))) return rc;
    ResampleDir lp{h->rows, u, h->W, nf, (unsigned)g.n[0], 2 * cnt, g.B, nf * g.B};
    hipError_t e = resample_launch(lp, st);
    if (e != hipSuccess) return chebhip_fail(CHEBHIP_ERR_DEVICE, "eval_grad line product launch: %s", hipGetErrorString(e));
    if (d == 1) {
      hipLaunchKernelGGL(k_points_grad1, dim3((cnt * nf + 255) / 256), dim3(256), 0, st, h->W, cnt, nf, value, a.scale[0], out + p0,
                         (size_t)npts);
    } else {
      a.V = h->W; a.D = h->W + (size_t)cnt * g.B; a.bs = 2 * cnt; a.out = out + p0;
      contract_launch<true>(d, dim3(cnt, nf, 2), block, st, g, a);
    }
    if ((rc = check_launch("eval_grad contraction"))) return rc;
  }
  return 0;
}

namespace {
// spread keeps the rows of a pass in the larger of the handle's two work arrays: direction k at P off[k]
struct SpreadPass { double *buf; long P; };
SpreadPass spread_pass(const cheb_points *h) {
  const PtGeo &g = h->geo;
  const long S = (long)g.off[h->d - 1] + g.n[h->d - 1], inW = (long)h->C * h->nf * (long)g.B / S;
  SpreadPass sp = inW > (long)h->C ? SpreadPass{h->W, inW} : SpreadPass{h->rows, (long)h->C};
  if (sp.P >= RS_KC) sp.P -= sp.P % RS_KC;       // whole LDS chunks
  const long cap = opt(OPT_POINTS_SPREAD_PASS);
  if (cap > 0 && cap < sp.P) sp.P = cap;
  return sp;
}

int spread_weights(cheb_points *h) {             // the inverse quadrature weights, uploaded once
  if (h->iw) return 0;
  const PtGeo &g = h->geo;
  std::vector<double> w, iw;
  for (int k = 0; k < h->d; k++) {
    if (h->basis[k] == CHEB_BASIS_FOURIER) {               // the weight 2 / n of every node of a periodic direction
      for (int j = 0; j < g.n[k]; j++) iw.push_back(0.5 * (double)g.n[k]);
      continue;
    }
    w.resize(g.n[k]);
    modal_weights_host(g.n[k], w.data());
    for (double v : w) iw.push_back((double)(1.0L / (long double)v));
  }
  return device_array(&h->iw, iw.size(), iw.data(), "inverse quadrature weights");
}

template <int BM>
void spread_launch(int d, const PtGeo &g, const SpreadArgs &a, hipStream_t st) {
  const dim3 grid((a.L + RS_BN - 1) / RS_BN, ((unsigned)g.n[0] + BM - 1) / BM);
  dispatch_dc(d, [&](auto dc) { hipLaunchKernelGGL((k_points_spread<decltype(dc)::value, BM>), grid, dim3(256), 0, st, g, a); });
}
}  // namespace

extern "C" long cheb_points_spread_pass(const cheb_points *h) { return h ? spread_pass(h).P : -1; }

namespace {
int spread_run(cheb_points *h, const double *s, const double *xi, long npts, const int *deriv, double *out, int flags, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  if (npts < 0) return chebhip_fail(CHEBHIP_ERR_ARG, "npts = %ld is negative", npts);
  if (flags & ~(CHEB_SPREAD_ACCUMULATE | CHEB_SPREAD_DELTA)) return chebhip_fail(CHEBHIP_ERR_ARG, "spread: unknown flags %d", flags);
  hipStream_t st = (hipStream_t)stream;
  const bool accumulate = flags & CHEB_SPREAD_ACCUMULATE;
  if (npts == 0 && accumulate) return 0;
  if (!out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (npts == 0) {
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)h->total * sizeof(double), st));
    return 0;
  }
  if (!s || !xi) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  const int d = h->d;
  if (overlap(out, h->total, s, h->nf * npts) || overlap(out, h->total, xi, npts * d))
    return chebhip_fail(CHEBHIP_ERR_ARG, "spread: the output must not overlap the strengths or the coordinates");
  int rc;
  if ((flags & CHEB_SPREAD_DELTA) && (rc = spread_weights(h))) return rc;
  const PtGeo &g = h->geo;
  const SpreadPass sp = spread_pass(h);
  for (long p0 = 0; p0 < npts; p0 += sp.P) {
    const unsigned cnt = (unsigned)std::min(sp.P, npts - p0);
    RowsJob job = chunk_job(h, xi + (size_t)p0 * d, cnt, sp.buf, (size_t)sp.P);
    job_deriv(job, deriv);
    if ((rc = launch_rows(job, st, "spread"))) return rc;
    const SpreadArgs a{sp.buf, s + p0, (flags & CHEB_SPREAD_DELTA) ? h->iw : nullptr, out, (size_t)npts,
                       (unsigned)sp.P, cnt, (unsigned)h->nf * g.B, g.B, (accumulate || p0 > 0) ? 1 : 0};
    if (g.n[0] > 64) spread_launch<128>(d, g, a, st); else spread_launch<64>(d, g, a, st);
    if ((rc = check_launch("spread"))) return rc;
  }
  return 0;
}
}  // namespace

extern "C" int cheb_points_spread(cheb_points *h, const double *s, const double *xi, long npts, double *out, int flags, void *stream) {
  return spread_run(h, s, xi, npts, nullptr, out, flags, stream);
}

extern "C" int cheb_points_spread_deriv(cheb_points *h, const double *s, const double *xi, long npts, const int *deriv, double *out,
                                        int flags, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL handle");
  int rc;
  if ((rc = check_deriv(h->d, deriv, "spread_deriv"))) return rc;
  return spread_run(h, s, xi, npts, deriv, out, flags, stream);
}

extern "C" int cheb_points_grid_reserve(cheb_points *h, const int *m_max) {
  if (!h || !m_max) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  const int d = h->d;
  long bound = h->nf;
  size_t nrows = 0;
  for (int k = 0; k < d; k++) {
    if (m_max[k] < 1) return chebhip_fail(CHEBHIP_ERR_ARG, "m_max[%d] = %d must be >= 1", k, m_max[k]);
    bound *= std::max(m_max[k], h->geo.n[k]);
    if (bound >= 0x80000000L) return chebhip_fail(CHEBHIP_ERR_DIMS, "a grid of 2^31 values or more");
    nrows += (size_t)m_max[k] * h->geo.n[k];
  }
  if (hipDeviceSynchronize() != hipSuccess) return chebhip_fail(CHEBHIP_ERR_DEVICE, "grid_reserve: device synchronisation failed");
  free_grid(h);
  // an intermediate has m_k or n_k points in direction k: at most `bound` values, whatever order the directions run in
  hipError_t e = hipMalloc(&h->grows, nrows * sizeof(double));
  for (int b = 0; b < 2 && b < d - 1 && e == hipSuccess; b++) e = hipMalloc(&h->gwork[b], (size_t)bound * sizeof(double));
  if (e != hipSuccess) { free_grid(h); return chebhip_fail(CHEBHIP_ERR_MEMORY, "grid buffers: %s", hipGetErrorString(e)); }
  size_t o = 0;
  for (int k = 0; k < d; k++) { h->mmax[k] = m_max[k]; h->goff[k] = o; o += (size_t)m_max[k] * h->geo.n[k]; }
  return 0;
}

namespace {
int grid_run(cheb_points *h, const double *u, const double *coords, const int *m, const int *deriv, double *out, void *stream) {
  if (!h || !m) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  const int d = h->d;
  const PtGeo &g = h->geo;
  long nout = h->nf;
  for (int k = 0; k < d; k++) {
    if (m[k] < 0) return chebhip_fail(CHEBHIP_ERR_ARG, "m[%d] = %d is negative", k, m[k]);
    if (m[k] > h->mmax[k]) return chebhip_fail(CHEBHIP_ERR_ARG, "m[%d] = %d exceeds the reserved %d (cheb_points_grid_reserve)", k, m[k], h->mmax[k]);
    nout *= m[k];
  }
  if (nout == 0) return 0;
  if (!u || !coords || !out) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  if (overlap(u, h->total, out, nout)) return chebhip_fail(CHEBHIP_ERR_ARG, "eval_grid: fields and output must not overlap");
  hipStream_t st = (hipStream_t)stream;
  RowsJob job{};
  job.nd = d;
  size_t co = 0;
  for (int k = 0; k < d; co += m[k], k++) job.e[k] = rows_entry(h, k, coords + co, 1, (unsigned)m[k], h->grows + h->goff[k]);
  job_deriv(job, deriv);
  int rc;
  if ((rc = launch_rows(job, st, "eval_grid"))) return rc;
  int order[MD];
  long cur[MD];
  for (int k = 0; k < d; k++) { order[k] = k; cur[k] = g.n[k]; }
  order_by_ratio(order, order + d, m, g.n);                    // shrinking directions first
  LineStep steps[MD];
  for (int s = 0; s < d; s++) steps[s] = LineStep{order[s], h->grows + h->goff[order[s]], m[order[s]]};
  hipError_t e = line_chain(d, cur, h->nf, 1, d, steps, u, out, h->gwork, st);
  return e == hipSuccess ? 0 : chebhip_fail(CHEBHIP_ERR_DEVICE, "eval_grid launch: %s", hipGetErrorString(e));
}
}  // namespace

extern "C" int cheb_points_eval_grid(cheb_points *h, const double *u, const double *coords, const int *m, double *out, void *stream) {
  return grid_run(h, u, coords, m, nullptr, out, stream);
}

extern "C" int cheb_points_eval_grid_deriv(cheb_points *h, const double *u, const double *coords, const int *m, const int *deriv,
                                           double *out, void *stream) {
  if (!h) return chebhip_fail(CHEBHIP_ERR_ARG, "NULL argument");
  int rc;
  if ((rc = check_deriv(h->d, deriv, "eval_grid_deriv"))) return rc;
  return grid_run(h, u, coords, m, deriv, out, stream);
}
