// opfun.hip -- functions of the Helmholtz operator B = sigma - sum_k s_k^2 d_k^2 in its own eigenbasis (cheb_opfun_*):
//     y_o = S [ sum_{terms t of output o} c_t f_t(s) .* (S^-1 x_{i_t}) ],   s = ((sigma + l_0[i_0]) + l_1[i_1]) + ...
// The line transforms are the solver's (precond.hip, which also holds the handle); this file has the one pointwise kernel between
// them, the weight functions' entry points (cheb_opfun_eval on the device, cheb_opfun_weight_host in long double) and the table.
//
// k_opfun_mix: one pass in mode space.  A block owns a piece of one line of the last dimension (d <= 3: the partial sum
// (sigma + l_0) + l_1 once per block, no 64-bit division per element), a lane one mode of it: it evaluates each distinct
// (kind, tau, par) of the table once, then walks the outputs and their terms in table order -- both loops uniform across the wave,
// every field access a coalesced 8-byte column of the stacked fields.  k_opfun_mix_nd forms s by the index chain of k_modal_scale
// for d > 3 (and for more than 65535 lines).  No LDS, no atomics; the table is a by-value argument.
#include "../../include/chebhip.h"
#include "opfun.h"
#include "opfun_fn.h"
#include "ops.h"
#include "sweep.h"
#include <cmath>

using namespace chebhip;

namespace {

constexpr int MD = 10;
struct MixGeo { int d; long gs[MD]; const double *lam[MD]; };

// The mode's weights, then its outputs term by term.  NW: the distinct weights a lane keeps in registers (4 or 32: the launch takes
// the smaller that holds the table's, for occupancy).  w[] is only ever indexed by constants: a term's weight is picked by selects
// on a wave-uniform number, so the array never leaves the registers.
template <int NW>
__device__ __forceinline__ void mix_point(const OpfunTable &tb, double s, long G, const double *__restrict__ x, double *__restrict__ y) {
  double w[NW];
#pragma unroll
  for (int v = 0; v < NW; v++) w[v] = 0.0;
  for (int u = 0; u < tb.nweights; u++) {                 // (rolled: one copy of the functions' code)
    const double wu = opfun::weight(tb.kind[u], tb.tau[u], tb.par[u], s);
#pragma unroll
    for (int v = 0; v < NW; v++) w[v] = u == v ? wu : w[v];
  }
  for (int o = 0; o < tb.nout; o++) {
    double acc = 0.0;
    for (int t = tb.first[o]; t < tb.first[o + 1]; t++) {
      const int u = tb.slot[t];
      double wt = w[0];
#pragma unroll
      for (int v = 1; v < NW; v++) wt = u == v ? w[v] : wt;
      acc += (tb.coef[t] * wt) * x[(long)tb.in[t] * G];
    }
    y[(long)o * G] = acc;
  }
}

template <int NW>
__global__ __launch_bounds__(256) void k_opfun_mix(const OpfunTable tb, int d, int n1, int nl, long G, const double *__restrict__ l0,
                                                   const double *__restrict__ l1, const double *__restrict__ l2,
                                                   const double *__restrict__ x, double *__restrict__ y) {
  const unsigned line = blockIdx.y;                       // d = 3: i0 * n1 + i1; d = 2: i0; d = 1: 0
  double s0 = 0.0;
  if (d == 3) { const unsigned i0 = line / (unsigned)n1, i1 = line - i0 * (unsigned)n1; s0 = l0[i0] + l1[i1]; }
  else if (d == 2) s0 = l0[line];
  const double *ll = d == 3 ? l2 : (d == 2 ? l1 : l0);
  const long row = (long)line * nl;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nl; i += gridDim.x * 256) mix_point<NW>(tb, s0 + ll[i], G, x + row + i, y + row + i);
}

template <int NW>
__global__ __launch_bounds__(256) void k_opfun_mix_nd(const OpfunTable tb, MixGeo geo, long G, const double *__restrict__ x, double *__restrict__ y) {
  GS_LOOP(q, G) {
    long g = q; double s = 0.0;
    for (int j = 0; j < geo.d; j++) { const long i = g / geo.gs[j]; g -= i * geo.gs[j]; s += geo.lam[j][i]; }
    mix_point<NW>(tb, s, G, x + q, y + q);
  }
}

__global__ __launch_bounds__(256) void k_opfun_eval(int kind, double tau, double par, long n, const double *__restrict__ s, double *__restrict__ w) {
  GS_LOOP(i, n) w[i] = opfun::weight(kind, tau, par, s[i]);
}

// phi_k(z) in long double: the nested series for |z| <= 1 (40 levels: exact to the last bit or two of the 64), the recurrence beyond
long double phi_host(int k, long double z) {
  long double fact = 1.0L;
  for (int j = 2; j <= k; j++) fact *= j;
  if (fabsl(z) <= 1.0L) {
    long double r = 1.0L;
    for (int j = 40; j >= 1; j--) r = 1.0L + z / (long double)(k + j) * r;
    return r / fact;
  }
  long double p = expm1l(z) / z, f = 1.0L;
  for (int j = 1; j < k; j++) { p = (p - 1.0L / f) / z; f *= (j + 1); }
  return p;
}

}  // namespace

namespace chebhip {

int opfun_check_weight(int kind, double tau, double par) {
  if (kind < 0 || kind >= opfun::NKINDS) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: kind = %d is not one of CHEB_OPFUN_ONE .. CHEB_OPFUN_POW", kind);
  if ((kind == opfun::K_EXP || (kind >= opfun::K_PHI1 && kind <= opfun::K_PHI3)) && !(std::isfinite(tau) && tau >= 0.0))
    return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: tau = %g must be finite and >= 0 for exp and phi_k", tau);
  if (kind == opfun::K_RES && !(std::isfinite(tau) && std::isfinite(par))) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: res needs finite par and tau (%g, %g)", par, tau);
  if (kind == opfun::K_POW && !std::isfinite(par)) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: pow needs a finite exponent, got %g", par);
  return 0;
}

int opfun_build_table(int nin, int nout, int nterms, const cheb_opfun_term *terms, OpfunTable *tb) {
  if (nterms < 0 || nterms > OPFUN_MAX_TERMS) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: %d terms, at most %d", nterms, OPFUN_MAX_TERMS);
  if (nterms > 0 && !terms) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: terms is NULL");
  for (int t = 0; t < nterms; t++) {
    const cheb_opfun_term &e = terms[t];
    if (e.out < 0 || e.out >= nout) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: term %d writes output %d of %d", t, e.out, nout);
    if (e.in < 0 || e.in >= nin) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: term %d reads input %d of %d", t, e.in, nin);
    if (!std::isfinite(e.coef)) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: term %d has coefficient %g", t, e.coef);
    int rc = opfun_check_weight(e.kind, e.tau, e.par); if (rc) return rc;
  }
  OpfunTable b = {};
  b.nin = (unsigned char)nin; b.nout = (unsigned char)nout;
  int n = 0;
  for (int o = 0; o < nout; o++) {
    b.first[o] = (unsigned char)n;
    for (int t = 0; t < nterms; t++) {
      const cheb_opfun_term &e = terms[t];
      if (e.out != o) continue;
      // what a kind does not read does not tell two weights apart
      const bool use_tau = e.kind >= opfun::K_RES && e.kind <= opfun::K_PHI3, use_par = e.kind == opfun::K_RES || e.kind == opfun::K_POW;
      const double tau = use_tau ? e.tau : 0.0, par = use_par ? e.par : 0.0;
      int u = 0;
      while (u < b.nweights && !(b.kind[u] == e.kind && b.tau[u] == tau && b.par[u] == par)) u++;
      if (u == b.nweights) { b.kind[u] = (unsigned char)e.kind; b.tau[u] = tau; b.par[u] = par; b.nweights++; }
      b.coef[n] = e.coef; b.in[n] = (unsigned char)e.in; b.slot[n] = (unsigned char)u;
      n++;
    }
  }
  for (int o = nout; o <= OPFUN_MAX_FIELDS; o++) b.first[o] = (unsigned char)n;
  *tb = b;
  return 0;
}

int opfun_mix_launch(const OpfunTable &tb, int d, const int *M, long G, const double *const *lam, const double *x, double *y, hipStream_t st) {
  if (G == 0) return 0;
  const int nl = M[d - 1];
  const long lines = G / nl;
  const bool few = tb.nweights <= 4;
  if (d <= 3 && lines <= 65535) {
    const dim3 grid((unsigned)((nl + 255) / 256), (unsigned)lines);
    const int n1 = d == 3 ? M[1] : 1;
    const double *l1 = d >= 2 ? lam[1] : nullptr, *l2 = d >= 3 ? lam[2] : nullptr;
    if (few) hipLaunchKernelGGL(k_opfun_mix<4>, grid, dim3(256), 0, st, tb, d, n1, nl, G, lam[0], l1, l2, x, y);
    else hipLaunchKernelGGL(k_opfun_mix<OPFUN_MAX_TERMS>, grid, dim3(256), 0, st, tb, d, n1, nl, G, lam[0], l1, l2, x, y);
  } else {
    MixGeo geo = {};
    geo.d = d;
    { long s = 1; for (int k = d - 1; k >= 0; k--) { geo.gs[k] = s; s *= M[k]; geo.lam[k] = lam[k]; } }
    const dim3 grid(grid1d(G, 256, 4096));
    if (few) hipLaunchKernelGGL(k_opfun_mix_nd<4>, grid, dim3(256), 0, st, tb, geo, G, x, y);
    else hipLaunchKernelGGL(k_opfun_mix_nd<OPFUN_MAX_TERMS>, grid, dim3(256), 0, st, tb, geo, G, x, y);
  }
  sweep_note_launch();
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace chebhip

static double weight_host(int kind, double tau, double par, double s) {
  const long double S = s, T = tau, P = par, z = -(T * S);
  switch (kind) {
    case opfun::K_ONE: return 1.0;
    case opfun::K_INV: return s != 0.0 ? (double)(1.0L / S) : 0.0;
    case opfun::K_RES: { const long double den = fmal(T, S, P); return den != 0.0L ? (double)(1.0L / den) : 0.0; }
    case opfun::K_EXP: return (double)expl(z);
    case opfun::K_PHI1: case opfun::K_PHI2: case opfun::K_PHI3: return (double)phi_host(kind - opfun::K_PHI1 + 1, z);
    default: return s == 0.0 ? (par == 0.0 ? 1.0 : 0.0) : s < 0.0 ? (double)NAN : (double)powl(S, P);
  }
}

extern "C" int cheb_opfun_weights_host(int kind, double tau, double par, long n, const double *s, double *w) {
  int rc = opfun_check_weight(kind, tau, par); if (rc) return rc;
  if (n < 0 || (n > 0 && (!s || !w))) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: weights need n >= 0 and two arrays");
  for (long i = 0; i < n; i++) w[i] = weight_host(kind, tau, par, s[i]);
  return 0;
}

extern "C" int cheb_opfun_weight_host(int kind, double tau, double par, double s, double *w) {
  if (!w) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: w is NULL");
  return cheb_opfun_weights_host(kind, tau, par, 1, &s, w);
}

extern "C" int cheb_opfun_check_terms(int nin, int nout, int nterms, const cheb_opfun_term *terms) {
  if (nin < 1 || nin > OPFUN_MAX_FIELDS || nout < 1 || nout > OPFUN_MAX_FIELDS) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: nin = %d, nout = %d must be in 1..16", nin, nout);
  OpfunTable tb;
  return opfun_build_table(nin, nout, nterms, terms, &tb);
}

extern "C" int cheb_opfun_eval(int kind, double tau, double par, const double *s_dev, long n, double *w_dev, void *stream) {
  int rc = opfun_check_weight(kind, tau, par); if (rc) return rc;
  if (n < 0 || (n > 0 && (!s_dev || !w_dev))) return chebhip_fail(CHEBHIP_ERR_ARG, "opfun: eval needs n >= 0 and two arrays");
  if (n == 0) return 0;
  if ((rc = require_device())) return rc;
  hipLaunchKernelGGL(k_opfun_eval, dim3(grid1d(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, kind, tau, par, n, s_dev, w_dev);
  HIP_TRY(hipGetLastError());
  return 0;
}
