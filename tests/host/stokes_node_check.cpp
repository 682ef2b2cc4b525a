// Host-side check of the Stokes node laws (csrc/stokes_node.h: st_rheology, st_node_vv, st_node_fn and their pair forms) against the same
// formulas in long double, with the bars of tests/callbacks_ref.py's docstring at a node (the gradient is exact input here, so its own
// error term is zero); u = 2^-53, d = dimensions:
//   Jacobian stress    |tau - truth| <= (d^2 + 4) u W,  W = |eta| |s_jk| + |eta'| |S0_jk| sum |S0| |s|
//   residual stress    the same bar with S0 = s (the operator linearised about the state the call leaves), for both rheologies: the
//                      eta' part of the weight covers what the error of eta contributes
//   strain             1 u (|g_jk| + |g_kj|) / 2
//   trace              d u sum |g_jj|
//   eta, eta'          relative: dq = (d^2 + 1) gamma / gamma0 + 2 q;  |p| dq / q + 1 + POW  and  (|p| + 1) dq / q + 4 + POW
//   a weight of 0 demands an exact 0
// POW is measured here, not taken from the device's figure (another library): the worst error of pow against powl on the q values of
// these cases, in ulps; the allowance is twice that, rounded up -- the rule by which callbacks_ref.POW_ULPS was set.
// Exact: DETA = false gives the bits of DETA = true with eta' = 0 and a finite S0; D = 3 on a gradient whose third row and column are
// zero gives the bits of D = 2 in the 2 x 2 block; the pair forms give the bits of the scalar ones.
// Prints one line per case ("case <name> d <d> nodes <n> worst <ratio of its bar> ..."), "pow_ulps <worst> allowance <int>", then "ok" or
// "FAILED <count>".  Built and run by tests/test_host_stokes_node.py; needs no GPU.
#include "stokes_node.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

typedef long double LD;
static const LD U = ldexpl(1.0L, -53);
static int g_failed = 0;

struct Rng {                                                    // xorshift64*; normal(): Box-Muller
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
  uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
  double uniform() { return ((next() >> 11) + 0.5) * (1.0 / 9007199254740992.0); }
  double normal() { return sqrt(-2.0 * log(uniform())) * cos(6.283185307179586 * uniform()); }
  int integer(int lo, int hi) { return lo + (int)(next() % (uint64_t)(hi - lo + 1)); }
};
struct V2 { double x, y; };                                     // the two-node value of the pair forms

// |y - t| as a fraction of cap u W; W = 0 demands y == 0 exactly (returns a ratio above 1 otherwise)
static double ratio(double y, LD t, LD W, double cap) {
  const LD err = fabsl((LD)y - t);
  if (W == 0.0L) return y == 0.0 ? 0.0 : 2.0;
  return (double)(err / (cap * U * W));
}
static bool same_bits(const void *a, const void *b, size_t n) { return memcmp(a, b, n) == 0; }

// long-double truths
template <int D>
static void truth_strain(const double (&g)[D][D], LD (&s)[D][D]) {
  for (int j = 0; j < D; j++) for (int k = 0; k < D; k++) s[j][k] = 0.5L * ((LD)g[j][k] + (LD)g[k][j]);
}
static void truth_rheology(const StRheology &rh, LD gamma, LD &eta, LD &deta, LD &q, LD &p) {
  eta = 1.0L; deta = 0.0L; q = 1.0L; p = 0.0L;
  if (rh.kind == 1) {
    p = (1.0L - (LD)rh.expo) / (2.0L * (LD)rh.expo);
    q = (LD)rh.eps + gamma / (LD)rh.gamma0;
    eta = (LD)rh.hardness * powl(q, p);
    deta = (LD)rh.hardness * p / (LD)rh.gamma0 * powl(q, p - 1.0L);
  }
}

// the q = eps + gamma / gamma0 values of the power-law cases: worst error of the host's pow against powl, in ulps of the result
static double g_pow_worst = 0.0;
static void measure_pow(double q, double p) {
  const LD t = powl((LD)q, (LD)p);
  const LD ulp = ldexpl(1.0L, ilogbl(t) - 52);
  const double e = (double)(fabsl((LD)pow(q, p) - t) / ulp);
  if (e > g_pow_worst) g_pow_worst = e;
}

template <int D>
static void gradient(Rng &r, bool scaled, double (&g)[D][D]) {  // scaled: noise x 10^k per node, k in -30 .. 30 (callbacks_ref.node_scaled)
  const double sc = scaled ? pow(10.0, r.integer(-30, 30)) : 1.0;
  for (int j = 0; j < D; j++) for (int k = 0; k < D; k++) g[j][k] = r.normal() * sc;
}

// ---- the Jacobian law: DETA on and off, gradients over 10^+-30, eta in 0.5 .. 10, eta' and the symmetric S0 of order 1
template <int D>
static void check_vv(int nodes, uint64_t seed) {
  Rng r(seed);
  double worst_tau[2] = {0, 0}, worst_tr = 0;
  int exact_bad = 0;
  for (int n = 0; n < nodes; n++) {
    double g[D][D], s0[D][D], tau[D][D], tau0[D][D], tauz[D][D], tr, tr0, trz;
    gradient(r, true, g);
    for (int j = 0; j < D; j++) for (int k = j; k < D; k++) { s0[j][k] = r.normal(); s0[k][j] = s0[j][k]; }
    const double eta = exp(log(0.5) + r.uniform() * (log(10.0) - log(0.5))), deta = r.normal();
    st_node_vv<D, true>(g, s0, eta, deta, tau, tr);
    st_node_vv<D, false>(g, s0, eta, deta, tau0, tr0);
    st_node_vv<D, true>(g, s0, eta, 0.0, tauz, trz);
    if (!same_bits(tau0, tauz, sizeof tau0) || !same_bits(&tr0, &trz, sizeof tr0) || !same_bits(&tr0, &tr, sizeof tr)) exact_bad++;
    LD s[D][D], z = 0, wz = 0, ttr = 0, wtr = 0;
    truth_strain(g, s);
    for (int j = 0; j < D; j++) for (int k = 0; k < D; k++) { z += s[j][k] * (LD)s0[j][k]; wz += fabsl(s[j][k]) * fabsl((LD)s0[j][k]); }
    for (int j = 0; j < D; j++) { ttr += (LD)g[j][j]; wtr += fabsl((LD)g[j][j]); }
    for (int j = 0; j < D; j++)
      for (int k = 0; k < D; k++) {
        const LD w0 = fabsl((LD)eta) * fabsl(s[j][k]), w1 = fabsl((LD)deta) * fabsl((LD)s0[j][k]) * wz;
        worst_tau[1] = fmax(worst_tau[1], ratio(tau[j][k], (LD)eta * s[j][k] + (LD)deta * (LD)s0[j][k] * z, w0 + w1, D * D + 4));
        worst_tau[0] = fmax(worst_tau[0], ratio(tau0[j][k], (LD)eta * s[j][k], w0, D * D + 4));
      }
    worst_tr = fmax(worst_tr, ratio(tr, ttr, wtr, D));
  }
  const bool ok = worst_tau[0] <= 1 && worst_tau[1] <= 1 && worst_tr <= 1 && exact_bad == 0;
  if (!ok) g_failed++;
  printf("case vv d %d nodes %d worst tau_deta_off %.3f tau_deta_on %.3f trace %.3f deta_off_bits_differ %d %s\n", D, nodes, worst_tau[0],
         worst_tau[1], worst_tr, exact_bad, ok ? "pass" : "FAIL");
}

// ---- the residual law: the linear rheology on gradients over 10^+-30, the power law on gradients of order 1
template <int D>
static void check_fn(const char *name, const StRheology &rh, int nodes, uint64_t seed, int pow_allow, bool measure) {
  Rng r(seed);
  const bool power = rh.kind == 1;
  double worst_s = 0, worst_tau = 0, worst_tr = 0, worst_eta = 0, worst_deta = 0;
  const double cap_tau = D * D + 4;
  for (int n = 0; n < nodes; n++) {
    double g[D][D], sd[D][D], tau[D][D], eta, deta, tr;
    gradient(r, !power, g);
    st_node_fn<D>(g, rh, sd, tau, eta, deta, tr);
    LD s[D][D], gamma = 0, ss = 0, teta, tdeta, q, p, ttr = 0, wtr = 0;
    truth_strain(g, s);
    for (int j = 0; j < D; j++) for (int k = 0; k < D; k++) { gamma += 0.5L * (s[j][k] * s[j][k]); ss += fabsl(s[j][k]) * fabsl(s[j][k]); }
    truth_rheology(rh, gamma, teta, tdeta, q, p);
    if (power && measure) measure_pow((double)q, (double)p);
    for (int j = 0; j < D; j++) { ttr += (LD)g[j][j]; wtr += fabsl((LD)g[j][j]); }
    for (int j = 0; j < D; j++)
      for (int k = 0; k < D; k++) {
        worst_s = fmax(worst_s, ratio(sd[j][k], s[j][k], 0.5L * (fabsl((LD)g[j][k]) + fabsl((LD)g[k][j])), 1));
        worst_tau = fmax(worst_tau, ratio(tau[j][k], teta * s[j][k], fabsl(teta) * fabsl(s[j][k]) + fabsl(tdeta) * fabsl(s[j][k]) * ss, cap_tau));
      }
    worst_tr = fmax(worst_tr, ratio(tr, ttr, wtr, D));
    if (power) {
      const LD dq = (D * D + 1) * gamma / (LD)rh.gamma0 + 2 * q;
      worst_eta = fmax(worst_eta, ratio(eta, teta, fabsl(teta), (double)(fabsl(p) * dq / q + 1 + pow_allow)));
      worst_deta = fmax(worst_deta, ratio(deta, tdeta, fabsl(tdeta), (double)((fabsl(p) + 1) * dq / q + 4 + pow_allow)));
    } else if (eta != 1.0 || deta != 0.0) worst_eta = 2.0;       // the linear law: eta = 1, eta' = 0 exactly
  }
  if (measure) return;
  const bool ok = worst_s <= 1 && worst_tau <= 1 && worst_tr <= 1 && worst_eta <= 1 && worst_deta <= 1;
  if (!ok) g_failed++;
  printf("case fn_%s d %d nodes %d worst strain %.3f tau %.3f trace %.3f eta %.3f deta %.3f %s\n", name, D, nodes, worst_s, worst_tau, worst_tr,
         worst_eta, worst_deta, ok ? "pass" : "FAIL");
}

// ---- D = 3 on a gradient whose third row and column are zero: the bits of D = 2 in the 2 x 2 block
static void check_embedding(const StRheology &lin, const StRheology &pw, int nodes, uint64_t seed) {
  Rng r(seed);
  int bad = 0;
  for (int n = 0; n < nodes; n++) {
    double g2[2][2], g3[3][3] = {}, a2[2][2], a3[3][3] = {}, t2[2][2], t3[3][3], s2[2][2], s3[3][3], e2, e3, d2, d3, r2, r3;
    gradient(r, false, g2);
    for (int j = 0; j < 2; j++) for (int k = j; k < 2; k++) { a2[j][k] = r.normal(); a2[k][j] = a2[j][k]; }
    for (int j = 0; j < 2; j++) for (int k = 0; k < 2; k++) { g3[j][k] = g2[j][k]; a3[j][k] = a2[j][k]; }
    for (int j = 0; j < 3; j++) { a3[j][2] = r.normal(); a3[2][j] = a3[j][2]; }          // a finite S0 in the third row and column
    const double eta = 0.5 + 9.5 * r.uniform(), deta = r.normal();
    st_node_vv<2, true>(g2, a2, eta, deta, t2, r2); st_node_vv<3, true>(g3, a3, eta, deta, t3, r3);
    for (int j = 0; j < 2; j++) for (int k = 0; k < 2; k++) bad += !same_bits(&t2[j][k], &t3[j][k], sizeof(double));
    bad += !same_bits(&r2, &r3, sizeof r2);
    for (const StRheology *rh : {&lin, &pw}) {
      st_node_fn<2>(g2, *rh, s2, t2, e2, d2, r2); st_node_fn<3>(g3, *rh, s3, t3, e3, d3, r3);
      for (int j = 0; j < 2; j++) for (int k = 0; k < 2; k++) bad += !same_bits(&t2[j][k], &t3[j][k], sizeof(double)) + !same_bits(&s2[j][k], &s3[j][k], sizeof(double));
      bad += !same_bits(&e2, &e3, sizeof e2) + !same_bits(&d2, &d3, sizeof d2) + !same_bits(&r2, &r3, sizeof r2);
    }
  }
  if (bad) g_failed++;
  printf("case embedding d 3 nodes %d values_that_differ %d %s\n", nodes, bad, bad ? "FAIL" : "pass");
}

// ---- the pair forms: lane q of every result is the scalar law on lane q of every operand, bit for bit
static void check_pairs(const StRheology &pw, int nodes, uint64_t seed) {
  Rng r(seed);
  int bad = 0;
  for (int n = 0; n < nodes; n++) {
    double g[2][3][3], a[2][3][3], t[2][3][3], s[2][3][3], eta[2], deta[2], tr[2], e[2], de[2];
    V2 G[3][3], A[3][3], T[3][3], S[3][3], E, DE, TR;
    for (int q = 0; q < 2; q++) {
      gradient(r, false, g[q]);
      for (int j = 0; j < 3; j++) for (int k = j; k < 3; k++) { a[q][j][k] = r.normal(); a[q][k][j] = a[q][j][k]; }
      eta[q] = 0.5 + 9.5 * r.uniform(); deta[q] = r.normal();
    }
    for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) { G[j][k] = V2{g[0][j][k], g[1][j][k]}; A[j][k] = V2{a[0][j][k], a[1][j][k]}; }
    st_node_vv2<true>(G, A, V2{eta[0], eta[1]}, V2{deta[0], deta[1]}, T, TR);
    for (int q = 0; q < 2; q++) {
      st_node_vv<3, true>(g[q], a[q], eta[q], deta[q], t[q], tr[q]);
      for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) bad += !same_bits(&t[q][j][k], &st_comp(T[j][k], q), sizeof(double));
      bad += !same_bits(&tr[q], &st_comp(TR, q), sizeof(double));
    }
    st_node_fn2(G, pw, S, T, E, DE, TR);
    for (int q = 0; q < 2; q++) {
      st_node_fn<3>(g[q], pw, s[q], t[q], e[q], de[q], tr[q]);
      for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) bad += !same_bits(&t[q][j][k], &st_comp(T[j][k], q), sizeof(double)) + !same_bits(&s[q][j][k], &st_comp(S[j][k], q), sizeof(double));
      bad += !same_bits(&e[q], &st_comp(E, q), sizeof(double)) + !same_bits(&de[q], &st_comp(DE, q), sizeof(double)) + !same_bits(&tr[q], &st_comp(TR, q), sizeof(double));
    }
  }
  if (bad) g_failed++;
  printf("case pairs d 3 nodes %d values_that_differ %d %s\n", nodes, bad, bad ? "FAIL" : "pass");
}

int main() {
  const StRheology LINEAR = {0, 1.0, 1.0, 1.0, 1.0}, POWER = {1, 1.0, 3.0, 1e-2, 1.0};     // the sets of tests/test_gpu_callbacks.py
  const int nodes = 400;
  // first the measurement of pow on the q values the power-law cases will see (same seeds), then the cases with its allowance
  check_fn<2>("power", POWER, nodes, 21, 0, true);
  check_fn<3>("power", POWER, nodes, 31, 0, true);
  const int pow_allow = (int)ceil(2.0 * g_pow_worst);
  check_vv<2>(nodes, 2); check_vv<3>(nodes, 3);
  check_fn<2>("linear", LINEAR, nodes, 20, pow_allow, false); check_fn<3>("linear", LINEAR, nodes, 30, pow_allow, false);
  check_fn<2>("power", POWER, nodes, 21, pow_allow, false); check_fn<3>("power", POWER, nodes, 31, pow_allow, false);
  check_embedding(LINEAR, POWER, nodes, 4);
  check_pairs(POWER, nodes, 5);
  printf("pow_ulps %.17g allowance %d\n", g_pow_worst, pow_allow);
  if (g_failed) printf("FAILED %d\n", g_failed); else printf("ok\n");
  return g_failed ? 1 : 0;
}
