// stokes_node.h -- what the Stokes callbacks do at ONE node, once: the rheology (stokes.C:1920-1944) and the node laws of StokesMatMultVV
// (stokes.C:647-662) and StokesFunction (:710-725).  Plain C++ (a host program includes it: tests/host/stokes_node_check.cpp holds these
// functions to long-double truth); every node kernel of stokes.hip calls them per node -- k_st_node_vv / k_st_node_fn, their pair forms and
// stage C of k_st_zfused16 -- so the routes give the same bits by construction.  What stays in a kernel is what differs between them: where
// g, s0 and eta come from, which slots are written, the pressure folded into the diagonal stress, the parity split of tau_z.
//
// The order of operations is part of the contract (the routes and the parent of every change are compared bit for bit):
//   strain[j][k] = 0.5 * (g[j][k] + g[k][j])
//   z = sum strain[j][k] * s0[j][k]  and  gamma = sum 0.5 * (strain[j][k] * strain[j][k]):  j outer, k inner, starting from 0.0
//   tau[j][k] = eta * strain[j][k] + deta * s0[j][k] * z  (DETA; the device contracts products and sums as the compiler's default allows)
//   trace = (g[0][0] + g[1][1]), then += g[2][2] for D = 3
//   DETA = false reads neither s0 nor deta: tau[j][k] = eta * strain[j][k]   (the j, k loops unroll without a pragma: same listings)
#pragma once
#include <cmath>

#ifdef __forceinline__                                                     // HIP's runtime header is in: device code too
#define ST_NODE_FN __host__ __device__ __forceinline__
#else
#define ST_NODE_FN inline
#endif

struct StRheology { int kind; double hardness, expo, eps, gamma0; };      // stokes.C:403; kind 0: linear, 1: power law

// lane q of a two-node value (double2, or anything with .x and .y)
template <class V2> ST_NODE_FN double &st_comp(V2 &v, int q) { return q ? v.y : v.x; }
ST_NODE_FN double st_sym(double a, double b) { return 0.5 * (a + b); }

// eta(gamma) and eta'(gamma), gamma = s : s / 2
ST_NODE_FN void st_rheology(const StRheology &rh, double gamma, double &eta, double &deta) {
  eta = 1.0; deta = 0.0;
  if (rh.kind == 1) {
    const double p = (1.0 - rh.expo) / (2.0 * rh.expo);
    // one pow: q^(p-1) = q^p / q (the second pow was half of the node kernel's time at 128^3; the quotient differs from
    // it by an ulp, far inside the 1e-10 bar)
    const double q = rh.eps + gamma / rh.gamma0, qp = pow(q, p);
    eta = rh.hardness * qp;
    deta = (fabs(rh.expo) > 1.0e-5) ? rh.hardness * p / rh.gamma0 * (qp / q) : 0.0;
  }
}

// Jacobian: tau = eta s + eta' S0 (S0 : s) of the gradient g, and its trace.  s0 is the stored (symmetric) strain.
template <int D, bool DETA>
ST_NODE_FN void st_node_vv(const double (&g)[D][D], const double (&s0)[D][D], double eta, double deta, double (&tau)[D][D], double &trace) {
  double strain[D][D], z = 0.0;
  for (int j = 0; j < D; j++)
    for (int k = 0; k < D; k++) { strain[j][k] = st_sym(g[j][k], g[k][j]); if (DETA) z += strain[j][k] * s0[j][k]; }
  for (int j = 0; j < D; j++)
    for (int k = 0; k < D; k++) tau[j][k] = DETA ? eta * strain[j][k] + deta * s0[j][k] * z : eta * strain[j][k];
  trace = g[0][0] + g[1][1];
  if (D == 3) trace += g[D - 1][D - 1];
}

// Residual: the symmetrised gradient s (the state the Jacobian reads as S0), eta and eta' by the rheology, tau = eta s, the trace.
template <int D>
ST_NODE_FN void st_node_fn(const double (&g)[D][D], const StRheology &rh, double (&s)[D][D], double (&tau)[D][D], double &eta, double &deta, double &trace) {
  double gamma = 0.0;
  for (int j = 0; j < D; j++)
    for (int k = 0; k < D; k++) { s[j][k] = st_sym(g[j][k], g[k][j]); gamma += 0.5 * (s[j][k] * s[j][k]); }
  st_rheology(rh, gamma, eta, deta);
  for (int j = 0; j < D; j++)
    for (int k = 0; k < D; k++) tau[j][k] = eta * s[j][k];
  trace = g[0][0] + g[1][1];
  if (D == 3) trace += g[D - 1][D - 1];
}

// The two laws on a node PAIR (D = 3): every operand holds the values of two nodes, lane q of each goes through the law above.
template <bool DETA, class V2>
ST_NODE_FN void st_node_vv2(const V2 (&g)[3][3], const V2 (&s0)[3][3], V2 eta, V2 deta, V2 (&tau)[3][3], V2 &trace) {
  for (int q = 0; q < 2; q++) {
    double gq[3][3], sq[3][3], tq[3][3];
    for (int j = 0; j < 3; j++)
      for (int k = 0; k < 3; k++) { gq[j][k] = q ? g[j][k].y : g[j][k].x; sq[j][k] = q ? s0[j][k].y : s0[j][k].x; }
    st_node_vv<3, DETA>(gq, sq, st_comp(eta, q), st_comp(deta, q), tq, st_comp(trace, q));
    for (int j = 0; j < 3; j++)
      for (int k = 0; k < 3; k++) st_comp(tau[j][k], q) = tq[j][k];
  }
}
template <class V2>
ST_NODE_FN void st_node_fn2(const V2 (&g)[3][3], const StRheology &rh, V2 (&s)[3][3], V2 (&tau)[3][3], V2 &eta, V2 &deta, V2 &trace) {
  for (int q = 0; q < 2; q++) {
    double gq[3][3], sq[3][3], tq[3][3];
    for (int j = 0; j < 3; j++)
      for (int k = 0; k < 3; k++) gq[j][k] = q ? g[j][k].y : g[j][k].x;
    st_node_fn<3>(gq, rh, sq, tq, st_comp(eta, q), st_comp(deta, q), st_comp(trace, q));
    for (int j = 0; j < 3; j++)
      for (int k = 0; k < 3; k++) { st_comp(tau[j][k], q) = tq[j][k]; st_comp(s[j][k], q) = sq[j][k]; }
  }
}
