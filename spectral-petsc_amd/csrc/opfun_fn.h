// opfun_fn.h -- the weight functions f(s) of ChebOpFun (cheb_opfun_*), one function per kind.  Included by the mixing
// kernel and by cheb_opfun_eval (opfun.hip), which runs exactly these functions over an array of s.
//
// Error counts in units of U = 2^-53 (relative; HIP documents exp, expm1 and pow as 1 ulp = 2 U); tests/opfun_ref.py holds the
// device to them.  z = -tau s is rounded once (1 U in z); a function g carries that on as |z g'(z) / g(z)| U.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace chebhip {
namespace opfun {

enum Kind { K_ONE = 0, K_INV = 1, K_RES = 2, K_EXP = 3, K_PHI1 = 4, K_PHI2 = 5, K_PHI3 = 6, K_POW = 7, NKINDS = 8 };

// |z| <= PHI_SERIES: phi_2, phi_3 by their series; beyond it by the recurrence phi_{k+1} = (phi_k - 1/k!) / z.
// The recurrence amplifies the error of phi_k by phi_k / |phi_k - 1/k!|: 0.76 (phi_1 -> phi_2) and 1.31 (phi_2 -> phi_3) at
// z = -2, growing without bound as z -> 0 (2.8 already at z = -1) and falling towards 0 as z -> -inf.  The nested series has no
// cancelling level for |z| <= 2 (each level 1 + z / (k + j) (..) stays in [1/3, 5/3]) and needs 24 levels there.
constexpr double PHI_SERIES = 2.0;
constexpr int PHI_LEVELS = 24;

// sum_j z^j k! / (j + k)! = 1 + z/(k+1) (1 + z/(k+2) (1 + ...)), |z| <= 2: the tail after 24 levels is below 2^-58 of the sum
template <int K>
__host__ __device__ __forceinline__ double phi_nested(double z) {
  double r = 1.0;
#pragma unroll
  for (int j = PHI_LEVELS; j >= 1; j--) r = fma(z * (1.0 / (double)(K + j)), r, 1.0);
  return r;
}

__host__ __device__ __forceinline__ double w_one(double) { return 1.0; }
// 1 U (the division); the caller multiplies once: the bits of the solver's W array
__host__ __device__ __forceinline__ double w_inv(double s) { return s != 0.0 ? 1.0 / s : 0.0; }
// 2 U: p + tau s in one rounding (fma: also where the two cancel), the division
__host__ __device__ __forceinline__ double w_res(double tau, double p, double s) {
  const double den = fma(tau, s, p);
  return den != 0.0 ? 1.0 / den : 0.0;
}
// (2 + tau s) U: exp 2 U, and the rounding of z moves the exponent by tau s U
__host__ __device__ __forceinline__ double w_exp(double tau, double s) { return exp(-(tau * s)); }
// 4 U: z 1 U (|z phi_1' / phi_1| < 1 for z < 0), expm1 2 U, the division 1 U
__host__ __device__ __forceinline__ double w_phi1(double tau, double s) {
  const double z = -(tau * s);
  return z != 0.0 ? expm1(z) / z : 1.0;
}
// series: level j has 3 roundings (1 / (k + j) as a constant, its product with z, the fma) and passes the error of level j + 1 on
// times |a_j r_{j+1}| / r_j <= 0.76 (z = -2, k = 2; smaller for every other level, |z| and k): e_0 <= 1 + 0.76 (2 + e_1) <= 5.3 U
// for phi_2, 4.4 U for phi_3; the scaling by 1/k! is exact for k = 2 and 1.5 U for k = 3; z itself 1 U: 6.3 U and 6.9 U.
// recurrence (|z| > 2): phi_1 3 U (z apart); phi_1 - 1: 3 * 0.76 + 1 U; / z: 1 U; z: 1 U -> phi_2 <= 5.3 U;
//                       phi_2 - 1/2: 4.3 * 1.31 + 1 U; / z: 1 U; z: 1 U -> phi_3 <= 8.7 U.
__host__ __device__ __forceinline__ double w_phi2(double tau, double s) {
  const double z = -(tau * s);
  if (fabs(z) <= PHI_SERIES) return 0.5 * phi_nested<2>(z);
  return (expm1(z) / z - 1.0) / z;
}
__host__ __device__ __forceinline__ double w_phi3(double tau, double s) {
  const double z = -(tau * s);
  if (fabs(z) <= PHI_SERIES) return (1.0 / 6.0) * phi_nested<3>(z);
  return ((expm1(z) / z - 1.0) / z - 0.5) / z;
}
// 2 U (pow); s < 0 has no real power: NaN, whatever p
__host__ __device__ __forceinline__ double w_pow(double p, double s) {
  if (s == 0.0) return p == 0.0 ? 1.0 : 0.0;
  if (s < 0.0) return __builtin_nan("");
  return pow(s, p);
}

__host__ __device__ __forceinline__ double weight(int kind, double tau, double par, double s) {
  switch (kind) {
    case K_ONE: return w_one(s);
    case K_INV: return w_inv(s);
    case K_RES: return w_res(tau, par, s);
    case K_EXP: return w_exp(tau, s);
    case K_PHI1: return w_phi1(tau, s);
    case K_PHI2: return w_phi2(tau, s);
    case K_PHI3: return w_phi3(tau, s);
    default: return w_pow(par, s);
  }
}

}  // namespace opfun
}  // namespace chebhip
