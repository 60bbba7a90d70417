// gw_math.h -- exp, tanh and log of the sampling heads, from rounded float64 +, -, *, / alone (include/gridstep.h "the pathwise actor
// step" states them; learner.py's pathwise_exp_np / _tanh_np / _log_np perform the same operations one by one, so the heads are
// restated to the bit whatever library the host has).  Nothing is contracted; frexp, ldexp and rint are exact.
// ONE copy (DESIGN.md section 24's rule) for the two files whose heads sample a tanh-Gaussian action: kernels_pathwise.hip
// (gs_k_pw_sample, gs_k_pw_head) and kernels_q_next.hip (gs_k_policy_rows_f32).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace {

constexpr double GW_LN2_HI = 6.93147180369123816490e-01, GW_LN2_LO = 1.90821492927058770002e-10, GW_INV_LN2 = 1.4426950408889634;
__device__ const double gw_inv_fact[24] = {1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889, 0.0001984126984126984, 2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08, 2.08767569878681e-09, 1.6059043836821613e-10, 1.1470745597729725e-11, 7.647163731819816e-13, 4.779477332387385e-14, 2.8114572543455206e-15, 1.5619206968586225e-16, 8.22063524662433e-18, 4.110317623312165e-19, 1.9572941063391263e-20, 8.896791392450574e-22, 3.8681701706306835e-23};      // 1 / j!
__device__ const double gw_inv_odd[15] = {0.3333333333333333, 0.2, 0.14285714285714285, 0.1111111111111111, 0.09090909090909091, 0.07692307692307693, 0.06666666666666667, 0.058823529411764705, 0.05263157894736842, 0.047619047619047616, 0.043478260869565216, 0.04, 0.037037037037037035, 0.034482758620689655, 0.03225806451612903};        // 1 / (2 j + 1), j = 1 .. 15

// exp(x): k = rint(x / ln 2), r = x - k ln 2 in two parts (|r| <= 0.347), the Taylor sum to r^17 by Horner's rule, times 2^k
__device__ __forceinline__ double gw_exp(double x) {
#pragma clang fp contract(off)
  const double k = rint(x * GW_INV_LN2);
  const double r = (x - k * GW_LN2_HI) - k * GW_LN2_LO;
  double p = gw_inv_fact[17];
  for (int j = 16; j >= 0; --j) p = gw_inv_fact[j] + r * p;
  return ldexp(p, (int)k);
}

// tanh(x), u = min(|x|, 40): below 0.5 from m = expm1(2 u) (the Taylor sum to (2 u)^23) as m / (m + 2), else from e = exp(-2 u)
// as (1 - e) / (1 + e); the sign of x
__device__ __forceinline__ double gw_tanh(double x) {
#pragma clang fp contract(off)
  const double u = fmin(fabs(x), 40.0);
  double t;
  if (u < 0.5) {
    const double y = 2.0 * u;
    double p = gw_inv_fact[23];
    for (int j = 22; j >= 1; --j) p = gw_inv_fact[j] + y * p;
    const double m = y * p;
    t = m / (m + 2.0);
  } else {
    const double e = gw_exp(-2.0 * u);
    t = (1.0 - e) / (1.0 + e);
  }
  return copysign(t, x);
}

// log(v), v > 0 and normal: v = m 2^e with sqrt(1/2) <= m < sqrt(2), s = (m - 1) / (m + 1), log m = 2 s (1 + z P(z)), z = s s,
// P the sum of z^(j - 1) / (2 j + 1), j = 1 .. 15, by Horner's rule; plus e ln 2 in two parts
__device__ __forceinline__ double gw_log(double v) {
#pragma clang fp contract(off)
  int e;
  double m = frexp(v, &e);
  if (m < 0.7071067811865476) { m = m * 2.0; e -= 1; }
  const double f = m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s;
  double p = gw_inv_odd[14];
  for (int j = 13; j >= 0; --j) p = gw_inv_odd[j] + z * p;
  const double t2 = 2.0 * s;
  const double logm = t2 + t2 * (z * p);
  const double ed = (double)e;
  return ed * GW_LN2_HI + (ed * GW_LN2_LO + logm);
}

// gs_logp_term of policy_head.h with this file's log
__device__ __forceinline__ double gw_logp_term(double eps, double ls, double act) {
#pragma clang fp contract(off)
  return (((-0.5 * eps) * eps - ls) - 0.91893853320467274178) - gw_log((1.0 - act * act) + 1e-6);
}

}  // namespace
