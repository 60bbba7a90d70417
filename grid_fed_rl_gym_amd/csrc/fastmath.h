// fastmath.h -- the three elementary functions of the environment prologue, written out.
//
// The load noise of one env step is 43 Box-Muller pairs per instance on the IEEE-123 feeder; with libm's log / sincos
// (general arguments: ~120 / ~250 vector instructions each) that phase was bound by FP64 VALU issue.  The arguments
// here are special -- a uniform in (0, 1], an angle that is a known fraction of a turn, a divisor that is the same
// for every instance -- so range reduction is exact and short:
//   gs_log01(u)            natural logarithm, u in (0, 1] (any positive normal double in fact)
//   gs_sincos_turns(t,..)  sin and cos of 2 pi t, |t| < 2^30: the quadrant comes from 4 t exactly
//   gs_fmod_pos(x, d, rd)  fmod(x, d) for x >= 0, exactly (the remainder of an fma, then one correction step)
//   gs_div_by(x, d, rd)    x / d with rd = RN(1 / d) supplied by the host: correctly rounded (Markstein's
//                          theorem: q = RN(x rd) is faithful, r = x - d q is exact in an fma, RN(q + r rd) = RN(x / d))
//   gs_sqrt_fast(x)        sqrt(x), same bits, 13 vector instructions instead of 21 (gs_sqrt_core: 10, for a known range)
//   gs_div_fast(a, b)      a / b, same bits, for operands that need none of the division's scaling: 8 instead of 11
// Kernels follow fdlibm's k_sin / k_cos / e_log polynomials; max error ~1 ulp (tests/test_fastmath.py compiles this
// header for the host with g++ and compares with libm / true division on 10^6 points: the arithmetic is the same on
// both sides because every multiply-add is an explicit fma).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define GS_HD __host__ __device__ __forceinline__
#else
#define GS_HD static inline
#endif
// No implicit contraction inside these functions: which multiply the compiler would fuse into which add depends on the
// code around the inlined copy, and two kernels that inline the same function must give the same bits (the step
// kernels with and without the fused checks are compared bit for bit).  Every fused multiply-add is written out.
#ifdef __clang__
#define GS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GS_NO_CONTRACT
#endif

// ---- short exact square root and division ----------------------------------------------------------------------------------
// The compiler's correctly rounded sqrt(double) is 21 vector instructions on gfx950 and its a / b is 11: a refinement core (the
// hardware estimate, then fused multiply-adds) inside a frame that scales tiny or huge operands into range and back and patches the
// special values.  Where the operands are known to need no scaling the core alone gives the same bits, because it IS the same
// arithmetic: gs_sqrt_refine and gs_div_fast below are those cores, operation for operation, read off the compiler's assembly.
// tests/test_fastmath_exact.py compares them bit for bit with sqrt and / on the host, with a seed of the hardware's accuracy moved
// about at random: the refinement does not depend on which estimate it starts from.
//
// The seed: v_rsq_f64 / v_rcp_f64 on the device; on the host a stand-in, which a test replaces by defining the macros first.
#if defined(__HIP_DEVICE_COMPILE__)
#define GS_RSQ_SEED(x) __builtin_amdgcn_rsq(x)
#define GS_RCP_SEED(x) __builtin_amdgcn_rcp(x)
#else
#ifndef GS_RSQ_SEED
#define GS_RSQ_SEED(x) (1.0 / sqrt(x))
#endif
#ifndef GS_RCP_SEED
#define GS_RCP_SEED(x) (1.0 / (x))
#endif
#endif

// sqrt(x) from y ~ 1 / sqrt(x): two multiplies and seven fused multiply-adds (Goldschmidt's coupled pair g -> sqrt x, h -> 1 / (2 sqrt x),
// then two residual steps).  Same bits as sqrt for x in [2^-767, +inf): the compiler scales by 2^256 below 2^-767 only.
GS_HD double gs_sqrt_refine(double x, double y) {
  GS_NO_CONTRACT
  double g = x * y, h = y * 0.5;
  const double r = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r, g);
  h = __builtin_fma(h, r, h);
  double d = __builtin_fma(-g, g, x);
  g = __builtin_fma(d, h, g);
  d = __builtin_fma(-g, g, x);
  return __builtin_fma(d, h, g);
}
// The bare core, for an argument known to lie in [2^-767, +inf) -- no zero, no infinity, no NaN: ten vector instructions.
GS_HD double gs_sqrt_core(double x) { return gs_sqrt_refine(x, GS_RSQ_SEED(x)); }

#if defined(__HIP_DEVICE_COMPILE__)
// one copy per kernel of the general square root, out of line: the waves that need it are the exception
static __device__ __attribute__((noinline)) double gs_sqrt_slow(double x) { return sqrt(x); }
#endif
// sqrt(x) for ANY x, bit for bit.  +0 and [2^-767, +inf) take the core (13 vector instructions with the test); a wave (on the host:
// an element) with anything else -- a subnormal or tiny value, +inf, NaN, a negative number, -0 -- takes the general sqrt.
//   The test is two compares: (x >= 2^-767) holds for the core's range and for +inf, the class test for +0 and +inf; exactly one of
// the two holds on +0 and on the core's range, both on +inf, neither on the rest.
//   +0 stays on the short path because it is ordinary here (a line that carries nothing has S = 0 exactly): the estimate of +0 is
// +inf, and with its high word held at 2^512's the core yields g = 0 * y = +0, residuals +0, result +0.  Inside the core's range
// the estimate is below 2^384 and the minimum changes nothing (an integer minimum on the high word: y is not negative here).
GS_HD double gs_sqrt_fast(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const bool core = (x >= 0x1p-767) != __builtin_amdgcn_class(x, 0x240);        // class bits: 0x040 +0, 0x200 +inf
  if (__builtin_amdgcn_ballot_w64(!core) != 0) return gs_sqrt_slow(x);           // wave-uniform: no lane diverges
#else
  uint64_t xb;
  __builtin_memcpy(&xb, &x, 8);
  const bool core = (x >= 0x1p-767) != (xb == 0 || xb == 0x7ff0000000000000ull);
  if (!core) return sqrt(x);
#endif
  double y = GS_RSQ_SEED(x);
  uint64_t yb;
  __builtin_memcpy(&yb, &y, 8);
  const uint32_t hi = (uint32_t)(yb >> 32);
  yb = ((uint64_t)(hi < 0x5ff00000u ? hi : 0x5ff00000u) << 32) | (uint32_t)yb;
  __builtin_memcpy(&y, &yb, 8);
  return gs_sqrt_refine(x, y);
}

// a / b, correctly rounded, for a normal b and a quotient that is normal (or a = +0): the reciprocal estimate, two Newton steps,
// the quotient, its exact remainder and one correction -- eight vector instructions, the arithmetic of the compiler's a / b without
// its scaling of operands near the ends of the exponent range and without its patching of special values.  Not for: b = 0, inf or
// NaN; a quotient that overflows or is subnormal; a = -0, which comes out as +0 (the remainder -b q + a of a zero quotient is +0).
GS_HD double gs_div_fast(double a, double b) {
  GS_NO_CONTRACT
  double y = GS_RCP_SEED(b);
  double e = __builtin_fma(-b, y, 1.0);
  y = __builtin_fma(y, e, y);
  e = __builtin_fma(-b, y, 1.0);
  y = __builtin_fma(y, e, y);
  const double q = a * y;
  const double r = __builtin_fma(-b, q, a);
  return __builtin_fma(r, y, q);
}

// (SHORT = false: the division as the compiler expands it -- the same bits; for a kernel that comes out worse through the short one)
template <bool SHORT = true>
GS_HD double gs_log01(double x) {
  GS_NO_CONTRACT
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
               Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
               Lg7 = 1.479819860511658591e-01;
  int k;
  double m = __builtin_frexp(x, &k);                 // x = m 2^k, m in [0.5, 1)
  if (m < 0.70710678118654752440) { m *= 2.0; k -= 1; }       // m in [sqrt(1/2), sqrt(2))
  const double f = m - 1.0;
  // f is in [-0.30, 0.42] and is +0 exactly (m = 1) or at least 2^-53 in magnitude, the divisor is in [1.70, 2.42]: the quotient is
  // +0 or normal, never -0 and never subnormal, and the short division gives the bits of f / (2 + f)
  const double s = SHORT ? gs_div_fast(f, 2.0 + f) : f / (2.0 + f);
  const double z = s * s;
  double R = Lg7;
  R = __builtin_fma(R, z, Lg6); R = __builtin_fma(R, z, Lg5); R = __builtin_fma(R, z, Lg4);
  R = __builtin_fma(R, z, Lg3); R = __builtin_fma(R, z, Lg2); R = __builtin_fma(R, z, Lg1);
  R *= z;
  const double hfsq = 0.5 * f * f;
  const double dk = (double)k;
  // log(1 + f) = f - hfsq + s (hfsq + R);  log x = k ln2 + log(1 + f)
  return __builtin_fma(dk, ln2_hi, f - (hfsq - __builtin_fma(s, hfsq + R, dk * ln2_lo)));
}

GS_HD void gs_sincos_turns(double t, double* sn, double* cs) {
  GS_NO_CONTRACT
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
               S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
               C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double q4 = 4.0 * t;                          // exact
  const double n = __builtin_rint(q4);
  const double x = (q4 - n) * 1.57079632679489661923;  // (q4 - n) exact, in [-1/2, 1/2]; x in [-pi/4, pi/4]
  const double z = x * x;
  double ps = S6;
  ps = __builtin_fma(ps, z, S5); ps = __builtin_fma(ps, z, S4); ps = __builtin_fma(ps, z, S3);
  ps = __builtin_fma(ps, z, S2); ps = __builtin_fma(ps, z, S1);
  const double s = __builtin_fma(x * z, ps, x);
  double pc = C6;
  pc = __builtin_fma(pc, z, C5); pc = __builtin_fma(pc, z, C4); pc = __builtin_fma(pc, z, C3);
  pc = __builtin_fma(pc, z, C2); pc = __builtin_fma(pc, z, C1);
  const double c = __builtin_fma(z * z, pc, __builtin_fma(-0.5, z, 1.0));
  const int q = (int)n & 3;                           // two's complement: right for negative n as well
  const double a = (q & 1) ? c : s, b = (q & 1) ? s : c;
  *sn = (q & 2) ? -a : a;
  *cs = ((q + 1) & 2) ? -b : b;
}

// x / d for a divisor d shared by many numerators, rd = RN(1 / d) (computed once, by a true division).
GS_HD double gs_div_by(double x, double d, double rd) {
  GS_NO_CONTRACT
  const double q = x * rd;
  const double r = __builtin_fma(-d, q, x);
  const double q1 = __builtin_fma(r, rd, q);
  return (__builtin_fabs(q) < __builtin_inf()) ? q1 : q;      // an infinite or NaN quotient stays what it is
}

// fmod(x, d) for x >= 0, d > 0, rd = RN(1 / d), x / d < 2^52: q is the true quotient's floor or one off, x - d q is
// exact in the fma (it is a multiple of ulp(x) below 2 d), and one conditional step brings it into [0, d).
GS_HD double gs_fmod_pos(double x, double d, double rd) {
  GS_NO_CONTRACT
  const double q = __builtin_floor(x * rd);
  double r = __builtin_fma(-d, q, x);
  if (r < 0.0) r += d;
  else if (r >= d) r -= d;
  return r;
}
