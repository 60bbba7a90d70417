// Host harness for the short exact square root and division of grid_fed_rl_gym_amd/csrc/fastmath.h (tests/test_fastmath_exact.py
// builds it with g++ -ffp-contract=off).  The hardware estimates are replaced by the true 1 / sqrt(x) and 1 / b cut to 26 significant
// bits and then moved by -1, 0 or +1 unit of that last place, drawn from a seeded generator: the refinement has to give the correctly
// rounded result from ANY estimate of that accuracy, not from a lucky one.
#include <math.h>
#include <stdint.h>
#include <string.h>

static uint64_t fx_state = 1;
static inline double fx_estimate(double t) {
  if (!(fabs(t) < INFINITY) || t == 0.0) return t;               // 1 / sqrt(0) = inf, 1 / sqrt(inf) = 0, NaN: as the hardware gives them
  uint64_t b;
  memcpy(&b, &t, 8);
  b &= ~((1ull << 27) - 1);                                      // the leading bit and 25 more
  fx_state = fx_state * 6364136223846793005ull + 1442695040888963407ull;
  b += (uint64_t)(((int64_t)((fx_state >> 33) % 3) - 1) * (int64_t)(1ull << 27));
  memcpy(&t, &b, 8);
  return t;
}
#define GS_RSQ_SEED(x) fx_estimate(1.0 / sqrt(x))
#define GS_RCP_SEED(x) fx_estimate(1.0 / (x))
#include "fastmath.h"

extern "C" {
void fx_seed(uint64_t s) { fx_state = s * 2 + 1; }
void fx_sqrt_fast(const double* x, double* out, long n) { for (long i = 0; i < n; ++i) out[i] = gs_sqrt_fast(x[i]); }
void fx_sqrt_core(const double* x, double* out, long n) { for (long i = 0; i < n; ++i) out[i] = gs_sqrt_core(x[i]); }
void fx_div_fast(const double* a, const double* b, double* out, long n) { for (long i = 0; i < n; ++i) out[i] = gs_div_fast(a[i], b[i]); }
void fx_log01(const double* x, double* out, long n) { for (long i = 0; i < n; ++i) out[i] = gs_log01(x[i]); }
// the uniform of a 32-bit word both ways: (r + 1/2) 2^-32 as an add and a multiply, and as the one fused multiply-add of env_device.h
void fx_unit32(const uint32_t* r, double* two_ops, double* one_fma, long n) {
  for (long i = 0; i < n; ++i) {
    two_ops[i] = ((double)r[i] + 0.5) * (1.0 / 4294967296.0);
    one_fma[i] = __builtin_fma((double)r[i], 1.0 / 4294967296.0, 0.5 / 4294967296.0);
  }
}
}
