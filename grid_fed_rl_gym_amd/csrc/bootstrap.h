// bootstrap.h -- the arithmetic of a bootstrap target, from rounded float64 +, -, * alone (include/gridstep.h states each formula;
// rollout.py's td_target_np / td_policy_np / q_combine_np / refresh_rows_np restate them one operation at a time).  ONE copy (DESIGN.md
// section 24's rule; section 28 lists the users) for every kernel that forms a target over the whole rollout or over the rows of a
// minibatch, which is what makes gs_learner_refresh's rows bit-equal to a full evaluation.  `fp contract(off)` is lexical: a helper
// that multiplies and adds carries the pragma in its own body, whatever its caller has.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "refresh.h"

namespace {

// batch row -> transition: the index clamped into [0, N), so that one the minibatch did not write cannot leave the rollout (the
// rule itself is refresh.h's GS_RF_CLAMP, which the host program of the refresh's checks can run)
__device__ __forceinline__ long long gb_row(long long j, long long N) { return GS_RF_CLAMP(j, N); }

// the minimum over the installed twins at element i; a twin that is not installed is NULL, and one of the two is there
__device__ __forceinline__ double gb_twin_min(const double* a, const double* b, size_t i) {
  return a && b ? fmin(a[i], b[i]) : a ? a[i] : b[i];
}

// the entropy-adjusted value m - alpha * lp: a rounded product, then a rounded difference
__device__ __forceinline__ double gb_soft_value(double m, double alpha, double lp) {
#pragma clang fp contract(off)
  return m - alpha * lp;
}

// the Bellman target r' + gamma * vnext, r' = (rew - shift) * scale: a rounded product, then a rounded product and a rounded sum
__device__ __forceinline__ double gb_td(double rew, double shift, double scale, double gamma, double vnext) {
#pragma clang fp contract(off)
  const double r = (rew - shift) * scale;
  return r + gamma * vnext;
}

}  // namespace
