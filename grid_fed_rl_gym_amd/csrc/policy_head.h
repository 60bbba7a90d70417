// policy_head.h -- the log-probability of a sampled action, shared by the heads of gs_k_policy_mlp and gs_k_policy_mlp_f32
// (include/gridstep.h, "on-policy rollouts"): the reference's Normal(mean, std).log_prob(x) - log(1 - tanh(x)^2 + 1e-6)
// (algorithms/offline.py:114-136) with (x - mean)^2 / (2 std^2) written as eps^2 / 2, x = mean + std eps being how x was made.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// one action's term: eps the 'PNOI' draw, ls the clamped log_std, act the action written.  No contraction: the NumPy restatement
// (MLPPolicy.log_prob_np) performs these operations one by one.
__device__ __forceinline__ double gs_logp_term(double eps, double ls, double act) {
#pragma clang fp contract(off)
  return (((-0.5 * eps) * eps - ls) - 0.91893853320467274178) - log((1.0 - act * act) + 1e-6);
}

// logp[row0 + r] = terms[r][0] + terms[r][1] + ... in action order, one thread per row (the result does not depend on how the head
// mapped threads to actions); terms[r][a] at terms + r * stride + a in LDS, written by the head before this call
template <int ROWS>
__device__ __forceinline__ void gs_logp_rows(const double* terms, int stride, int A, int row0, int B, double* __restrict__ logp) {
  __syncthreads();
  const int r = threadIdx.x;
  if (r < ROWS && row0 + r < B) {
    double s = terms[r * stride];
    for (int a = 1; a < A; ++a) s += terms[r * stride + a];
    logp[row0 + r] = s;
  }
}
