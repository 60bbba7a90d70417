// kernels_pathwise.hip -- the pathwise actor step (pathwise.h; include/gridstep.h "the pathwise actor step"): the
// policy's loss is differentiated THROUGH the twin Q networks.  What stands between the unchanged matrix kernels of kernels_train.hip:
//   gs_k_pw_sample       per sample, float64 on the float32 pre-head values: the noise, the action a = tanh(mean + std eps), its
//                        log-probability, and the action columns of the twins' input rows
//   gs_k_pw_rows         the observation columns of those rows: a float32 copy, one thread per element
//   gs_k_pw_seed         the head gradient of a twin's value: 1.0f
//   gs_k_pw_input_grad   dQ/da: the backward pass continued through the twin's first layer to the action columns, and the twin's value
//   gs_k_pw_head         per sample: the smaller twin, the loss terms, and dL / d(pre-head) of the POLICY rounded once to float32
//   gs_k_pw_stats        ONE workgroup: the loss statistics and the gradient norm, in gs_k_train_stats' order
// No atomics: every sum has an order fixed by the networks' shapes and n.  Where include/gridstep.h states a formula nothing is
// contracted.
#include <hip/hip_runtime.h>
#include <math.h>

#include "block_reduce.h"
#include "env_device.h"
#include "pathwise.h"
#include "train.h"

namespace {

// ---- exp, tanh and log of the heads, from rounded float64 +, -, *, / alone (include/gridstep.h "the pathwise actor step" states them;
// learner.py's pathwise_exp_np / _tanh_np / _log_np perform the same operations one by one, so the heads are restated to the bit
// whatever library the host has).  Nothing is contracted; frexp, ldexp and rint are exact.
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

// component `comp` of the four normals of one Philox call (env_device.h's rng_normal_component), tag 'PWNO', counter (sample, quad, draw, tag)
__device__ __forceinline__ double gw_noise(uint64_t seed, uint32_t sample, uint32_t quad, uint32_t draw, int comp) {
  const U4 r = philox(sample, quad, draw, GS_PW_NOISE_TAG, (uint32_t)seed, (uint32_t)(seed >> 32));
  return rng_normal_component(r, comp);
}

}  // namespace

// ---- the sampled action, its log-probability and the action columns of the twins' input rows ---------------------------------------
extern "C" __global__ void __launch_bounds__(64)
gs_k_pw_sample(GsPwSampleArgs S) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S.n) return;
  const int A = S.A;
  const float* pre = S.pre + (size_t)i * S.row_stride;
  double* act = S.actions + (size_t)i * A;
  double* eps_out = S.noise + (size_t)i * A;
  float* sa = S.sa + (size_t)i * (S.D + A) + S.D;
  double lp = 0.0;
  for (int k = 0; k < A; ++k) {
    const double mean = (double)pre[k];
    const double ls = fmin(fmax((double)pre[A + k], -20.0), 2.0);
    const double eps = S.stochastic ? gw_noise(S.seed, (uint32_t)i, (uint32_t)(k >> 2), S.draw, k & 3) : 0.0;
    const double x = mean + gw_exp(ls) * eps;
    const double a = gw_tanh(x);
    const double term = gw_logp_term(eps, ls, a);
    lp = k ? lp + term : term;
    act[k] = a; eps_out[k] = eps; sa[k] = (float)a;
  }
  S.logp[i] = lp;
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_pw_rows(GsPwRowsArgs R) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)R.n * R.D) return;
  const long long i = t / R.D;
  const int c = (int)(t - i * R.D);
  R.sa[(size_t)i * R.DA + c] = R.obs[t];
}

extern "C" __global__ void __launch_bounds__(64)
gs_k_pw_seed(GsPwSeedArgs S) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S.n) return;
  float* g = S.ghead + (size_t)i * S.row_stride;
  g[0] = 1.0f;
  for (int k = 1; k < S.width16; ++k) g[k] = 0.0f;
}

// ---- dQ/da = delta0 W0[:, D .. D + A) --------------------------------------------------------------------------------------------
// One thread per (sample, action).  GS_PW_JT rows of W0's action columns lie in LDS at a time; a thread walks its sample's row of
// delta0 sixteen bytes at a time (the row starts at a multiple of 16 floats and is padded to one, with zeros) and adds the products in
// ascending j: ONE chain whose order depends on H0 alone.
extern "C" __global__ void __launch_bounds__(GS_PW_THREADS)
gs_k_pw_input_grad(GsPwInputGradArgs P) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float wl[GS_PW_JT * GS_PW_MAX_A];
  const int A = P.A, DA = P.D + P.A;
  const long long t = (long long)blockIdx.x * GS_PW_THREADS + threadIdx.x;
  const bool ok = t < (long long)P.n * A;
  const long long i = ok ? t / A : 0;
  const int k = ok ? (int)(t - i * A) : 0;
  const float* const drow = P.delta0 + (size_t)i * P.row_stride;
  float acc = 0.0f;
  for (int j0 = 0; j0 < P.H0; j0 += GS_PW_JT) {
    const int jn = min(GS_PW_JT, P.H0 - j0);
    if (j0) __syncthreads();                 // every thread has read the previous rows
    for (int e = threadIdx.x; e < jn * A; e += GS_PW_THREADS) {
      const int jj = e / A, kk = e - jj * A;
      wl[e] = P.W0[(size_t)(j0 + jj) * DA + P.D + kk];
    }
    __syncthreads();
    if (ok) {
      for (int jj = 0; jj < jn; jj += 4) {
        const float4 d = *(const float4*)(drow + j0 + jj);
        const float dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (jj + r < jn) {
            const float term = dv[r] * wl[(jj + r) * A + k];
            acc = (j0 + jj + r) ? acc + term : term;
          }
        }
      }
    }
  }
  if (!ok) return;
  P.dqda[t] = acc;
  if (k == 0) P.q[i] = (double)P.qpre[(size_t)i * P.row_stride];
}

// ---- the head: the smaller twin, the loss terms, dL / d(mean | log_std) ------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(64)
gs_k_pw_head(GsPwHeadArgs H) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H.n) return;
  const int A = H.A;
  const float* pre = H.pre + (size_t)i * H.row_stride;
  float* g = H.ghead + (size_t)i * H.row_stride;
  const double nd = (double)H.n;
  int w;
  if (H.q[0] && H.q[1]) w = H.q[0][i] <= H.q[1][i] ? 0 : 1;
  else w = H.q[0] ? 0 : 1;
  const double qmin = H.q[w][i];
  const float* dq = H.dqda[w] + (size_t)i * A;
  const double* a = H.actions + (size_t)i * A;
  const double* eps = H.noise + (size_t)i * A;
  const bool with_bc = H.bc_coef != 0.0;
  const double* stored = nullptr;
  if (with_bc) {
    long long j = H.idx[i];
    j = j < 0 ? 0 : (j >= H.N ? H.N - 1 : j);  // (an index the minibatch did not write cannot leave the rollout)
    stored = H.act + (size_t)j * A;
  }
  double bc = 0.0;
  for (int k = 0; k < A; ++k) {
    const double d = with_bc ? a[k] - stored[k] : 0.0;
    const double sq = d * d;
    bc = k ? bc + sq : sq;
  }
  H.which[i] = w; H.qmin[i] = qmin; H.bc[i] = bc;
  H.terms[i] = (H.alpha * H.logp[i] - qmin) + H.bc_coef * bc;
  for (int k = 0; k < A; ++k) {
    const double lsr = (double)pre[A + k];
    const bool inside = lsr >= -20.0 && lsr <= 2.0;
    const double ls = fmin(fmax(lsr, -20.0), 2.0);
    const double ak = a[k];
    const double om = 1.0 - ak * ak;
    const double d = with_bc ? ak - stored[k] : 0.0;
    const double t1 = (H.alpha * (2.0 * ak)) / (om + 1e-6);
    const double t2 = (2.0 * H.bc_coef) * d;
    const double G = (((t1 - (double)dq[k]) + t2) * om) / nd;
    g[k] = (float)G;
    g[A + k] = inside ? (float)((G * gw_exp(ls)) * eps[k] - H.alpha / nd) : 0.0f;
  }
  for (int k = 2 * A; k < H.width16; ++k) g[k] = 0.0f;
}

// ---- statistics of the step: ONE workgroup, thread i over entries i, i + 1024, ..., then the tree of gs_block_sum -------------------
extern "C" __global__ void __launch_bounds__(GS_TR_STAT_THREADS)
gs_k_pw_stats(GsPwStatArgs S) {
#pragma clang fp contract(off)
  __shared__ double lds[GS_TR_STAT_THREADS / 64];
  const int tid = threadIdx.x;
  double t0 = 0.0, tq = 0.0, tl = 0.0, gs = 0.0;
  for (int k = tid; k < S.n; k += GS_TR_STAT_THREADS) {
    t0 = t0 + S.terms[k];
    tq = tq + S.qmin[k];
    tl = tl + S.logp[k];
  }
  for (int k = tid; k < S.blocks; k += GS_TR_STAT_THREADS) gs = gs + S.blocksum[k];
  t0 = gs_block_sum(t0, lds);
  gs = gs_block_sum(gs, lds);
  tq = gs_block_sum(tq, lds); tl = gs_block_sum(tl, lds);
  if (tid) return;
  const double n = (double)S.n, nan = __builtin_nan("");
  double* o = S.stats;
  o[GS_TR_STAT_LOSS] = t0 / n;
  o[GS_TR_STAT_SURR] = tq / n; o[GS_TR_STAT_ENT] = -(tl / n);
  o[GS_TR_STAT_KL] = nan; o[GS_TR_STAT_CLIPFRAC] = nan; o[GS_TR_STAT_VLOSS] = nan;
  o[GS_TR_STAT_GNORM] = sqrt(gs);
}
