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
#include "bootstrap.h"
#include "env_device.h"
#include "gw_math.h"
#include "pathwise.h"
#include "train.h"

namespace {

// exp, tanh and log of the heads (gw_exp, gw_tanh, gw_log, gw_logp_term): gw_math.h, shared with kernels_q_next.hip

// component `comp` of the four normals of one Philox call (env_device.h's rng_normal_component), counter (sample, quad, draw, tag);
// tag 0: 'PWNO'
__device__ __forceinline__ double gw_noise(uint64_t seed, uint32_t sample, uint32_t quad, uint32_t draw, uint32_t tag, int comp) {
  const U4 r = philox(sample, quad, draw, tag ? tag : GS_PW_NOISE_TAG, (uint32_t)seed, (uint32_t)(seed >> 32));
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
    const double eps = S.stochastic ? gw_noise(S.seed, (uint32_t)i, (uint32_t)(k >> 2), S.draw, S.tag, k & 3) : 0.0;
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
    j = GS_RF_CLAMP(j, H.N);                 // (gb_row's rule, as text: called, H.N is read ahead of the test and this kernel's code changes)
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
