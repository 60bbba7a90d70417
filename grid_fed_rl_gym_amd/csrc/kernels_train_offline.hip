// kernels_train_offline.hip -- the in-sample losses of offline RL as heads of the learner (train.h; include/gridstep.h "the learner's
// loss").  They stand where gs_k_train_head and gs_k_train_stats stand in a step; the forward pass before them
// and the backward pass, the gradient reduction and Adam after them are the kernels of kernels_train.hip, unchanged.
//   gs_k_train_head_awr        per sample, float64 on the float32 pre-head values: the stored action's log-probability, the weight
//                              fmin(exp(A / temperature), weight_max), its cap flag, loss terms, dL / d(pre-head) rounded once
//   gs_k_train_head_expectile  a critic: q (v - ret)^2 with q = tau below the return and 1 - tau above it
//   gs_k_train_stats_awr       ONE workgroup: gs_k_train_stats for a policy whose rollout may hold no log-probabilities
// The expectile critic's statistics are gs_k_train_stats' own (a critic's sum of term0).
#include <hip/hip_runtime.h>
#include <math.h>

#include "block_reduce.h"
#include "bootstrap.h"
#include "train.h"

// ---- the advantage-weighted head: L = -(1/n) sum w_i lp_i - ent_coef (1/n) sum h_i -------------------------------------------------
extern "C" __global__ void __launch_bounds__(64)
gs_k_train_head_awr(GsTrainAwrHeadArgs H) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H.n) return;
  const float* pre = H.pre + (size_t)i * H.row_stride;
  float* g = H.ghead + (size_t)i * H.row_stride;
  const double inv_n = 1.0 / (double)H.n;
  const int A = H.A;
  const long long j = gb_row(H.idx[i], H.N);
  const double* act = H.act + (size_t)j * A;
  const double adv = (double)H.adv[i];
  const double lim = 1.0 - 1e-7;
  double lp = 0.0, ent = 0.0;
  for (int k = 0; k < A; ++k) {
    const double mean = (double)pre[k], lsr = (double)pre[A + k];
    const double ls = fmin(fmax(lsr, -20.0), 2.0);
    const double a = act[k];
    const double x = atanh(fmin(fmax(a, -lim), lim));
    const double e = (x - mean) * exp(-ls);
    const double term = (((-0.5 * e) * e - ls) - 0.91893853320467274178) - log((1.0 - a * a) + 1e-6);
    lp = k ? lp + term : term;
    const double h = ls + 1.4189385332046727418;      // 0.5 log(2 pi e)
    ent = k ? ent + h : h;
  }
  const double u = exp(adv / H.temperature);          // (temperature +inf: exp(0) = 1)
  const double w = fmin(u, H.weight_max);
  H.lp_new[i] = lp; H.weight[i] = w; H.capped[i] = u > H.weight_max ? 1 : 0;
  H.term0[i] = w * lp;
  H.term1[i] = ent;
  const double dlp = -(w * inv_n);
  const double dent = -(H.ent_coef * inv_n);
  for (int k = 0; k < A; ++k) {
    const double mean = (double)pre[k], lsr = (double)pre[A + k];
    const bool inside = lsr >= -20.0 && lsr <= 2.0;
    const double ls = fmin(fmax(lsr, -20.0), 2.0);
    const double x = atanh(fmin(fmax(act[k], -lim), lim));
    const double inv = exp(-ls);
    const double e = (x - mean) * inv;
    g[k] = (float)(dlp * (e * inv));
    g[A + k] = inside ? (float)(dlp * (e * e - 1.0) + dent) : 0.0f;
  }
  for (int k = 2 * A; k < H.width16; ++k) g[k] = 0.0f;
}

// ---- the expectile head: L = (1/n) sum q_i (v_i - ret_i)^2 --------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(64)
gs_k_train_head_expectile(GsTrainExpectileArgs H) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H.n) return;
  const float* pre = H.pre + (size_t)i * H.row_stride;
  float* g = H.ghead + (size_t)i * H.row_stride;
  const double inv_n = 1.0 / (double)H.n;
  const double d = (double)pre[0] - (double)H.ret[i];
  const double q = d < 0.0 ? H.tau : 1.0 - H.tau;
  H.term0[i] = q * (d * d);
  g[0] = (float)(q * ((2.0 * d) * inv_n));
  for (int k = 1; k < H.width16; ++k) g[k] = 0.0f;
}

// ---- statistics of an advantage-weighted step: ONE workgroup, thread i over entries i, i + 1024, ..., then the tree of gs_block_sum --
extern "C" __global__ void __launch_bounds__(GS_TR_STAT_THREADS)
gs_k_train_stats_awr(GsTrainAwrStatArgs S) {
#pragma clang fp contract(off)
  __shared__ double lds[GS_TR_STAT_THREADS / 64];
  __shared__ long long lds_i[GS_TR_STAT_THREADS / 64];
  const int tid = threadIdx.x;
  const bool have_old = S.logp != nullptr;
  double t0 = 0.0, t1 = 0.0, kl = 0.0, gs = 0.0;
  long long nc = 0;
  for (int k = tid; k < S.n; k += GS_TR_STAT_THREADS) {
    t0 = t0 + S.term0[k];
    t1 = t1 + S.term1[k];
    if (have_old) {
      const long long j = gb_row(S.idx[k], S.N);
      kl = kl + (S.logp[j] - S.lp_new[k]);
    }
    nc += S.capped[k];
  }
  for (int k = tid; k < S.blocks; k += GS_TR_STAT_THREADS) gs = gs + S.blocksum[k];
  t0 = gs_block_sum(t0, lds);
  gs = gs_block_sum(gs, lds);
  t1 = gs_block_sum(t1, lds); kl = gs_block_sum(kl, lds); nc = gs_block_sum(nc, lds_i);
  if (tid) return;
  const double n = (double)S.n, nan = __builtin_nan("");
  const double surr = t0 / n, ent = t1 / n;
  double* o = S.stats;
  o[GS_TR_STAT_LOSS] = -surr - S.ent_coef * ent;
  o[GS_TR_STAT_SURR] = surr; o[GS_TR_STAT_ENT] = ent; o[GS_TR_STAT_KL] = have_old ? kl / n : nan; o[GS_TR_STAT_CLIPFRAC] = (double)nc / n;
  o[GS_TR_STAT_VLOSS] = nan;
  o[GS_TR_STAT_GNORM] = sqrt(gs);
}
