// kernels_conservative.hip -- the conservative critic step (conservative.h; include/gridstep.h "the conservative critic step";
// DESIGN.md section 26): one twin's regression on its Bellman target plus conservative_weight times
//     logsumexp over ALL 3 n values Q(s, a_data) | Q(s, a_uniform) | Q(s, a_policy)  -  mean Q(s, a_data),
// the logsumexp running over the batch as the reference's does.  What stands between the unchanged kernels of kernels_train.hip,
// gs_k_q_gather (the data block and the targets) and gs_k_pw_sample (the policy block's actions):
//   gs_k_cql_rows    the observation columns of the uniform and the policy block, and the uniform actions
//   gs_k_cql_lse     ONE workgroup: the maximum, the sum of exponentials, the logsumexp and the data rows' mean
//   gs_k_cql_head    per row: the softmax weight, the data rows' loss term, dL/dq rounded once to float32
//   gs_k_cql_stats   ONE workgroup: the loss statistics and the gradient norm, in gs_k_train_stats' order
// No atomics: every sum has an order fixed by n.  Where include/gridstep.h states a formula nothing is contracted.
#include <hip/hip_runtime.h>
#include <math.h>

#include "block_reduce.h"
#include "conservative.h"
#include "env_device.h"
#include "gw_math.h"
#include "train.h"

namespace {

// e_j of the logsumexp: the head recomputes what the reduction summed, from the same two float64 values, so the bits agree
__device__ __forceinline__ double cql_exp_below(double q, double m) {
#pragma clang fp contract(off)
  const double d = q - m;
  return d < GS_CQL_EXP_FLOOR ? 0.0 : gw_exp(d);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256)
gs_k_cql_rows(GsCqlRowsArgs R) {
#pragma clang fp contract(off)
  const int DA = R.D + R.A;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)R.n * DA) return;
  const long long i = t / DA;
  const int c = (int)(t - i * DA);
  float* const uniform = R.sa + ((size_t)R.n + i) * DA;
  if (c < R.D) {
    const float o = R.obs[(size_t)i * R.D + c];
    uniform[c] = o;
    R.sa[((size_t)2 * R.n + i) * DA + c] = o;
  } else {
    const int k = c - R.D;
    const U4 r = philox((uint32_t)i, (uint32_t)(k >> 2), R.draw, GS_CQL_UNIFORM_TAG, (uint32_t)R.seed, (uint32_t)(R.seed >> 32));
    const uint32_t word = (k & 2) ? ((k & 1) ? r.d : r.c) : ((k & 1) ? r.b : r.a);
    const double u = ((double)word + 0.5) * (1.0 / 2147483648.0) - 1.0;
    R.random[(size_t)i * R.A + k] = u;
    uniform[c] = (float)u;
  }
}

// thread t takes j = t, t + 1024, ... ascending, then the tree of gs_block_reduce: gs_k_train_stats' order
extern "C" __global__ void __launch_bounds__(GS_TR_STAT_THREADS)
gs_k_cql_lse(GsCqlLseArgs L) {
#pragma clang fp contract(off)
  __shared__ double lds[GS_TR_STAT_THREADS / 64];
  const int tid = threadIdx.x, rows = 3 * L.n;
  double m = -__builtin_inf();
  for (int j = tid; j < rows; j += GS_TR_STAT_THREADS) m = fmax(m, (double)L.qpre[(size_t)j * L.row_stride]);
  m = gs_block_reduce(m, lds, GsMax());
  double s = 0.0, sq = 0.0;
  for (int j = tid; j < rows; j += GS_TR_STAT_THREADS) {
    const double q = (double)L.qpre[(size_t)j * L.row_stride];
    s = s + cql_exp_below(q, m);
    if (j < L.n) sq = sq + q;
  }
  s = gs_block_sum(s, lds);
  sq = gs_block_sum(sq, lds);
  if (tid) return;
  L.scalars[0] = m; L.scalars[1] = s; L.scalars[2] = m + gw_log(s); L.scalars[3] = sq / (double)L.n;
}

extern "C" __global__ void __launch_bounds__(64)
gs_k_cql_head(GsCqlHeadArgs H) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= 3 * H.n) return;
  const double q = (double)H.qpre[(size_t)j * H.row_stride];
  const double p = cql_exp_below(q, H.scalars[0]) / H.scalars[1];
  const double inv_n = 1.0 / (double)H.n;
  double g;
  if (j < H.n) {
    const double dq = q - (double)H.y[j];
    H.terms[j] = dq * dq;
    g = (2.0 * dq) * inv_n + H.cw * (p - inv_n);
  } else {
    g = H.cw * p;
  }
  H.q[j] = q; H.weights[j] = p;
  float* const gh = H.ghead + (size_t)j * H.row_stride;
  gh[0] = (float)g;
  for (int k = 1; k < H.width16; ++k) gh[k] = 0.0f;
}

extern "C" __global__ void __launch_bounds__(GS_TR_STAT_THREADS)
gs_k_cql_stats(GsCqlStatArgs S) {
#pragma clang fp contract(off)
  __shared__ double lds[GS_TR_STAT_THREADS / 64];
  const int tid = threadIdx.x;
  double t0 = 0.0, gs = 0.0;
  for (int k = tid; k < S.n; k += GS_TR_STAT_THREADS) t0 = t0 + S.terms[k];
  for (int k = tid; k < S.blocks; k += GS_TR_STAT_THREADS) gs = gs + S.blocksum[k];
  t0 = gs_block_sum(t0, lds);
  gs = gs_block_sum(gs, lds);
  if (tid) return;
  const double nan = __builtin_nan("");
  const double vl = t0 / (double)S.n, penalty = S.scalars[2] - S.scalars[3];
  double* o = S.stats;
  o[GS_TR_STAT_LOSS] = vl + S.cw * penalty; o[GS_TR_STAT_VLOSS] = vl; o[GS_TR_STAT_SURR] = penalty;
  o[GS_TR_STAT_ENT] = nan; o[GS_TR_STAT_KL] = nan; o[GS_TR_STAT_CLIPFRAC] = nan;
  o[GS_TR_STAT_GNORM] = sqrt(gs);
}
