// kernels_refresh.hip -- per-minibatch refresh of the rollout's bootstrap signals (include/gridstep.h "per-minibatch targets";
// DESIGN.md section 27):
//   gs_k_refresh_terms       the batch rows that end an episode under the mask, compacted in ascending order (one workgroup)
//   gs_k_refresh_rows        the observation rows, stored actions and (t, b) pairs of the batch, gathered into contiguous blocks
//   gs_k_refresh_td_policy   gs_k_q_next_td's arithmetic on the refreshed rows, scattered to their transitions and terminal entries
//   gs_k_refresh_td_value    gs_k_q_td's
//   gs_k_refresh_combine     gs_k_q_combine's, one source at a time
// "The arithmetic of" is a fact of the code: those kernels and these call the same functions of bootstrap.h.
// The networks between the gather and the scatter are the existing kernels (gs_k_policy_rows_f32, gs_k_q_mlp_f32 / _rows_f32,
// gs_k_value_mlp_f32) over the gathered blocks.  One thread per element or batch row; where include/gridstep.h states a formula
// nothing is contracted.  Duplicate indices in a batch compute the same bits from the same inputs, so their colliding stores are benign.
#include <hip/hip_runtime.h>
#include <math.h>

#include "bootstrap.h"
#include "refresh.h"

extern "C" __global__ void __launch_bounds__(GS_RF_TERM_THREADS)
gs_k_refresh_terms(GsRefreshTermsArgs G) {
  constexpr int WAVES = GS_RF_TERM_THREADS / 64;
  __shared__ int wsum[WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int running = 0;                           // (the same in every thread)
  for (int base = 0; base < G.n; base += GS_RF_TERM_THREADS) {
    const int i = base + tid;
    int e = -1;
    if (i < G.n) {
      const long long j = gb_row(G.idx[i], G.N);
      if (G.done[j] & G.mask) e = G.map[j];
    }
    const unsigned long long ballot = __ballot(e >= 0);
    const int before = __popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(ballot);
    __syncthreads();
    int off = running, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      if (w < wave) off += wsum[w];
      total += wsum[w];
    }
    if (i < G.n) {
      int k = -1;
      if (e >= 0) {
        k = off + before;
        G.ie[2 * k] = i; G.ie[2 * k + 1] = e;
        G.tb[2 * k] = G.term_idx[2 * e]; G.tb[2 * k + 1] = G.term_idx[2 * e + 1];
      }
      G.pos[i] = k;
    }
    running += total;
    __syncthreads();                         // (wsum is rewritten by the next chunk)
  }
  if (tid == 0) G.count[0] = running;
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_refresh_rows(GsRefreshRowsArgs G) {
  const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= (long long)G.n * G.W) return;
  const int i = (int)(x / G.W), c = (int)(x - (long long)i * G.W);
  const long long j = gb_row(G.idx[i], G.N);
  if (c < G.D) {
    if (G.own) G.own[(size_t)i * G.D + c] = G.obs_seq[(size_t)j * G.D + c];
    if (G.next) G.next[(size_t)i * G.D + c] = G.obs_seq[(size_t)(j + G.B) * G.D + c];
    if (G.term && i < min(*G.count, G.n)) G.term[(size_t)i * G.D + c] = G.term_obs[(size_t)G.ie[2 * i + 1] * G.D + c];
  }
  if (c < G.A && G.act) G.act[(size_t)i * G.A + c] = G.actions[(size_t)j * G.A + c];
  if (c < 2 && G.tb) G.tb[2 * i + c] = c == 0 ? (int32_t)(j / G.B) : (int32_t)(j % G.B);
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_refresh_td_policy(GsRefreshTdPolicyArgs G) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G.n) return;
  const size_t j = (size_t)gb_row(G.idx[i], G.N);
  const int A = G.A;
  for (int c = 0; c < 2 * A; ++c) G.pre[j * (2 * A) + c] = G.s_pre[(size_t)i * (2 * A) + c];
  for (int c = 0; c < A; ++c) {
    G.act[j * A + c] = G.s_act[(size_t)i * A + c];
    G.eps[j * A + c] = G.s_eps[(size_t)i * A + c];
  }
  const double lp = G.s_lp[i];
  G.lp[j] = lp;
  if (G.s_q[0]) G.q[0][j] = G.s_q[0][i];
  if (G.s_q[1]) G.q[1][j] = G.s_q[1][i];
  const double m = gb_twin_min(G.s_q[0], G.s_q[1], (size_t)i);
  G.q_min[j] = m;
  const double v = gb_soft_value(m, G.alpha, lp);
  double vnext = G.done[j] ? 0.0 : v;
  const int k = G.pos ? G.pos[i] : -1;
  if (k >= 0) {
    const size_t e = (size_t)G.ie[2 * k + 1];
    for (int c = 0; c < 2 * A; ++c) G.t_pre[e * (2 * A) + c] = G.st_pre[(size_t)k * (2 * A) + c];
    for (int c = 0; c < A; ++c) {
      G.t_act[e * A + c] = G.st_act[(size_t)k * A + c];
      G.t_eps[e * A + c] = G.st_eps[(size_t)k * A + c];
    }
    const double tlp = G.st_lp[k];
    G.t_lp[e] = tlp;
    if (G.st_q[0]) G.t_q[0][e] = G.st_q[0][k];
    if (G.st_q[1]) G.t_q[1][e] = G.st_q[1][k];
    const double tm = gb_twin_min(G.st_q[0], G.st_q[1], (size_t)k);
    G.t_q_min[e] = tm;
    vnext = gb_soft_value(tm, G.alpha, tlp);
    G.t_value[e] = vnext;
  }
  G.td[j] = gb_td(G.rew[j], G.reward_shift, G.reward_scale, G.gamma, vnext);
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_refresh_td_value(GsRefreshTdValueArgs G) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G.n) return;
  const size_t j = (size_t)gb_row(G.idx[i], G.N);
  double vnext = G.vn[i];
  if (G.done[j]) {
    const int k = G.pos ? G.pos[i] : -1;
    vnext = k >= 0 ? G.tv[k] : 0.0;
  }
  G.td[j] = gb_td(G.rew[j], G.reward_shift, G.reward_scale, G.gamma, vnext);
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_refresh_combine(GsRefreshCombineArgs C) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C.n) return;
  const size_t j = (size_t)gb_row(C.idx[i], C.N);
  if (C.s_q[0]) C.q[0][j] = C.s_q[0][i];
  if (C.s_q[1]) C.q[1][j] = C.s_q[1][i];
  const double m = gb_twin_min(C.s_q[0], C.s_q[1], (size_t)i);
  C.q_min[j] = m;
  if (C.values) C.q_adv[j] = m - C.values[i];
}
