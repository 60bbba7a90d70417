// kernels_episodes.hip -- episode accounting over the last rollout (GsEpisodeArgs, gs_internal.h; include/gridstep.h "episode
// accounting"): which episodes the rollout finished, what each returned, how long it ran and what it cost.
//   gs_k_ep_count        seg[b] = the transitions of instance b that ended an episode
//   gs_k_ep_offsets      seg -> its exclusive prefix sum, the total to n_ep: ONE workgroup, a chunk of B per trip, the total carried
//   gs_k_ep_accumulate   the recurrence per instance, t = 0 .. T - 1 in order; records from seg[b] on; the carries stored
//   gs_k_ep_stats        ONE workgroup over the list: counts, extremes, means, the standard deviation
// Every [.][B] array is read with the lanes along b, so a wavefront's accesses are contiguous.  Stores are 4 or 8 bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.h"
#include "gs_internal.h"

extern "C" __global__ void __launch_bounds__(256)
gs_k_ep_count(GsEpisodeArgs E) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= E.B) return;
  const uint8_t* const done = E.done + b;
  const size_t B = (size_t)E.B;
  int n = 0, t = 0;
  for (; t + 8 <= E.T; t += 8) {      // eight steps' flags in flight
    uint8_t f[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) f[u] = done[(size_t)(t + u) * B];
#pragma unroll
    for (int u = 0; u < 8; ++u) n += f[u] != 0;
  }
  for (; t < E.T; ++t) n += done[(size_t)t * B] != 0;
  E.seg[b] = n;
}

// ---- the offset pass -----------------------------------------------------------------------------------------------------------
template <int CTRL, int ROWS> __device__ __forceinline__ int ep_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROWS, 0xf, false); }
// inclusive prefix sum over the 64 lanes of a wavefront: four shifts inside each row of 16, then the rows' last lanes broadcast on
__device__ __forceinline__ int ep_wave_scan(int v) {
  v += ep_dpp<0x111, 0xf>(v);      // row_shr:1
  v += ep_dpp<0x112, 0xf>(v);      // row_shr:2
  v += ep_dpp<0x114, 0xf>(v);      // row_shr:4
  v += ep_dpp<0x118, 0xf>(v);      // row_shr:8
  v += ep_dpp<0x142, 0xa>(v);      // row_bcast:15 -> rows 1 and 3 take lane 15 of the row before
  v += ep_dpp<0x143, 0xc>(v);      // row_bcast:31 -> rows 2 and 3 take lane 31
  return v;
}

extern "C" __global__ void __launch_bounds__(GS_EP_SCAN_THREADS)
gs_k_ep_offsets(GsEpisodeArgs E) {
  constexpr int W = GS_EP_SCAN_THREADS / 64;
  __shared__ int wave_total[W];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int base = 0; base < E.B; base += GS_EP_SCAN_THREADS) {      // (uniform: every thread takes every trip)
    const int i = base + tid;
    const int v = i < E.B ? E.seg[i] : 0;
    const int incl = ep_wave_scan(v);
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < W; ++w) { const int x = wave_total[w]; before += w < wave ? x : 0; total += x; }
    if (i < E.B) E.seg[i] = carry + before + (incl - v);
    carry += total;
    __syncthreads();
  }
  if (tid == 0) *E.n_ep = carry;
}

// ---- the accumulate pass -------------------------------------------------------------------------------------------------------
// One thread per instance, U steps' loads issued before the first dependent addition; the additions themselves stay in step order.
template <bool COSTS, int U>
__device__ __forceinline__ void ep_accumulate(const GsEpisodeArgs& E) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = b < E.B;
  const int bb = live ? b : 0;      // (idle lanes of the last workgroup read instance 0 and store nothing)
  const size_t B = (size_t)E.B;
  double ret = 0.0, cost[3] = {0.0, 0.0, 0.0};
  int len = 0, ord = 0, partial = E.start == GS_EP_UNKNOWN ? 1 : 0, viol[3] = {0, 0, 0}, anyv = 0;
  if (E.start == GS_EP_CONTINUE) {
    ret = E.c_ret[bb]; len = E.c_len[bb]; ord = E.c_ord[bb]; partial = ((const uint8_t*)E.c_partial)[bb];
    if constexpr (COSTS) {
      for (int c = 0; c < 3; ++c) { cost[c] = E.c_cost[c * B + bb]; viol[c] = E.c_viol[c * B + bb]; }
      anyv = E.c_anyv[bb];
    }
  }
  long long k = live ? E.seg[bb] : E.cap;
  auto step = [&](int t, double r, uint8_t flag, const double* cs, const double* mg) {
    ret = ret + r;
    len += 1;
    if constexpr (COSTS) {
      bool any = false;
      for (int c = 0; c < 3; ++c) { cost[c] = cost[c] + cs[c]; const bool v = mg[c] < 0.0; viol[c] += v; any = any || v; }
      anyv += any;
    }
    if (flag != 0) {
      if (live && k < E.cap) {
        E.e_idx[2 * k] = t; E.e_idx[2 * k + 1] = b;
        E.e_ret[k] = ret; E.e_len[k] = len; E.e_ord[k] = ord; E.e_flags[k] = (flag & 3) | (partial ? GS_EP_PARTIAL : 0);
        if constexpr (COSTS) {
          for (int c = 0; c < 3; ++c) { E.e_cost[(size_t)c * E.cap + k] = cost[c]; E.e_viol[(size_t)c * E.cap + k] = viol[c]; }
          E.e_anyv[k] = anyv;
        }
      }
      k += 1;
      ret = 0.0; len = 0; ord += 1; partial = 0;
      if constexpr (COSTS) { for (int c = 0; c < 3; ++c) { cost[c] = 0.0; viol[c] = 0; } anyv = 0; }
    }
  };
  int t0 = 0;
  for (; t0 + U <= E.T; t0 += U) {
    double r[U], cs[U][3], mg[U][3]; uint8_t f[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = (size_t)(t0 + u) * B + bb;
      r[u] = E.rew[i]; f[u] = E.done[i];
      if constexpr (COSTS)
        for (int c = 0; c < 3; ++c) { cs[u][c] = E.costs[c * E.chan_stride + i]; mg[u][c] = E.margins[c * E.chan_stride + i]; }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) step(t0 + u, r[u], f[u], cs[u], mg[u]);
  }
  for (int t = t0; t < E.T; ++t) {
    const size_t i = (size_t)t * B + bb;
    double cs[3] = {0.0, 0.0, 0.0}, mg[3] = {0.0, 0.0, 0.0};
    if constexpr (COSTS)
      for (int c = 0; c < 3; ++c) { cs[c] = E.costs[c * E.chan_stride + i]; mg[c] = E.margins[c * E.chan_stride + i]; }
    step(t, E.rew[i], E.done[i], cs, mg);
  }
  // the partial flags of four neighbouring instances as one word (lanes 4 j .. 4 j + 3 -> lane 4 j; idle lanes give 0)
  unsigned word = live ? (unsigned)partial : 0u;
  word |= (unsigned)__shfl_down((int)word, 1) << 8;
  word |= (unsigned)__shfl_down((int)word, 2) << 16;
  if (!live) return;
  if ((b & 3) == 0) E.c_partial[b >> 2] = word;
  E.c_ret[b] = ret; E.c_len[b] = len; E.c_ord[b] = ord;
  if constexpr (COSTS) {
    for (int c = 0; c < 3; ++c) { E.c_cost[c * B + b] = cost[c]; E.c_viol[c * B + b] = viol[c]; }
    E.c_anyv[b] = anyv;
  }
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_ep_accumulate(GsEpisodeArgs E) { ep_accumulate<false, 8>(E); }

extern "C" __global__ void __launch_bounds__(256)
gs_k_ep_accumulate_costs(GsEpisodeArgs E) { ep_accumulate<true, 4>(E); }

// ---- the statistics pass -------------------------------------------------------------------------------------------------------
// Every quantity is reduced over the workgroup by block_reduce.h (the order of the operations is stated there), the 16 wavefronts
// known at compile time (fmin and fmax: its GsMin and GsMax).
constexpr int EP_STAT_WAVES = GS_EP_STAT_THREADS / 64;
static_assert(EP_STAT_WAVES == 16, "the second butterfly runs over 16 lanes");

extern "C" __global__ void __launch_bounds__(GS_EP_STAT_THREADS)
gs_k_ep_stats(GsEpisodeArgs E) {
#pragma clang fp contract(off)
  __shared__ double lds_f[GS_EP_STAT_THREADS / 64];
  __shared__ long long lds_i[GS_EP_STAT_THREADS / 64];
  const int tid = threadIdx.x;
  const bool with_costs = E.e_cost != nullptr;
  const int n = min(*E.n_ep, E.cap);
  const double inf = __builtin_inf(), nan = __builtin_nan("");
  // pass 1: each thread over entries tid, tid + 1024, ... in order
  long long cnt = 0, cnt_partial = 0, len_sum = 0, viol[3] = {0, 0, 0}, n_success = 0;
  double ret_sum = 0.0, ret_min = inf, ret_max = -inf, len_min = inf, len_max = -inf, cost_sum[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
  for (int k = tid; k < n; k += GS_EP_STAT_THREADS) {
    if (E.e_flags[k] & GS_EP_PARTIAL) { cnt_partial += 1; continue; }
    const double r = E.e_ret[k];
    const int len = E.e_len[k];
    cnt += 1; ret_sum = ret_sum + r; ret_min = fmin(ret_min, r); ret_max = fmax(ret_max, r);
    len_sum += len; len_min = fmin(len_min, (double)len); len_max = fmax(len_max, (double)len);
    bool clean = true;
    if (with_costs) {
      for (int c = 0; c < 3; ++c) { cost_sum[c] = cost_sum[c] + E.e_cost[(size_t)c * E.cap + k]; viol[c] += E.e_viol[(size_t)c * E.cap + k]; }
      clean = E.e_anyv[k] == 0;
    }
    n_success += clean && r > E.success_return;
  }
  cnt = gs_block_sum<EP_STAT_WAVES>(cnt, lds_i);
  cnt_partial = gs_block_sum<EP_STAT_WAVES>(cnt_partial, lds_i);
  len_sum = gs_block_sum<EP_STAT_WAVES>(len_sum, lds_i);
  n_success = gs_block_sum<EP_STAT_WAVES>(n_success, lds_i);
  ret_sum = gs_block_sum<EP_STAT_WAVES>(ret_sum, lds_f);
  ret_min = gs_block_reduce<EP_STAT_WAVES>(ret_min, lds_f, GsMin());
  ret_max = gs_block_reduce<EP_STAT_WAVES>(ret_max, lds_f, GsMax());
  len_min = gs_block_reduce<EP_STAT_WAVES>(len_min, lds_f, GsMin());
  len_max = gs_block_reduce<EP_STAT_WAVES>(len_max, lds_f, GsMax());
  if (with_costs)
    for (int c = 0; c < 3; ++c) { cost_sum[c] = gs_block_sum<EP_STAT_WAVES>(cost_sum[c], lds_f); viol[c] = gs_block_sum<EP_STAT_WAVES>(viol[c], lds_i); }
  const double N = (double)cnt;
  const double mean = ret_sum / N;
  // pass 2: the squared deviations from the mean, the same entries in the same order
  double m2 = 0.0;
#pragma unroll 4
  for (int k = tid; k < n; k += GS_EP_STAT_THREADS) {
    if (E.e_flags[k] & GS_EP_PARTIAL) continue;
    const double d = E.e_ret[k] - mean;
    m2 = m2 + d * d;
  }
  m2 = gs_block_sum<EP_STAT_WAVES>(m2, lds_f);
  if (tid != 0) return;
  GsEpisodeStats& S = *E.stats;
  const bool some = cnt > 0;
  S.count = cnt; S.count_partial = cnt_partial;
  S.ret_mean = some ? mean : nan; S.ret_std = some ? sqrt(m2 / N) : nan;
  S.ret_min = some ? ret_min : nan; S.ret_max = some ? ret_max : nan;
  S.len_mean = some ? (double)len_sum / N : nan; S.len_min = some ? len_min : nan; S.len_max = some ? len_max : nan;
  for (int c = 0; c < 3; ++c) { S.cost_mean[c] = some && with_costs ? cost_sum[c] / N : nan; S.violating[c] = viol[c]; }
  S.n_success = n_success;
}
