// kernels_batches.hip -- on-policy minibatch epochs over the last rollout (GsOpb*Args, gs_internal.h; include/gridstep.h "on-policy
// minibatch epochs"): the combined advantage, the keyed permutation, the minibatch's statistics and the gather.
//   gs_k_opb_combine     comb[j] = adv[j] - lambda[0] cadv[0][j] - ...: one thread per transition, every operation rounded on its own
//   gs_k_opb_index       one thread per position of the minibatch: the permutation walk, idx[i] = j, stage[i] = comb[j]
//   gs_k_opb_mbstats     ONE workgroup over stage: mean and population standard deviation in the order of gs_k_ep_stats
//   gs_k_opb_gather_*    one wavefront per sample, lanes along the observation's columns; the sample's scalars by its first lanes
// Nothing here reads or writes the slab: the kernels see the rollout's and the critics' arrays (read only) and the batch's own.
// Stores are 4 or 8 bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "block_reduce.h"
#include "gs_internal.h"
#include "env_device.h"

namespace {

// one pass of the four-round Feistel network over [0, 2^(2 hb)): include/gridstep.h
__device__ __forceinline__ uint32_t opb_pass(uint32_t x, int hb, uint32_t mask, uint32_t epoch, uint32_t k0, uint32_t k1) {
  uint32_t L = x >> hb, R = x & mask;
#pragma unroll
  for (uint32_t round = 0; round < 4; ++round) {
    const uint32_t w = philox(R, round, epoch, 0x5045524Du, k0, k1).a;
    const uint32_t next = L ^ (w & mask);
    L = R; R = next;
  }
  return (L << hb) | R;
}

// gs_k_ep_stats's reduction (kernels_episodes.hip): block_reduce.h over the 16 wavefronts, known at compile time
constexpr int OPB_STAT_WAVES = GS_OPB_STAT_THREADS / 64;
static_assert(OPB_STAT_WAVES == 16, "the second butterfly runs over 16 lanes");

}  // namespace

extern "C" {

__global__ void __launch_bounds__(256)
gs_k_opb_combine(GsOpbCombineArgs A) {
#pragma clang fp contract(off)
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.N) return;
  double v = A.adv[j];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (A.cadv[c]) { const double share = A.lambda[c] * A.cadv[c][j]; v = v - share; }
  A.comb[j] = v;
}

__global__ void __launch_bounds__(256)
gs_k_opb_index(GsOpbIndexArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && A.adv_stats && A.adv_norm != GS_OPB_NORM_MINIBATCH) {
    const bool roll = A.adv_norm == GS_OPB_NORM_ROLLOUT;
    A.adv_stats[0] = roll ? A.roll_stats[0] : __builtin_nan("");
    __asm__ volatile("" ::: "memory");      // (two 8-byte stores, not one of 16)
    A.adv_stats[1] = roll ? A.roll_stats[1] : __builtin_nan("");
  }
  if (i >= A.n) return;
  const uint32_t mask = (1u << A.half_bits) - 1u;
  // the walk: first + i < N (checked on the host) lies on a cycle of the bijection, so it comes back below N
  uint32_t y = (uint32_t)(A.first + i);
  do y = opb_pass(y, A.half_bits, mask, A.epoch, A.seed_lo, A.seed_hi); while ((long long)y >= A.N);
  A.idx[i] = (int32_t)y;
  if (A.comb) A.stage[i] = A.comb[y];
}

__global__ void __launch_bounds__(GS_OPB_STAT_THREADS)
gs_k_opb_mbstats(const double* __restrict__ stage, int n, double* __restrict__ adv_stats) {
#pragma clang fp contract(off)
  __shared__ double lds[GS_OPB_STAT_THREADS / 64];
  const int tid = threadIdx.x;
  // pass 1: each thread over entries tid, tid + 1024, ... in order
  double sum = 0.0;
#pragma unroll 4
  for (int k = tid; k < n; k += GS_OPB_STAT_THREADS) sum = sum + stage[k];
  sum = gs_block_sum<OPB_STAT_WAVES>(sum, lds);
  const double dn = (double)n;
  const double mean = sum / dn;
  // pass 2: the squared deviations from the mean, the same entries in the same order
  double m2 = 0.0;
#pragma unroll 4
  for (int k = tid; k < n; k += GS_OPB_STAT_THREADS) {
    const double d = stage[k] - mean;
    m2 = m2 + d * d;
  }
  m2 = gs_block_sum<OPB_STAT_WAVES>(m2, lds);
  if (tid != 0) return;
  adv_stats[0] = mean;
  __asm__ volatile("" ::: "memory");      // (two 8-byte stores, not one of 16)
  adv_stats[1] = sqrt(m2 / dn);
}

}  // extern "C"

// ---- the gather ------------------------------------------------------------------------------------------------------------------
namespace {

// W values of type O at o: one 8-byte store for a float pair; a double pair goes out as two 8-byte stores, kept apart
template <typename O, int W> struct OpbPut;
template <> struct OpbPut<float, 1> { static __device__ __forceinline__ void put(float* o, const double* y) { o[0] = (float)y[0]; } };
template <> struct OpbPut<double, 1> { static __device__ __forceinline__ void put(double* o, const double* y) { o[0] = y[0]; } };
template <> struct OpbPut<float, 2> {
  static __device__ __forceinline__ void put(float* o, const double* y) { *(float2*)o = make_float2((float)y[0], (float)y[1]); }
};
template <> struct OpbPut<double, 2> {
  static __device__ __forceinline__ void put(double* o, const double* y) {
    o[0] = y[0];
    __asm__ volatile("" ::: "memory");
    o[1] = y[1];
  }
};

// The observation rows of the wavefront's samples.  A lane owns W neighbouring columns per pass (W = 2: 16-byte loads) and keeps
// their shift and scale over GS_OPB_PASSES passes while the samples go by; every load of the passes is issued before the first is used.
template <typename O, int W>
__device__ __forceinline__ void opb_rows(const GsOpbGatherArgs& G, const long long (&j)[GS_OPB_SAMPLES], const int (&i)[GS_OPB_SAMPLES],
                                         const bool (&ok)[GS_OPB_SAMPLES], int lane) {
#pragma clang fp contract(off)
  typedef double V __attribute__((ext_vector_type(W)));
  const int D = G.D;
  const bool norm = G.shift != nullptr;
  for (int c0 = 0; c0 < D; c0 += 64 * W * GS_OPB_PASSES) {
    // raw rows: (x - 0) * 1 gives x's bits back
    V sh[GS_OPB_PASSES], sc[GS_OPB_PASSES];
#pragma unroll
    for (int p = 0; p < GS_OPB_PASSES; ++p) {
      const int c = c0 + (p * 64 + lane) * W;
      sh[p] = 0.0; sc[p] = 1.0;
      if (norm && c < D) { sh[p] = *(const V*)(G.shift + c); sc[p] = *(const V*)(G.scale + c); }
    }
    V x[GS_OPB_SAMPLES][GS_OPB_PASSES];
#pragma unroll
    for (int s = 0; s < GS_OPB_SAMPLES; ++s)
#pragma unroll
      for (int p = 0; p < GS_OPB_PASSES; ++p) {
        const int c = c0 + (p * 64 + lane) * W;
        x[s][p] = 0.0;
        if (ok[s] && c < D) x[s][p] = *(const V*)(G.obs_seq + (size_t)j[s] * D + c);
      }
#pragma unroll
    for (int s = 0; s < GS_OPB_SAMPLES; ++s)
#pragma unroll
      for (int p = 0; p < GS_OPB_PASSES; ++p) {
        const int c = c0 + (p * 64 + lane) * W;
        if (!(ok[s] && c < D)) continue;
        double y[W];
#pragma unroll
        for (int w = 0; w < W; ++w) { const double d = x[s][p][w] - sh[p][w]; y[w] = d * sc[p][w]; }
        OpbPut<O, W>::put((O*)G.out_obs + (size_t)i[s] * D + c, y);
      }
  }
}

template <typename O>
__device__ __forceinline__ void opb_gather(const GsOpbGatherArgs& G) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int first = (blockIdx.x * GS_OPB_WAVES + (threadIdx.x >> 6)) * GS_OPB_SAMPLES;
  int i[GS_OPB_SAMPLES]; long long j[GS_OPB_SAMPLES]; bool ok[GS_OPB_SAMPLES];
#pragma unroll
  for (int s = 0; s < GS_OPB_SAMPLES; ++s) {
    i[s] = first + s;
    ok[s] = i[s] < G.n;
    j[s] = ok[s] ? G.idx[i[s]] : 0;
    ok[s] = ok[s] && j[s] >= 0 && j[s] < G.N;      // (the index kernel writes nothing else)
  }
  // scalar k of the sample is lane k's: its load goes out ahead of the rows', its store follows them
  double sv[GS_OPB_SAMPLES];
#pragma unroll
  for (int s = 0; s < GS_OPB_SAMPLES; ++s) {
    sv[s] = 0.0;
    if (!ok[s]) continue;
#pragma unroll
    for (int k = 0; k < GS_OPB_SCALARS; ++k)
      if (lane == k && G.sc_dst[k]) sv[s] = k == GS_OPB_SC_ADV ? G.stage[i[s]] : G.sc_src[k][j[s]];
  }
  const bool adv_normalised = G.sc_dst[GS_OPB_SC_ADV] && G.adv_norm != GS_OPB_NORM_NONE;
  const double adv_mean = adv_normalised ? G.adv_stats[0] : 0.0, adv_den = adv_normalised ? G.adv_stats[1] + G.adv_eps : 1.0;
  if (G.out_obs) {
    if (G.vec2) opb_rows<O, 2>(G, j, i, ok, lane);
    else opb_rows<O, 1>(G, j, i, ok, lane);
  }
#pragma unroll
  for (int s = 0; s < GS_OPB_SAMPLES; ++s) {
    if (!ok[s]) continue;
    if (G.out_act)
      for (int c = lane; c < G.A; c += 64) ((O*)G.out_act)[(size_t)i[s] * G.A + c] = (O)G.act[(size_t)j[s] * G.A + c];
#pragma unroll
    for (int k = 0; k < GS_OPB_SCALARS; ++k) {
      if (lane != k || !G.sc_dst[k]) continue;
      double v = sv[s];
      if (k == GS_OPB_SC_ADV && adv_normalised) { const double d = v - adv_mean; v = d / adv_den; }
      ((O*)G.sc_dst[k])[i[s]] = (O)v;
    }
  }
}

}  // namespace

extern "C" {

__global__ void __launch_bounds__(64 * GS_OPB_WAVES)
gs_k_opb_gather_f64(GsOpbGatherArgs G) { opb_gather<double>(G); }

__global__ void __launch_bounds__(64 * GS_OPB_WAVES)
gs_k_opb_gather_f32(GsOpbGatherArgs G) { opb_gather<float>(G); }

}  // extern "C"
