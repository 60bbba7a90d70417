// kernels_policy_f32.hip -- the MLP policy of gs_rollout(GS_POLICY_MLP) / gs_policy_mlp_eval at the precision of the reference's
// torch actors (GS_COMPUTE_F32, include/gridstep.h): float32 operands and float32 accumulation on v_mfma_f32_16x16x4_f32, the head
// in float64.  The float64 kernel (kernels_policy.hip) is the default and is not touched by this file.
//
// Mapping.  As there, a workgroup of four wavefronts owns GS_POL_ROWS = 32 instances (B = 8192: 256 workgroups, one per compute
// unit), wavefront w takes column tiles w, w + 4, w + 8, w + 12 for both row tiles: 8 independent accumulators of 4 floats (the
// instruction issues every 32 cycles and a dependent one waits 40, so consecutive products go to different accumulators).
// Operand maps: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15], one float per lane; C/D[row = 4 (lane >> 4) +
// reg][col = lane & 15] -- NOT the float64 instruction's row map.  One 16-byte operand per lane holds the four k-steps of a block
// of 16 (k = 16 kb + 4 (lane >> 4) + j); per block 2 LDS reads and 4 weight loads (1 KB contiguous per wavefront each, packed by
// the host: policy.h) feed 32 products, and the operands of the next block are loaded before the products of this one issue.
//
// The normalisation stage.  z = (obs - shift) * scale is computed in float64 on the raw observation and rounded to float32 once.
// The workgroup does that ONCE per element, into LDS (32 rows x 688 floats = 88 KB for the 123-bus feeder, beside 33 KB of
// activations), and all four wavefronts read the first layer's A operand from there like every other layer's: reading the tile
// from global memory in each wavefront, as the float64 kernel does, would repeat the float64 subtract / multiply / convert -- which
// runs at a quarter of the float32 rate -- four times, in the one loop that has to keep the matrix pipe fed.  An observation wider
// than GS_POL32_PANEL_KB blocks is staged in several panels behind one another, the accumulators carried across.
// Padded columns: zero weights and bias give act(0) = 0, and shift = scale = 0 beyond obs_dim give z = 0.
// The stage, the operand loads and the product loop live in mlp_f32.h, templated on the row tiles, where the value kernel
// (kernels_value.hip) shares them.  A sampling head with P.logp set also files the actions' log-probability terms in the
// observation tile's LDS, and one thread per instance adds them in action order (policy_head.h).
#include <hip/hip_runtime.h>
#include <math.h>

#include "env_device.h"
#include "mlp_f32.h"
#include "policy.h"
#include "policy_head.h"

namespace {

constexpr int GQ_RT = GS_POL_ROWS / 16;      // row tiles per workgroup

// component `comp` of the four normals of one Philox call (env_device.h's rng_normal_component), tag 'PNOI' (the float64 kernel's
// gp_noise, word for word: the stochastic contract of gs_policy_mlp is one contract)
__device__ __forceinline__ double gq_noise(uint64_t seed, uint64_t instance, uint32_t t, uint32_t quad, int comp) {
  const U4 r = philox((uint32_t)instance, t, quad, 0x504E4F49u, (uint32_t)seed, (uint32_t)(seed >> 32));
  return rng_normal_component(r, comp);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64 * GS_POL_WAVES)
gs_k_policy_mlp_f32(GsPolicyArgsF32 P) {
  extern __shared__ __attribute__((aligned(16))) float gq_lds[];
  float* const act_lds = gq_lds;                                           // [GS_POL_ROWS][GS_POL32_ACT_STRIDE]
  float* const obs_lds = gq_lds + GS_POL_ROWS * GS_POL32_ACT_STRIDE;       // [GS_POL_ROWS][P.obs_stride]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * GS_POL_ROWS;
  gq_v4 acc[GQ_RT][GQ_CT];
  for (int l = 0; l < P.n_layers; ++l) {
    const GsPolicyLayerF32 L = P.L[l];
    const bool full = L.nt == GQ_CT * GS_POL_WAVES;
#pragma unroll
    for (int rt = 0; rt < GQ_RT; ++rt)
#pragma unroll
      for (int c = 0; c < GQ_CT; ++c) acc[rt][c] = gq_v4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* in[GQ_RT];
    if (l == 0) {
#pragma unroll
      for (int rt = 0; rt < GQ_RT; ++rt) in[rt] = obs_lds + (16 * rt + (lane & 15)) * P.obs_stride + 4 * (lane >> 4);
      for (int kb0 = 0; kb0 < L.kb; kb0 += GS_POL32_PANEL_KB) {
        const int kb1 = min(kb0 + GS_POL32_PANEL_KB, L.kb);
        if (kb0) __syncthreads();            // every wavefront has read the previous panel
        if (P.D & 1) gq_stage<GS_POL_ROWS, false>(P.obs, P.shift, P.scale, P.D, P.B, P.obs_stride, obs_lds, row0, kb0, kb1, wave, lane);
        else gq_stage<GS_POL_ROWS, true>(P.obs, P.shift, P.scale, P.D, P.B, P.obs_stride, obs_lds, row0, kb0, kb1, wave, lane);
        __syncthreads();
        if (full) gq_layer<GQ_RT, true>(acc, in, L, kb0, kb1, wave, lane);
        else gq_layer<GQ_RT, false>(acc, in, L, kb0, kb1, wave, lane);
      }
    } else {
#pragma unroll
      for (int rt = 0; rt < GQ_RT; ++rt) in[rt] = act_lds + (16 * rt + (lane & 15)) * GS_POL32_ACT_STRIDE + 4 * (lane >> 4);
      if (full) gq_layer<GQ_RT, true>(acc, in, L, 0, L.kb, wave, lane);
      else gq_layer<GQ_RT, false>(acc, in, L, 0, L.kb, wave, lane);
    }
    __syncthreads();                         // every wavefront has read the previous activations
    const bool last = l == P.n_layers - 1;
#pragma unroll
    for (int c = 0; c < GQ_CT; ++c) {
      const int tile = wave + GS_POL_WAVES * c;
      if (tile >= L.nt) continue;
      const int col = 16 * tile + (lane & 15);
      const float bias = L.b[col];
#pragma unroll
      for (int rt = 0; rt < GQ_RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = acc[rt][c][r] + bias;
          act_lds[(16 * rt + 4 * (lane >> 4) + r) * GS_POL32_ACT_STRIDE + col] = last ? v : gq_activation(v, P.activation);
        }
    }
    __syncthreads();
  }
  // head, in float64 on the float32 pre-head values: a = tanh(mean) or tanh(mean + exp(clamp(log_std, -20, 2)) eps); with P.logp
  // the sampled action's log-probability term as well, into the observation tile's LDS (no wavefront reads that any more)
  const bool sample = P.head == GS_HEAD_GAUSSIAN_TANH && P.stochastic;
  double* const terms = (double*)obs_lds;                                  // [GS_POL_ROWS][P.A]
  for (int idx = threadIdx.x; idx < GS_POL_ROWS * P.A; idx += blockDim.x) {
    const int r = idx / P.A, a = idx - r * P.A, b = row0 + r;
    if (b >= P.B) break;
    double x = (double)act_lds[r * GS_POL32_ACT_STRIDE + a];
    if (sample) {
      const double ls = fmin(fmax((double)act_lds[r * GS_POL32_ACT_STRIDE + P.A + a], -20.0), 2.0);
      const double eps = gq_noise(P.seed, (uint64_t)(P.first_instance + b), (uint32_t)P.t, (uint32_t)(a >> 2), a & 3);
      x += exp(ls) * eps;
      const double act = tanh(x);
      P.act[(size_t)b * P.A + a] = act;
      if (P.logp) terms[idx] = gs_logp_term(eps, ls, act);
    } else {
      P.act[(size_t)b * P.A + a] = tanh(x);
    }
  }
  if (sample && P.logp) gs_logp_rows<GS_POL_ROWS>(terms, P.A, P.A, row0, P.B, P.logp);
}
