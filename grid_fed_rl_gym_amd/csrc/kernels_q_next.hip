// kernels_q_next.hip -- policy-action TD targets over the last rollout (include/gridstep.h "policy-action TD targets"; DESIGN.md
// section 25):
//   gs_k_policy_rows_f32   the installed float32 tanh-Gaussian policy over any number of rows of float64 observations: the pre-head
//                          values, the noise, the sampled (or the deterministic) action and its log-probability
//   gs_k_q_next_td         the minimum over the target twins and r' + gamma (min Q_target(s', a') - alpha log pi(a' | s'))
//
// gs_k_policy_rows_f32 has the value kernel's tile (kernels_value.hip): a workgroup of four wavefronts owns GS_VAL_ROWS = 64 rows in
// four row tiles, the observation tile is staged by gq_stage in panels of at most P.panel_kb blocks with the accumulators carried
// across, and EVERY layer -- the last one too, 2 A columns padded to whole tiles -- runs through gq_layer on
// v_mfma_f32_16x16x4_f32.  The layer table is the policy's installed one, the image Adam rewrites.  The last layer leaves mean |
// log_std in the activation tile; the head is gs_k_pw_sample's (kernels_pathwise.hip), operation for operation in float64 on those
// float32 values, one thread per (row, action), its log-probability terms filed in the observation panel's LDS (no wavefront reads
// that any more) and added per row in ONE chain from k = 0.  A row's outputs depend on that row, the image, seed, draw and the
// row's noise index alone; the order of every sum is a function of the layer shapes.
#include <hip/hip_runtime.h>
#include <math.h>

#include "bootstrap.h"
#include "env_device.h"
#include "gw_math.h"
#include "mlp_f32.h"
#include "q_next.h"

namespace {

// component `comp` of the four normals of one Philox call (env_device.h's rng_normal_component), counter (index, quad, draw, tag)
__device__ __forceinline__ double gn_noise(uint64_t seed, uint32_t index, uint32_t quad, uint32_t draw, uint32_t tag, int comp) {
  const U4 r = philox(index, quad, draw, tag, (uint32_t)seed, (uint32_t)(seed >> 32));
  return rng_normal_component(r, comp);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64 * GS_POL_WAVES)
gs_k_policy_rows_f32(GsPolicyRowsArgs P) {
  constexpr int RT = GS_VAL_ROWS / 16;       // row tiles per workgroup
  float* const act_lds = gq_net_lds;                                       // [GS_VAL_ROWS][GS_POL32_ACT_STRIDE]
  float* const in_lds = gq_net_lds + GS_VAL_ROWS * GS_POL32_ACT_STRIDE;    // [GS_VAL_ROWS][P.obs_stride]; then the head's terms
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * GS_VAL_ROWS;
  const int rows = P.rows_dev ? min(*P.rows_dev, P.rows) : P.rows;
  if (row0 >= rows) return;                  // (the whole workgroup)
  const int last = P.n_layers - 1;
  gq_v4 acc[RT][GQ_CT];
  for (int l = 0; l < P.n_layers; ++l) {
    const GsPolicyLayerF32 L = P.L[l];
    const bool full = L.nt == GQ_CT * GS_POL_WAVES;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int c = 0; c < GQ_CT; ++c) acc[rt][c] = gq_v4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* in[RT];
    if (l == 0) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) in[rt] = in_lds + (16 * rt + (lane & 15)) * P.obs_stride + 4 * (lane >> 4);
      for (int kb0 = 0; kb0 < L.kb; kb0 += P.panel_kb) {
        const int kb1 = min(kb0 + P.panel_kb, L.kb);
        if (kb0) __syncthreads();            // every wavefront has read the previous panel
        if (P.D & 1) gq_stage<GS_VAL_ROWS, false>(P.obs, P.shift, P.scale, P.D, rows, P.obs_stride, in_lds, row0, kb0, kb1, wave, lane);
        else gq_stage<GS_VAL_ROWS, true>(P.obs, P.shift, P.scale, P.D, rows, P.obs_stride, in_lds, row0, kb0, kb1, wave, lane);
        __syncthreads();
        if (full) gq_layer<RT, true>(acc, in, L, kb0, kb1, wave, lane);
        else gq_layer<RT, false>(acc, in, L, kb0, kb1, wave, lane);
      }
    } else {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) in[rt] = act_lds + (16 * rt + (lane & 15)) * GS_POL32_ACT_STRIDE + 4 * (lane >> 4);
      if (full) gq_layer<RT, true>(acc, in, L, 0, L.kb, wave, lane);
      else gq_layer<RT, false>(acc, in, L, 0, L.kb, wave, lane);
    }
    __syncthreads();                         // every wavefront has read the previous activations
#pragma unroll
    for (int c = 0; c < GQ_CT; ++c) {
      const int tile = wave + GS_POL_WAVES * c;
      if (tile >= L.nt) continue;
      const int col = 16 * tile + (lane & 15);
      const float bias = L.b[col];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = acc[rt][c][r] + bias;
          act_lds[(16 * rt + 4 * (lane >> 4) + r) * GS_POL32_ACT_STRIDE + col] = l == last ? v : gq_activation(v, P.activation);
        }
    }
    __syncthreads();
  }
  // the head of gs_k_pw_sample, one thread per (row, action)
  {
#pragma clang fp contract(off)
    const int A = P.A, TS = A | 1;           // (gs_qn_term_stride)
    double* const terms = (double*)in_lds;   // [GS_VAL_ROWS][TS]
    for (int e = threadIdx.x; e < GS_VAL_ROWS * A; e += blockDim.x) {
      const int r = e / A, k = e - r * A, row = row0 + r;
      if (row >= rows) break;
      const float m32 = act_lds[r * GS_POL32_ACT_STRIDE + k], l32 = act_lds[r * GS_POL32_ACT_STRIDE + A + k];
      P.pre_head[(size_t)row * (2 * A) + k] = m32;
      P.pre_head[(size_t)row * (2 * A) + A + k] = l32;
      const uint32_t index = P.idx ? (uint32_t)(P.idx[2 * row] * P.B + P.idx[2 * row + 1]) : (uint32_t)row;
      const double mean = (double)m32;
      const double ls = fmin(fmax((double)l32, -20.0), 2.0);
      const double eps = P.stochastic ? gn_noise(P.seed, index, (uint32_t)(k >> 2), P.draw, P.tag, k & 3) : 0.0;
      const double x = mean + gw_exp(ls) * eps;
      const double a = gw_tanh(x);
      P.act[(size_t)row * A + k] = a;
      P.noise[(size_t)row * A + k] = eps;
      terms[r * TS + k] = gw_logp_term(eps, ls, a);
    }
    __syncthreads();
    const int r = threadIdx.x;
    if (r < GS_VAL_ROWS && row0 + r < rows) {
      double lp = terms[r * TS];
      for (int k = 1; k < A; ++k) lp = lp + terms[r * TS + k];
      P.logp[row0 + r] = lp;
    }
  }
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_q_next_td(GsQNextTdArgs G) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  size_t i;
  double vnext;
  if (G.phase == 0) {
    if (e >= (long long)G.T * G.B) return;
    i = (size_t)e;
    const double m = gb_twin_min(G.q[0], G.q[1], i);
    G.q_min[i] = m;
    const double v = gb_soft_value(m, G.alpha, G.lp[i]);
    vnext = G.done[i] ? 0.0 : v;
  } else {
    if (e >= min(*G.term_count, G.term_cap)) return;
    const double m = gb_twin_min(G.term_q[0], G.term_q[1], (size_t)e);
    G.term_q_min[e] = m;
    vnext = gb_soft_value(m, G.alpha, G.term_lp[e]);
    G.term_value[e] = vnext;
    const int t = G.term_idx[2 * e], b = G.term_idx[2 * e + 1];
    if ((unsigned)t >= (unsigned)G.T || (unsigned)b >= (unsigned)G.B) return;
    i = (size_t)t * G.B + b;
    if (!(G.done[i] & G.mask)) return;       // (phase 0 wrote this transition's target)
  }
  G.td[i] = gb_td(G.rew[i], G.reward_shift, G.reward_scale, G.gamma, vnext);
}
