// kernels_value.hip -- the value network of gs_value_mlp_set (include/gridstep.h; GS_HEAD_LINEAR, float32 layers) over a row-major
// [rows][obs_dim] float64 matrix: gs_k_value_mlp_f32; and the advantages of the last rollout: gs_k_gae.
//
// gs_k_value_mlp_f32.  The layers of gs_k_policy_mlp_f32 (mlp_f32.h: float64 normalisation rounded once into LDS, hidden layers on
// v_mfma_f32_16x16x4_f32, float32 activations) with another tile: a workgroup of four wavefronts owns GS_VAL_ROWS = 64 rows, four
// row tiles.  The policy kernel's 32 rows were chosen so that B = 8192 fills 256 compute units once; this kernel runs over half a
// million rows, every compute unit is busy at any tile, and what counts is the weight traffic: a wavefront's four weight operands
// of a k block now feed 64 products instead of 32 (16 accumulators of 4 floats), so the matrices are read from L2 half as often.
// A 64-row observation tile of the 123-bus feeder (64 x 692 floats) does not fit beside the activations, so the observation is
// staged in panels of at most GS_VAL_PANEL_KB blocks, the accumulators carried across (policy.h).
// The last layer (width 1) is a dot product: four lanes per row, lane q taking the k with (k >> 2) & 3 = q, one fmaf chain in
// ascending order per k & 3 (sixteen sums a row, each a sixteenth of the terms: 43 at obs_dim 684), added pairwise -- a padded 16-column tile would spend a hidden layer's quarter on
// fifteen columns of zeros in one wavefront while three wait.  Its weights are read from the packed image where the tile's row 0
// lies (lanes 0, 16, 32, 48 of every block).  A row's value depends on that row alone: every sum runs over k in an order fixed by
// the layer's shape, whatever the row's place in its tile and whatever the launch.
#include <hip/hip_runtime.h>
#include <math.h>

#include "mlp_f32.h"
#include "policy.h"

namespace {

constexpr int GV_RT = GS_VAL_ROWS / 16;      // row tiles per workgroup
static_assert(64 * GS_POL_WAVES == 4 * GS_VAL_ROWS, "the dot product of the last layer: four lanes per row");

// this lane's share of  in_row[16 kb0 .. 16 kb1) . W[0][the same]: columns 16 kb + 4 q + j of every block onto p[j], j = 0 .. 3
__device__ __forceinline__ void gv_dot(gq_v4& p, const float* in_row, int kbase, const float* __restrict__ wl, int kb0, int kb1, int q) {
  for (int kb = kb0; kb < kb1; ++kb) {
    const gq_v4 x = *(const gq_v4*)(in_row + 16 * (kb - kbase) + 4 * q);
    const gq_v4 w = *(const gq_v4*)(wl + ((size_t)kb * 64 + 16 * q) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = fmaf(x[j], w[j], p[j]);
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64 * GS_POL_WAVES)
gs_k_value_mlp_f32(GsValueArgs P) {
  extern __shared__ __attribute__((aligned(16))) float gv_lds[];
  float* const act_lds = gv_lds;                                           // [GS_VAL_ROWS][GS_POL32_ACT_STRIDE]
  float* const obs_lds = gv_lds + GS_VAL_ROWS * GS_POL32_ACT_STRIDE;       // [GS_VAL_ROWS][P.obs_stride]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * GS_VAL_ROWS;
  const int rows = P.rows_dev ? min(*P.rows_dev, P.rows) : P.rows;
  if (row0 >= rows) return;                  // (the whole workgroup: the terminal list is launched over its capacity)
  const int drow = threadIdx.x >> 2, dq = threadIdx.x & 3;                 // the last layer: this lane's row and quarter
  const int last = P.n_layers - 1;
  gq_v4 part4 = gq_v4{0.0f, 0.0f, 0.0f, 0.0f};
  gq_v4 acc[GV_RT][GQ_CT];
  for (int l = 0; l < P.n_layers; ++l) {
    const GsPolicyLayerF32 L = P.L[l];
    const bool full = L.nt == GQ_CT * GS_POL_WAVES;
#pragma unroll
    for (int rt = 0; rt < GV_RT; ++rt)
#pragma unroll
      for (int c = 0; c < GQ_CT; ++c) acc[rt][c] = gq_v4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* in[GV_RT];
    if (l == 0) {
#pragma unroll
      for (int rt = 0; rt < GV_RT; ++rt) in[rt] = obs_lds + (16 * rt + (lane & 15)) * P.obs_stride + 4 * (lane >> 4);
      for (int kb0 = 0; kb0 < L.kb; kb0 += P.panel_kb) {
        const int kb1 = min(kb0 + P.panel_kb, L.kb);
        if (kb0) __syncthreads();            // every wavefront has read the previous panel
        if (P.D & 1) gq_stage<GS_VAL_ROWS, false>(P.obs, P.shift, P.scale, P.D, rows, P.obs_stride, obs_lds, row0, kb0, kb1, wave, lane);
        else gq_stage<GS_VAL_ROWS, true>(P.obs, P.shift, P.scale, P.D, rows, P.obs_stride, obs_lds, row0, kb0, kb1, wave, lane);
        __syncthreads();
        if (last == 0) gv_dot(part4, obs_lds + drow * P.obs_stride, kb0, L.w, kb0, kb1, dq);
        else if (full) gq_layer<GV_RT, true>(acc, in, L, kb0, kb1, wave, lane);
        else gq_layer<GV_RT, false>(acc, in, L, kb0, kb1, wave, lane);
      }
    } else if (l == last) {
      gv_dot(part4, act_lds + drow * GS_POL32_ACT_STRIDE, 0, L.w, 0, L.kb, dq);
    } else {
#pragma unroll
      for (int rt = 0; rt < GV_RT; ++rt) in[rt] = act_lds + (16 * rt + (lane & 15)) * GS_POL32_ACT_STRIDE + 4 * (lane >> 4);
      if (full) gq_layer<GV_RT, true>(acc, in, L, 0, L.kb, wave, lane);
      else gq_layer<GV_RT, false>(acc, in, L, 0, L.kb, wave, lane);
    }
    if (l == last) break;
    __syncthreads();                         // every wavefront has read the previous activations
#pragma unroll
    for (int c = 0; c < GQ_CT; ++c) {
      const int tile = wave + GS_POL_WAVES * c;
      if (tile >= L.nt) continue;
      const int col = 16 * tile + (lane & 15);
      const float bias = L.b[col];
#pragma unroll
      for (int rt = 0; rt < GV_RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          act_lds[(16 * rt + 4 * (lane >> 4) + r) * GS_POL32_ACT_STRIDE + col] = gq_activation(acc[rt][c][r] + bias, P.activation);
    }
    __syncthreads();
  }
  // this lane's four sums as (s0 + s1) + (s2 + s3), the four lanes' the same way in every one of them (the additions commute),
  // the bias, and the widening
  float part = (part4[0] + part4[1]) + (part4[2] + part4[3]);
  part += __shfl_xor(part, 1);
  part += __shfl_xor(part, 2);
  const int row = row0 + drow;
  if (dq == 0 && row < rows) {
    const double v = (double)(part + P.L[last].b[0]);
    P.out[row] = v;
    if (P.scatter_idx) {
      const int t = P.scatter_idx[2 * row], b = P.scatter_idx[2 * row + 1];
      if ((unsigned)t < (unsigned)P.scatter_T && (unsigned)b < (unsigned)P.scatter_B) P.scatter_out[(size_t)t * P.scatter_B + b] = v;
    }
  }
}

// ---- generalised advantage estimation over the last rollout ------------------------------------------------------------------------
// One thread per instance b, t from T - 1 down to 0; every array is [.][B], so a wavefront's accesses are contiguous.  The recurrence
// of include/gridstep.h, operation by operation (rollout.py's gae_np restates it): no contraction.
// ret[t][b] holds, on entry, the value of the terminal observation of every transition that ended an episode (gs_k_value_mlp_f32
// scattered it there); it is read before the return is written over it.
extern "C" __global__ void __launch_bounds__(256)
gs_k_gae(GsGaeArgs G) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= G.B) return;
  const double gl = G.gamma * G.lambda;
  double adv_next = 0.0;
  for (int t = G.T - 1; t >= 0; --t) {
    const size_t i = (size_t)t * G.B + b;
    const uint8_t flag = G.done[i];
    const bool done = flag != 0;
    const double v = G.values[i];
    const double vnext = done ? ((flag & G.mask) ? G.ret[i] : 0.0) : G.values[i + G.B];
    const double r = (G.rew[i] - G.reward_shift) * G.reward_scale;
    const double delta = (r + G.gamma * vnext) - v;
    const double adv = done ? delta : delta + gl * adv_next;
    G.adv[i] = adv;
    G.ret[i] = adv + v;
    adv_next = adv;
  }
}
