// kernels_q.hip -- state-action critics over the last rollout (include/gridstep.h "state-action critics"):
//   gs_k_q_mlp_f32   a Q network (GS_HEAD_LINEAR, float32 layers) on the rows (obs_seq[t][b], actions[t][b])
//   gs_k_q_combine   the minimum over the twins and q_adv = min(Q1, Q2) - V
//   gs_k_q_td        the one-step TD target r' + gamma * vnext
//   gs_k_q_gather    the Q learner's input rows and targets, and the Q-based signals of the policy's and the critic's heads
//   gs_k_q_polyak    the target networks' soft update
//
// gs_k_q_mlp_f32 has the structure of gs_k_value_mlp_f32 (kernels_value.hip): a workgroup of four wavefronts owns GS_VAL_ROWS = 64
// rows in four row tiles, the input tile is staged in panels of at most GS_VAL_PANEL_KB blocks with the accumulators carried across,
// the hidden layers run on v_mfma_f32_16x16x4_f32 (gq_layer, mlp_f32.h) and the last layer (width 1) is a dot product, four lanes a
// row.  Only the stage differs: a row's input comes from TWO matrices.  Column k < D is obs[row][k], normalised in float64 and
// rounded once; column D <= k < D + A is the stored float64 action act[row][k - D] rounded once (the host's normalisation image
// holds shift 0 and scale 1 there, and (a - 0) * 1 is a); the rest is 0.  A lane stages two adjacent columns, so with D odd (the
// 13-bus feeder: 71 + 4) one lane's pair straddles the two matrices, and with D + A odd the last pair straddles the padding: every
// column picks its source by itself.  A row's value depends on that row and the image alone: every sum runs over k in an order
// fixed by the layer's shape, whatever the row's place in its tile and whatever the launch.
// The small kernels take one thread per element or sample; where include/gridstep.h states a formula nothing is contracted.
#include <hip/hip_runtime.h>
#include <math.h>

#include "mlp_f32.h"
#include "q.h"

namespace {

constexpr int GQA_RT = GS_VAL_ROWS / 16;     // row tiles per workgroup
static_assert(64 * GS_POL_WAVES == 4 * GS_VAL_ROWS, "the dot product of the last layer: four lanes per row");

// columns [16 kb0, 16 kb1) of the workgroup's 64 input rows into `tile` (row stride `stride`), float64 rounded once.  Wavefront w
// takes rows 16 w .. 16 w + 15 (clamped to `nrows`), eight rows at a time, a lane two adjacent columns.
// EVEN: D is even, so a pair that starts below D - 1 lies in the observation at a 16-byte aligned address
template <bool EVEN>
__device__ __forceinline__ void gqa_stage(const double* __restrict__ obs, const double* __restrict__ act, const double* __restrict__ shift,
                                          const double* __restrict__ scale, int D, int A, int nrows, int stride, float* tile, int row0, int kb0,
                                          int kb1, int wave, int lane) {
  constexpr int SR = GS_VAL_ROWS / GS_POL_WAVES, G = 8;
  static_assert(SR % G == 0, "a wavefront stages whole groups of eight rows");
  const int width = 16 * (kb1 - kb0), DA = D + A;
#pragma unroll 1
  for (int g = SR * wave; g < SR * wave + SR; g += G) {
    const double* so[G];
    const double* sa[G];
#pragma unroll
    for (int r = 0; r < G; ++r) {
      const size_t row = (size_t)min(row0 + g + r, nrows - 1);
      so[r] = obs + row * D; sa[r] = act + row * A;
    }
    for (int c = 2 * lane; c < width; c += 128) {
      const int k = 16 * kb0 + c;            // even, and below the padded width of shift / scale
      const gq_d2 sh = *(const gq_d2*)(shift + k), sc = *(const gq_d2*)(scale + k);
      gq_d2 v[G];
      if (k + 1 < D) {                       // both columns are the observation's
#pragma unroll
        for (int r = 0; r < G; ++r) {
          if (EVEN) v[r] = *(const gq_d2*)(so[r] + k);
          else v[r] = gq_d2{so[r][k], so[r][k + 1]};
        }
      } else {                               // the last observation column, the actions, the padding: k + 1 >= D
#pragma unroll
        for (int r = 0; r < G; ++r) {
          double a = 0.0, b = 0.0;
          if (k < D) a = so[r][k];
          else if (k < DA) a = sa[r][k - D];
          if (k + 1 < DA) b = sa[r][k + 1 - D];
          v[r] = gq_d2{a, b};
        }
      }
#pragma unroll
      for (int r = 0; r < G; ++r)
        *(gq_v2*)(tile + (g + r) * stride + c) = gq_v2{(float)((v[r][0] - sh[0]) * sc[0]), (float)((v[r][1] - sh[1]) * sc[1])};
    }
  }
}

// this lane's share of  in_row[16 kb0 .. 16 kb1) . W[0][the same]: columns 16 kb + 4 q + j of every block onto p[j], j = 0 .. 3
// (the order of the value kernel's last layer)
__device__ __forceinline__ void gqa_dot(gq_v4& p, const float* in_row, int kbase, const float* __restrict__ wl, int kb0, int kb1, int q) {
  for (int kb = kb0; kb < kb1; ++kb) {
    const gq_v4 x = *(const gq_v4*)(in_row + 16 * (kb - kbase) + 4 * q);
    const gq_v4 w = *(const gq_v4*)(wl + ((size_t)kb * 64 + 16 * q) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = fmaf(x[j], w[j], p[j]);
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64 * GS_POL_WAVES)
gs_k_q_mlp_f32(GsQArgs P) {
  extern __shared__ __attribute__((aligned(16))) float gqa_lds[];
  float* const act_lds = gqa_lds;                                          // [GS_VAL_ROWS][GS_POL32_ACT_STRIDE]
  float* const in_lds = gqa_lds + GS_VAL_ROWS * GS_POL32_ACT_STRIDE;       // [GS_VAL_ROWS][P.obs_stride]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * GS_VAL_ROWS;
  const int rows = P.rows;
  if (row0 >= rows) return;
  const int drow = threadIdx.x >> 2, dq = threadIdx.x & 3;                 // the last layer: this lane's row and quarter
  const int last = P.n_layers - 1;
  gq_v4 part4 = gq_v4{0.0f, 0.0f, 0.0f, 0.0f};
  gq_v4 acc[GQA_RT][GQ_CT];
  for (int l = 0; l < P.n_layers; ++l) {
    const GsPolicyLayerF32 L = P.L[l];
    const bool full = L.nt == GQ_CT * GS_POL_WAVES;
#pragma unroll
    for (int rt = 0; rt < GQA_RT; ++rt)
#pragma unroll
      for (int c = 0; c < GQ_CT; ++c) acc[rt][c] = gq_v4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* in[GQA_RT];
    if (l == 0) {
#pragma unroll
      for (int rt = 0; rt < GQA_RT; ++rt) in[rt] = in_lds + (16 * rt + (lane & 15)) * P.obs_stride + 4 * (lane >> 4);
      for (int kb0 = 0; kb0 < L.kb; kb0 += P.panel_kb) {
        const int kb1 = min(kb0 + P.panel_kb, L.kb);
        if (kb0) __syncthreads();            // every wavefront has read the previous panel
        if (P.D & 1) gqa_stage<false>(P.obs, P.act, P.shift, P.scale, P.D, P.A, rows, P.obs_stride, in_lds, row0, kb0, kb1, wave, lane);
        else gqa_stage<true>(P.obs, P.act, P.shift, P.scale, P.D, P.A, rows, P.obs_stride, in_lds, row0, kb0, kb1, wave, lane);
        __syncthreads();
        if (last == 0) gqa_dot(part4, in_lds + drow * P.obs_stride, kb0, L.w, kb0, kb1, dq);
        else if (full) gq_layer<GQA_RT, true>(acc, in, L, kb0, kb1, wave, lane);
        else gq_layer<GQA_RT, false>(acc, in, L, kb0, kb1, wave, lane);
      }
    } else if (l == last) {
      gqa_dot(part4, act_lds + drow * GS_POL32_ACT_STRIDE, 0, L.w, 0, L.kb, dq);
    } else {
#pragma unroll
      for (int rt = 0; rt < GQA_RT; ++rt) in[rt] = act_lds + (16 * rt + (lane & 15)) * GS_POL32_ACT_STRIDE + 4 * (lane >> 4);
      if (full) gq_layer<GQA_RT, true>(acc, in, L, 0, L.kb, wave, lane);
      else gq_layer<GQA_RT, false>(acc, in, L, 0, L.kb, wave, lane);
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
      for (int rt = 0; rt < GQA_RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          act_lds[(16 * rt + 4 * (lane >> 4) + r) * GS_POL32_ACT_STRIDE + col] = gq_activation(acc[rt][c][r] + bias, P.activation);
    }
    __syncthreads();
  }
  // this lane's four sums as (s0 + s1) + (s2 + s3), the four lanes' the same way in every one of them, the bias, and the widening
  float part = (part4[0] + part4[1]) + (part4[2] + part4[3]);
  part += __shfl_xor(part, 1);
  part += __shfl_xor(part, 2);
  const int row = row0 + drow;
  if (dq == 0 && row < rows) P.out[row] = (double)(part + P.L[last].b[0]);
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_q_combine(GsQCombineArgs C) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C.n) return;
  double m[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const double* a = C.q[s][0];
    const double* b = C.q[s][1];
    m[s] = a && b ? fmin(a[i], b[i]) : a ? a[i] : b[i];
    C.q_min[s][i] = m[s];
  }
  C.q_adv[i] = m[0] - C.values[i];
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_q_td(GsQTdArgs G) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  size_t i;
  double vnext;
  if (G.phase == 0) {
    if (e >= (long long)G.T * G.B) return;
    i = (size_t)e;
    vnext = G.done[i] ? 0.0 : G.values[i + G.B];
  } else {
    if (e >= min(*G.term_count, G.term_cap)) return;
    const int t = G.term_idx[2 * e], b = G.term_idx[2 * e + 1];
    if ((unsigned)t >= (unsigned)G.T || (unsigned)b >= (unsigned)G.B) return;
    i = (size_t)t * G.B + b;
    if (!(G.done[i] & G.mask)) return;       // (phase 0 wrote this transition's target)
    vnext = G.term_values[e];
  }
  const double r = (G.rew[i] - G.reward_shift) * G.reward_scale;
  G.td[i] = r + G.gamma * vnext;
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_q_gather(GsQGatherArgs G) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int W = G.DA > 0 ? G.DA : 1;
  if (e >= (long long)G.n * W) return;
  const int i = (int)(e / W), k = (int)(e - (long long)i * W);
  long long j = G.idx[i];
  j = j < 0 ? 0 : (j >= G.N ? G.N - 1 : j);  // (an index the minibatch did not write cannot leave the rollout)
  if (k == 0) G.y[i] = (float)G.src[j];
  if (G.DA > 0) G.sa[e] = k < G.D ? G.obs[(size_t)i * G.D + k] : (float)G.act[(size_t)j * (G.DA - G.D) + (k - G.D)];
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_q_polyak(GsQPolyakArgs A) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  A.t[i] = (A.tau * A.p[i]) + (A.omt * A.t[i]);
}
