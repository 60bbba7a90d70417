// mlp_f32.h -- device functions the float32 MLP kernels share (gs_k_policy_mlp_f32, kernels_policy_f32.hip; gs_k_value_mlp_f32,
// kernels_value.hip; gs_k_q_mlp_f32, kernels_q.hip; the three matrix kernels of kernels_train.hip): the float64 normalisation stage
// into LDS, the operand loads and the product loop of one layer on v_mfma_f32_16x16x4_f32, the hidden activation, the dot product
// of a last layer of width 1, and gq_scalar_net, the whole body of the value and the Q kernel.  Operand maps and the weight layout:
// kernels_policy_f32.hip, policy.h.
// Templated on the row tiles of the workgroup (RT = rows / 16): 2 for the policy and the training kernels, 4 for the value and the Q
// kernel; everything else (four wavefronts, four column tiles per wavefront, k blocks of 16) is common.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "policy.h"

typedef float gq_v4 __attribute__((ext_vector_type(4)));
typedef float gq_v2 __attribute__((ext_vector_type(2)));
typedef double gq_d2 __attribute__((ext_vector_type(2)));

// the dynamic LDS of a kernel whose body is gq_scalar_net: activations, then the staged input panel
extern __shared__ __attribute__((aligned(16))) float gq_net_lds[];

namespace {

constexpr int GQ_CT = 4;                     // column tiles per wavefront
static_assert(GQ_CT * GS_POL_WAVES * 16 >= GS_POL_MAX_WIDTH, "every column tile of the widest layer has a wavefront");

// z = (obs - shift) * scale, float64, rounded once; columns [16 kb0, 16 kb1) of the workgroup's ROWS rows into `tile` (row stride
// `stride`).  Wavefront w takes rows SR w .. SR w + SR - 1, SR = ROWS / 4 (rows clamped to `nrows`), eight rows at a time, a lane two
// adjacent columns.
template <int ROWS, bool EVEN>
__device__ __forceinline__ void gq_stage(const double* __restrict__ obs, const double* __restrict__ shift, const double* __restrict__ scale, int D,
                                         int nrows, int stride, float* tile, int row0, int kb0, int kb1, int wave, int lane) {
  constexpr int SR = ROWS / GS_POL_WAVES, G = 8;
  static_assert(SR % G == 0, "a wavefront stages whole groups of eight rows");
  const int width = 16 * (kb1 - kb0);
#pragma unroll 1
  for (int g = SR * wave; g < SR * wave + SR; g += G) {
    const double* src[G];
#pragma unroll
    for (int r = 0; r < G; ++r) src[r] = obs + (size_t)min(row0 + g + r, nrows - 1) * D;
    for (int c = 2 * lane; c < width; c += 128) {
      const int k = 16 * kb0 + c;            // even, and below the padded width of shift / scale
      const gq_d2 sh = *(const gq_d2*)(shift + k), sc = *(const gq_d2*)(scale + k);
      gq_d2 v[G];
#pragma unroll
      for (int r = 0; r < G; ++r) {
        if (EVEN) {      // D even: k < D means k + 1 < D, and the address is 16-byte aligned
          v[r] = *(const gq_d2*)(src[r] + min(k, D - 2));
        } else {
          v[r] = gq_d2{src[r][min(k, D - 1)], src[r][min(k + 1, D - 1)]};
        }
      }
#pragma unroll
      for (int r = 0; r < G; ++r) {
        const double a = k < D ? v[r][0] : 0.0, b = k + 1 < D ? v[r][1] : 0.0;
        *(gq_v2*)(tile + (g + r) * stride + c) = gq_v2{(float)((a - sh[0]) * sc[0]), (float)((b - sh[1]) * sc[1])};
      }
    }
  }
}

template <int RT>
struct GqFrag { gq_v4 x[RT], w[GQ_CT]; };

// in[rt]: this lane's operand of block `kbase` (row 16 rt + (lane & 15), columns 4 (lane >> 4) ..) in LDS
template <int RT, bool FULL>
__device__ __forceinline__ void gq_load(GqFrag<RT>& f, const float* const (&in)[RT], int kbase, const float* __restrict__ wl, int kb_total, int kb, int nt,
                                        int wave, int lane) {
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) f.x[rt] = *(const gq_v4*)(in[rt] + 16 * (kb - kbase));
#pragma unroll
  for (int c = 0; c < GQ_CT; ++c) {
    const int tile = wave + GS_POL_WAVES * c;
    if (FULL || tile < nt) f.w[c] = *(const gq_v4*)(wl + (((size_t)tile * kb_total + kb) * 64 + lane) * 4);
  }
}

// acc[rt][c] += in[rows of tile rt][16 kb0 .. 16 kb1) W[columns of tile wave + 4 c][the same]^T
// FULL: the layer has all sixteen column tiles, so every wavefront has its four (no predicates in the loop)
template <int RT, bool FULL>
__device__ __forceinline__ void gq_layer(gq_v4 (&acc)[RT][GQ_CT], const float* const (&in)[RT], const GsPolicyLayerF32& L, int kb0, int kb1,
                                         int wave, int lane) {
  if (!FULL && wave >= L.nt) return;         // (a narrow layer: this wavefront has no column tile)
  GqFrag<RT> cur, nxt;
  gq_load<RT, FULL>(cur, in, kb0, L.w, L.kb, kb0, L.nt, wave, lane);
  for (int kb = kb0; kb < kb1; ++kb) {
    if (kb + 1 < kb1) gq_load<RT, FULL>(nxt, in, kb0, L.w, L.kb, kb + 1, L.nt, wave, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < GQ_CT; ++c) {
        if (!FULL && wave + GS_POL_WAVES * c >= L.nt) continue;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.x[rt][j], cur.w[c][j], acc[rt][c], 0, 0, 0);
      }
    cur = nxt;
  }
}

// The last layer of a scalar-output network (width 1) as a dot product, four lanes a row: lane q's share of
// in_row[16 kb0 .. 16 kb1) . W[0][the same], columns 16 kb + 4 q + j of every block onto p[j], j = 0 .. 3, one fmaf chain in
// ascending k per j.  in_row: the row's columns from block `kbase` on, in LDS; wl: the layer's packed image, whose row 0 lies at
// lanes 0, 16, 32, 48 of every block.
__device__ __forceinline__ void gq_dot(gq_v4& p, const float* in_row, int kbase, const float* __restrict__ wl, int kb0, int kb1, int q) {
  for (int kb = kb0; kb < kb1; ++kb) {
    const gq_v4 x = *(const gq_v4*)(in_row + 16 * (kb - kbase) + 4 * q);
    const gq_v4 w = *(const gq_v4*)(wl + ((size_t)kb * 64 + 16 * q) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = fmaf(x[j], w[j], p[j]);
  }
}

__device__ __forceinline__ float gq_activation(float x, int kind) {
  if (kind == GS_ACT_RELU) return x > 0.0f ? x : 0.0f;
  if (kind == GS_ACT_TANH) return tanhf(x);
  return x > 0.0f ? x : expm1f(x);           // elu, alpha = 1
}

// ---- a network with a scalar output (GS_HEAD_LINEAR) over any number of rows: the whole body of gs_k_value_mlp_f32 (kernels_value.hip)
// and of gs_k_q_mlp_f32 (kernels_q.hip).  A workgroup of four wavefronts owns GS_VAL_ROWS rows in four row tiles; the input tile is
// staged into LDS in panels of at most P.panel_kb blocks, the accumulators carried across; hidden layers are gq_layer, the last
// layer is gq_dot.  P: GsValueArgs or GsQArgs (rows, D, n_layers, activation, obs_stride, panel_kb, L[]).  rows_dev: NULL, or the
// device word that holds how many of P.rows rows are there.  What the two kernels do not share comes as the static members of Net:
// stage<EVEN>(P, tile, rows, row0, kb0, kb1, wave, lane) fills columns [16 kb0, 16 kb1) of the workgroup's rows (EVEN: P.D is even),
// store(P, row, v) keeps a row's value.
// (P is __restrict__: the kernel's argument block is read through a reference here, and without the promise that no store reaches
// it the loads of P.D, P.obs_stride, ... are not hoisted out of the layer loop as they are when the kernel reads P itself.)
static_assert(64 * GS_POL_WAVES == 4 * GS_VAL_ROWS, "the dot product of the last layer: four lanes per row");

template <typename Net, typename Args>
__device__ __forceinline__ void gq_scalar_net(const Args& __restrict__ P, const int32_t* rows_dev) {
  constexpr int RT = GS_VAL_ROWS / 16;       // row tiles per workgroup
  float* const act_lds = gq_net_lds;                                       // [GS_VAL_ROWS][GS_POL32_ACT_STRIDE]
  float* const in_lds = gq_net_lds + GS_VAL_ROWS * GS_POL32_ACT_STRIDE;    // [GS_VAL_ROWS][P.obs_stride]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * GS_VAL_ROWS;
  const int rows = rows_dev ? min(*rows_dev, P.rows) : P.rows;
  if (row0 >= rows) return;                  // (the whole workgroup)
  const int drow = threadIdx.x >> 2, dq = threadIdx.x & 3;                 // the last layer: this lane's row and quarter
  const int last = P.n_layers - 1;
  gq_v4 part4 = gq_v4{0.0f, 0.0f, 0.0f, 0.0f};
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
        if (P.D & 1) Net::template stage<false>(P, in_lds, rows, row0, kb0, kb1, wave, lane);
        else Net::template stage<true>(P, in_lds, rows, row0, kb0, kb1, wave, lane);
        __syncthreads();
        if (last == 0) gq_dot(part4, in_lds + drow * P.obs_stride, kb0, L.w, kb0, kb1, dq);
        else if (full) gq_layer<RT, true>(acc, in, L, kb0, kb1, wave, lane);
        else gq_layer<RT, false>(acc, in, L, kb0, kb1, wave, lane);
      }
    } else if (l == last) {
      gq_dot(part4, act_lds + drow * GS_POL32_ACT_STRIDE, 0, L.w, 0, L.kb, dq);
    } else {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) in[rt] = act_lds + (16 * rt + (lane & 15)) * GS_POL32_ACT_STRIDE + 4 * (lane >> 4);
      if (full) gq_layer<RT, true>(acc, in, L, 0, L.kb, wave, lane);
      else gq_layer<RT, false>(acc, in, L, 0, L.kb, wave, lane);
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
      for (int rt = 0; rt < RT; ++rt)
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
  if (dq == 0 && row < rows) Net::store(P, row, (double)(part + P.L[last].b[0]));
}

}  // namespace
