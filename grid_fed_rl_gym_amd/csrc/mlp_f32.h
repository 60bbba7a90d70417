// mlp_f32.h -- device functions the float32 MLP kernels share (gs_k_policy_mlp_f32, kernels_policy_f32.hip; gs_k_value_mlp_f32,
// kernels_value.hip): the float64 normalisation stage into LDS, the operand loads and the product loop of one layer on
// v_mfma_f32_16x16x4_f32, and the hidden activation.  Operand maps and the weight layout: kernels_policy_f32.hip, policy.h.
// Templated on the row tiles of the workgroup (RT = rows / 16): 2 for the policy kernel, 4 for the value kernel; everything else
// (four wavefronts, four column tiles per wavefront, k blocks of 16) is common.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "policy.h"

typedef float gq_v4 __attribute__((ext_vector_type(4)));
typedef float gq_v2 __attribute__((ext_vector_type(2)));
typedef double gq_d2 __attribute__((ext_vector_type(2)));

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

__device__ __forceinline__ float gq_activation(float x, int kind) {
  if (kind == GS_ACT_RELU) return x > 0.0f ? x : 0.0f;
  if (kind == GS_ACT_TANH) return tanhf(x);
  return x > 0.0f ? x : expm1f(x);           // elu, alpha = 1
}

}  // namespace
