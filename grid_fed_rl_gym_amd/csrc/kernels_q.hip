// kernels_q.hip -- state-action critics over the last rollout (include/gridstep.h "state-action critics"):
//   gs_k_q_mlp_f32   a Q network (GS_HEAD_LINEAR, float32 layers) on the rows (obs_seq[t][b], actions[t][b])
//   gs_k_q_mlp_rows_f32   the same body over a list whose length lies on the device
//   gs_k_q_combine   the minimum over the twins and q_adv = min(Q1, Q2) - V
//   gs_k_q_td        the one-step TD target r' + gamma * vnext
//   gs_k_q_gather    the Q learner's input rows and targets, and the Q-based signals of the policy's and the critic's heads
//   gs_k_q_polyak    the target networks' soft update
//
// gs_k_q_mlp_f32 has the body of gs_k_value_mlp_f32 (kernels_value.hip), gq_scalar_net of mlp_f32.h: a workgroup of four wavefronts
// owns GS_VAL_ROWS = 64 rows in four row tiles, the input tile is staged in panels of at most GS_VAL_PANEL_KB blocks with the
// accumulators carried across, the hidden layers run on v_mfma_f32_16x16x4_f32 (gq_layer) and the last layer (width 1) is a dot
// product, four lanes a row (gq_dot).  Only the stage differs: a row's input comes from TWO matrices.  Column k < D is obs[row][k], normalised in float64 and
// rounded once; column D <= k < D + A is the stored float64 action act[row][k - D] rounded once (the host's normalisation image
// holds shift 0 and scale 1 there, and (a - 0) * 1 is a); the rest is 0.  A lane stages two adjacent columns, so with D odd (the
// 13-bus feeder: 71 + 4) one lane's pair straddles the two matrices, and with D + A odd the last pair straddles the padding: every
// column picks its source by itself.  A row's value depends on that row and the image alone: every sum runs over k in an order
// fixed by the layer's shape, whatever the row's place in its tile and whatever the launch.
// The small kernels take one thread per element or sample; where include/gridstep.h states a formula nothing is contracted.
#include <hip/hip_runtime.h>
#include <math.h>

#include "bootstrap.h"
#include "mlp_f32.h"
#include "q.h"

namespace {

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

// what gq_scalar_net (mlp_f32.h) takes from this kernel: the stage over two matrices, and a plain store
struct GqaNet {
  template <bool EVEN>
  static __device__ __forceinline__ void stage(const GsQArgs& P, float* tile, int rows, int row0, int kb0, int kb1, int wave, int lane) {
    gqa_stage<EVEN>(P.obs, P.act, P.shift, P.scale, P.D, P.A, rows, P.obs_stride, tile, row0, kb0, kb1, wave, lane);
  }
  static __device__ __forceinline__ void store(const GsQArgs& P, int row, double v) { P.out[row] = v; }
};

}  // namespace

extern "C" __global__ void __launch_bounds__(64 * GS_POL_WAVES)
gs_k_q_mlp_f32(GsQArgs P) { gq_scalar_net<GqaNet>(P, nullptr); }

// the same body launched over a list's capacity, the row count read on the device (the terminal list of gs_rollout_evaluate_q_next)
extern "C" __global__ void __launch_bounds__(64 * GS_POL_WAVES)
gs_k_q_mlp_rows_f32(GsQArgs P, const int32_t* rows_dev) { gq_scalar_net<GqaNet>(P, rows_dev); }

extern "C" __global__ void __launch_bounds__(256)
gs_k_q_combine(GsQCombineArgs C) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C.n) return;
  double m[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    m[s] = gb_twin_min(C.q[s][0], C.q[s][1], (size_t)i);
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
  G.td[i] = gb_td(G.rew[i], G.reward_shift, G.reward_scale, G.gamma, vnext);
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_q_gather(GsQGatherArgs G) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int W = G.DA > 0 ? G.DA : 1;
  if (e >= (long long)G.n * W) return;
  const int i = (int)(e / W), k = (int)(e - (long long)i * W);
  const long long j = gb_row(G.idx[i], G.N);
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
