// kernels_value.hip -- the value network of gs_value_mlp_set (include/gridstep.h; GS_HEAD_LINEAR, float32 layers) over a row-major
// [rows][obs_dim] float64 matrix: gs_k_value_mlp_f32; and the advantages of the last rollout: gs_k_gae.
//
// gs_k_value_mlp_f32 (its body is gq_scalar_net of mlp_f32.h, shared with gs_k_q_mlp_f32).
// The layers of gs_k_policy_mlp_f32 (mlp_f32.h: float64 normalisation rounded once into LDS, hidden layers on
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

#include "bootstrap.h"
#include "mlp_f32.h"
#include "policy.h"

namespace {

// What gq_scalar_net (mlp_f32.h) takes from this kernel: the observation's stage, and a store that also scatters a row's value to
// its (t, b)
struct GvNet {
  template <bool EVEN>
  static __device__ __forceinline__ void stage(const GsValueArgs& P, float* tile, int rows, int row0, int kb0, int kb1, int wave, int lane) {
    gq_stage<GS_VAL_ROWS, EVEN>(P.obs, P.shift, P.scale, P.D, rows, P.obs_stride, tile, row0, kb0, kb1, wave, lane);
  }
  static __device__ __forceinline__ void store(const GsValueArgs& P, int row, double v) {
    P.out[row] = v;
    if (P.scatter_idx) {
      const int t = P.scatter_idx[2 * row], b = P.scatter_idx[2 * row + 1];
      if ((unsigned)t < (unsigned)P.scatter_T && (unsigned)b < (unsigned)P.scatter_B) P.scatter_out[(size_t)t * P.scatter_B + b] = v;
    }
  }
};

}  // namespace

// the row count may be read on the device: the terminal list is launched over its capacity
extern "C" __global__ void __launch_bounds__(64 * GS_POL_WAVES)
gs_k_value_mlp_f32(GsValueArgs P) { gq_scalar_net<GvNet>(P, P.rows_dev); }

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
    const double delta = gb_td(G.rew[i], G.reward_shift, G.reward_scale, G.gamma, vnext) - v;
    const double adv = done ? delta : delta + gl * adv_next;
    G.adv[i] = adv;
    G.ret[i] = adv + v;
    adv_next = adv;
  }
}
