// policy.h -- the MLP policy of gs_rollout(GS_POLICY_MLP): the rules of gs_policy_mlp (include/gridstep.h) checked on the host, the
// weights laid out in the operand order of v_mfma_f64_16x16x4, and the argument block of gs_k_policy_mlp (kernels_policy.hip).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/gridstep.h"

// Tile shape of gs_k_policy_mlp.  A workgroup of GS_POL_WAVES wavefronts owns GS_POL_ROWS instances (two 16-row tiles of the matrix
// instruction); an output column tile is 16 wide; the k axis advances in blocks of 8 (one 16-byte operand per lane: k-steps j = 0, 1
// of a block take k = 8 kb + 2 (lane >> 4) + j), two blocks per loop trip, so every layer's input width is padded to 16.
constexpr int GS_POL_ROWS = 32, GS_POL_WAVES = 4, GS_POL_MAX_WIDTH = 256;
constexpr int GS_POL_LDS_STRIDE = GS_POL_MAX_WIDTH + 8;      // doubles per activation row in LDS (16 rows x 16 bytes spread over the banks)
constexpr int GS_POL_LDS_BYTES = GS_POL_ROWS * GS_POL_LDS_STRIDE * 8;

struct GsPolicyLayer {
  const double* w;      // [nt][kb][64 lanes][2]: W[16 nt + (lane & 15)][8 kb + 2 (lane >> 4) + j], zero beyond the layer's shape
  const double* b;      // [16 nt]
  int32_t kb, nt;       // 8-wide k blocks (even), 16-wide column tiles
};

struct GsPolicyArgs {
  const double* obs;    // [B][D]
  double* act;          // [B][A]
  int32_t B, D, A, n_layers, activation, head, stochastic, t;
  uint64_t seed; int64_t first_instance;
  GsPolicyLayer L[GS_POLICY_MAX_LAYERS];
};

// empty, or why `p` breaks the rules of gs_policy_mlp
std::string gs_policy_check(const gs_policy_mlp* p, int32_t obs_dim, int32_t action_dim);
// The device image of a checked policy: every layer's packed weights and padded bias behind one another in `blob`; w_off / b_off:
// where layer l starts (in doubles), kb / nt: its block counts
struct GsPolicyImage { std::vector<double> blob; size_t w_off[GS_POLICY_MAX_LAYERS], b_off[GS_POLICY_MAX_LAYERS]; int32_t kb[GS_POLICY_MAX_LAYERS], nt[GS_POLICY_MAX_LAYERS]; };
GsPolicyImage gs_policy_pack(const gs_policy_mlp& p);
