// policy.h -- the MLP policy of gs_rollout(GS_POLICY_MLP): the rules of gs_policy_mlp (include/gridstep.h) checked on the host, the
// weights laid out in the operand order of v_mfma_f64_16x16x4, and the argument block of gs_k_policy_mlp (kernels_policy.hip); below
// that the same for the float32 compute path (gs_policy_mlp_opts, v_mfma_f32_16x16x4, gs_k_policy_mlp_f32 in kernels_policy_f32.hip).
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

// ---- the float32 compute path (GS_COMPUTE_F32): gs_k_policy_mlp_f32, kernels_policy_f32.hip --------------------------------------
// Same workgroup (GS_POL_WAVES wavefronts, GS_POL_ROWS instances, 16-wide column tiles) on v_mfma_f32_16x16x4_f32.  The k axis
// advances in blocks of 16: one 16-byte operand per lane holds the four k-steps j = 0 .. 3 of a block, k = 16 kb + 4 (lane >> 4) + j,
// so every layer's input width is padded to 16.  LDS: the normalised float32 observation tile, in panels of at most
// GS_POL32_PANEL_KB blocks (one panel for every obs_dim <= 1008), and one activation tile; both row strides are 4 mod 16 floats, so
// that the sixteen rows of an operand read start on sixteen different banks.
constexpr int GS_POL32_PANEL_KB = 63;
constexpr int GS_POL32_ACT_STRIDE = GS_POL_MAX_WIDTH + 4;   // floats per activation row
inline int gs_pol32_obs_stride(int kb0) { return 16 * (kb0 < GS_POL32_PANEL_KB ? kb0 : GS_POL32_PANEL_KB) + 4; }   // floats per observation row
inline int gs_pol32_lds_bytes(int kb0) { return GS_POL_ROWS * (gs_pol32_obs_stride(kb0) + GS_POL32_ACT_STRIDE) * 4; }

struct GsPolicyLayerF32 {
  const float* w;       // [nt][kb][64 lanes][4]: W[16 nt + (lane & 15)][16 kb + 4 (lane >> 4) + j], zero beyond the layer's shape
  const float* b;       // [16 nt]
  int32_t kb, nt;       // 16-wide k blocks, 16-wide column tiles
};

struct GsPolicyArgsF32 {
  const double* obs;    // [B][D]
  double* act;          // [B][A]
  const double* shift;  // [16 L[0].kb]: obs_shift, 0 beyond D
  const double* scale;  // [16 L[0].kb]: obs_scale, 0 beyond D (a padded column normalises to 0)
  int32_t B, D, A, n_layers, activation, head, stochastic, t;
  uint64_t seed; int64_t first_instance;
  int32_t obs_stride, reserved;
  GsPolicyLayerF32 L[GS_POLICY_MAX_LAYERS];
};

// empty, or why `p` with the options `o` (may be NULL) breaks the rules of gs_policy_mlp / gs_policy_mlp_opts
std::string gs_policy_check_opts(const gs_policy_mlp* p, const gs_policy_mlp_opts* o, int32_t obs_dim, int32_t action_dim);
inline bool gs_policy_is_f32(const gs_policy_mlp_opts* o) { return o && o->compute == GS_COMPUTE_F32; }
// The float32 device image of a checked policy: `blob` holds every layer's packed weights and padded bias, rounded to nearest
// (offsets in floats, multiples of 4); `norm` holds shift [16 kb[0]] then scale [16 kb[0]]
struct GsPolicyImageF32 {
  std::vector<float> blob; std::vector<double> norm;
  size_t w_off[GS_POLICY_MAX_LAYERS], b_off[GS_POLICY_MAX_LAYERS]; int32_t kb[GS_POLICY_MAX_LAYERS], nt[GS_POLICY_MAX_LAYERS];
};
GsPolicyImageF32 gs_policy_pack_f32(const gs_policy_mlp& p, const gs_policy_mlp_opts& o);
