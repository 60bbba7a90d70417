// policy.h -- the MLP policy of gs_rollout(GS_POLICY_MLP): the rules of gs_policy_mlp (include/gridstep.h) checked on the host, the
// weights laid out in the operand order of v_mfma_f64_16x16x4, and the argument block of gs_k_policy_mlp (kernels_policy.hip); below
// that the same for the float32 compute path (gs_policy_mlp_opts, v_mfma_f32_16x16x4, gs_k_policy_mlp_f32 in kernels_policy_f32.hip),
// then the value network and the advantage kernel of on-policy rollouts (gs_k_value_mlp_f32, gs_k_gae in kernels_value.hip).
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
  double* logp;         // [B] or NULL: the log-probability of the sampled action (stochastic Gaussian head only; policy_head.h)
  int32_t logp_behind, reserved;      // its per-action terms lie behind the activation tile in LDS (3 A > GS_POL_LDS_STRIDE), not inside it
  GsPolicyLayer L[GS_POLICY_MAX_LAYERS];
};
// LDS of gs_k_policy_mlp: the activation tile, and behind it the log-probability terms where the tile's rows have no room for them
inline bool gs_pol_logp_behind(int A) { return 3 * A > GS_POL_LDS_STRIDE; }
inline int gs_pol_lds_bytes(int A) { return GS_POL_LDS_BYTES + (gs_pol_logp_behind(A) ? GS_POL_ROWS * A * 8 : 0); }
// The most any policy needs (A <= GS_POL_MAX_WIDTH / 2).  The cap on a kernel's dynamic LDS is a setting of the FUNCTION, shared by
// every handle of the process: it is always set to this, never to one handle's own need, which a second handle could lower.
constexpr int GS_POL_LDS_MAX = GS_POL_LDS_BYTES + GS_POL_ROWS * (GS_POL_MAX_WIDTH / 2) * 8;

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
// ... with room for the log-probability terms [GS_POL_ROWS][A] doubles, which reuse the observation tile (wider for every obs_dim > 2 A)
constexpr int GS_POL32_LDS_MAX = GS_POL_ROWS * (16 * GS_POL32_PANEL_KB + 4 + GS_POL32_ACT_STRIDE) * 4;      // a full panel (> 8 A bytes a row for every A); see GS_POL_LDS_MAX
inline int gs_pol32_lds_bytes(int kb0, int A) { const int obs = gs_pol32_obs_stride(kb0) * 4; return GS_POL_ROWS * ((obs > 8 * A ? obs : 8 * A) + GS_POL32_ACT_STRIDE * 4); }

struct GsPolicyLayerF32 {
  const float* w;       // [nt][kb][64 lanes][4]: W[16 nt + (lane & 15)][16 kb + 4 (lane >> 4) + j], zero beyond the layer's shape
  const float* b;       // [16 nt]
  int32_t kb, nt;       // 16-wide k blocks, 16-wide column tiles
};
// That layout, stated once for the host and the device (a constexpr function is both): where W[o][k] lies in `w` of a layer with kb k
// blocks.  The image of W^T (train.h, GsTrainNet::T) holds W[o][k] at gs_pol32_slot(k, o, that image's kb).
constexpr size_t gs_pol32_slot(int o, int k, int kb) {
  return (((size_t)(o >> 4) * kb + (k >> 4)) * 64 + ((k & 15) >> 2) * 16 + (o & 15)) * 4 + (k & 3);
}

struct GsPolicyArgsF32 {
  const double* obs;    // [B][D]
  double* act;          // [B][A]
  const double* shift;  // [16 L[0].kb]: obs_shift, 0 beyond D
  const double* scale;  // [16 L[0].kb]: obs_scale, 0 beyond D (a padded column normalises to 0)
  int32_t B, D, A, n_layers, activation, head, stochastic, t;
  uint64_t seed; int64_t first_instance;
  int32_t obs_stride, reserved;
  double* logp;         // [B] or NULL: as GsPolicyArgs::logp
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
// The way back, for one layer of n_out x n_in whose packed image `L` lies in HOST memory: W row-major [n_out][n_in], then b [n_out],
// into `dst` (torch order; the image holds float32 values, so this is exact).  `wt`, unless NULL, receives the packed image of W^T
// (L.nt k blocks, L.kb column tiles); its padding is not written.
void gs_policy_unpack_f32(const GsPolicyLayerF32& L, int n_out, int n_in, float* dst, float* wt);

// ---- the value network (GS_HEAD_LINEAR): gs_k_value_mlp_f32, kernels_value.hip ---------------------------------------------------
// The float32 path's layers with a scalar output, over any number of rows.  A workgroup of GS_POL_WAVES wavefronts owns GS_VAL_ROWS
// rows (four 16-row tiles: every weight operand feeds twice the products it feeds in the policy kernel); the observation tile is
// staged in panels of at most GS_VAL_PANEL_KB blocks (64 rows x 340 floats = 85 KB beside 65 KB of activations), the blocks spread
// evenly over the panels.  The last layer is a dot product per row (four lanes a row), not a padded tile.
constexpr int GS_VAL_ROWS = 64, GS_VAL_PANEL_KB = 21;
inline int gs_val_panel_kb(int kb0) { const int panels = (kb0 + GS_VAL_PANEL_KB - 1) / GS_VAL_PANEL_KB; return (kb0 + panels - 1) / panels; }
inline int gs_val_obs_stride(int kb0) { return 16 * gs_val_panel_kb(kb0) + 4; }
inline int gs_val_lds_bytes(int kb0) { return GS_VAL_ROWS * (gs_val_obs_stride(kb0) + GS_POL32_ACT_STRIDE) * 4; }
constexpr int GS_VAL_LDS_MAX = GS_VAL_ROWS * (16 * GS_VAL_PANEL_KB + 4 + GS_POL32_ACT_STRIDE) * 4;      // a full panel; see GS_POL_LDS_MAX
static_assert(GS_POL_LDS_MAX <= 160 * 1024 && GS_POL32_LDS_MAX <= 160 * 1024 && GS_VAL_LDS_MAX <= 160 * 1024, "a compute unit of gfx950 has 160 KB of LDS");

struct GsValueArgs {
  const double* obs;          // [rows][D]
  double* out;                // [rows]
  const double* shift;        // [16 L[0].kb], as GsPolicyArgsF32
  const double* scale;
  const int32_t* rows_dev;    // NULL, or the device word holding the number of rows actually there (<= rows: the launch covers `rows`)
  const int32_t* scatter_idx; // NULL, or [rows][2] (t, b): row k's value is ALSO written to scatter_out[t * scatter_B + b]
  double* scatter_out;        // [scatter_T][scatter_B]
  int32_t rows, D, n_layers, activation, obs_stride, panel_kb, scatter_T, scatter_B;
  GsPolicyLayerF32 L[GS_POLICY_MAX_LAYERS];
};
// empty, or why `p` with `o` breaks the rules of gs_value_mlp_set (include/gridstep.h)
std::string gs_value_check(const gs_policy_mlp* p, const gs_policy_mlp_opts* o, int32_t obs_dim);

// gs_k_gae (kernels_value.hip): the recurrence of gs_rollout_evaluate over [T][B] arrays; ret holds the terminal values on entry
struct GsGaeArgs {
  const double* values;       // [T + 1][B]
  const double* rew;          // [T][B]
  const uint8_t* done;        // [T][B]
  double* adv;                // [T][B]
  double* ret;                // [T][B]
  int32_t T, B, mask, reserved;
  double gamma, lambda, reward_shift, reward_scale;
};
