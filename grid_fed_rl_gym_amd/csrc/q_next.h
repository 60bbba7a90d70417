// q_next.h -- policy-action TD targets (include/gridstep.h "policy-action TD targets"): the argument blocks of
// the kernels of kernels_q_next.hip, shared with abi_q_next.hip, and the LDS of gs_k_policy_rows_f32.
#pragma once
#include <stdint.h>

#include "policy.h"

constexpr uint32_t GS_QN_ROLLOUT_TAG = 0x514E5854u;    // 'QNXT': the noise of rollout row (t + 1, b), index t B + b
constexpr uint32_t GS_QN_TERMINAL_TAG = 0x514E5445u;   // 'QNTE': the noise of the terminal observation of transition (t, b)

// gs_k_policy_rows_f32: the value kernel's tile (GS_VAL_ROWS rows a workgroup, panels of at most GS_VAL_PANEL_KB blocks) under the
// POLICY's layer table and normalisation image.  LDS: the activation tile, then the observation panel; the head's per-action terms
// ([GS_VAL_ROWS] rows of A | 1 doubles: an odd stride spreads a wavefront's rows over the banks) reuse the panel, which is made
// wide enough for them.  The cap of the function is GS_VAL_LDS_MAX (a full panel holds the terms of every A <= 128), always.
inline int gs_qn_term_stride(int A) { return A | 1; }
inline int gs_qn_lds_bytes(int kb0, int A) {
  const int obs = gs_val_obs_stride(kb0) * 4, terms = gs_qn_term_stride(A) * 8;
  return GS_VAL_ROWS * ((obs > terms ? obs : terms) + GS_POL32_ACT_STRIDE * 4);
}
static_assert(((GS_POL_MAX_WIDTH / 2) | 1) * 8 <= (16 * GS_VAL_PANEL_KB + 4) * 4, "a full panel holds the head's terms of the widest action");
static_assert(GS_VAL_LDS_MAX <= 160 * 1024, "gs_k_policy_rows_f32 stays within the value kernel's LDS");

struct GsPolicyRowsArgs {
  const double* obs;          // [rows][D]
  const int32_t* rows_dev;    // NULL, or the device word holding the number of rows actually there (<= rows)
  const int32_t* idx;         // NULL: row k's noise index is k; or [rows][2] (t, b): it is t * B + b
  const double* shift;        // [16 L[0].kb]: the policy's normalisation image (GsPolicyArgsF32)
  const double* scale;
  float* pre_head;            // [rows][2 A] mean | log_std as the head reads them
  double* act;                // [rows][A]
  double* logp;               // [rows]
  double* noise;              // [rows][A] eps_k as the head used it (0 when stochastic == 0)
  int32_t rows, B, D, A, n_layers, activation, obs_stride, panel_kb, stochastic, reserved;
  uint32_t draw, tag;
  uint64_t seed;
  GsPolicyLayerF32 L[GS_POLICY_MAX_LAYERS];
};

// gs_k_q_next_td, one thread per element, by the functions of bootstrap.h.  phase 0, per transition i = t B + b:
//   q_next_min[i] = gb_twin_min at i;  v = gb_soft_value(q_next_min[i], alpha, lp[i]);  td[i] = gb_td(rew[i], shift, scale, gamma,
//   done[i] ? 0 : v).
// phase 1, per entry e of the terminal list (launched over its capacity, the count read on the device): term_q_min[e] and
// term_value[e] = gb_soft_value(term_q_min[e], alpha, term_lp[e]) the same way; where done[i] & mask for the entry's (t, b): td[i] =
// gb_td(.., term_value[e]).
struct GsQNextTdArgs {
  const double* q[2];         // [T][B] each; NULL: that twin is not installed
  const double* lp;           // [T][B]
  const double* rew;          // [T][B]
  const uint8_t* done;        // [T][B]
  const double* term_q[2];    // [term_cap] each
  const double* term_lp;      // [term_cap]
  const int32_t* term_count; const int32_t* term_idx;      // [1], [term_cap][2] (t, b)
  double* q_min;              // [T][B]
  double* term_q_min;         // [term_cap]
  double* term_value;         // [term_cap]
  double* td;                 // [T][B]
  int32_t T, B, mask, term_cap, phase, reserved;
  double gamma, alpha, reward_shift, reward_scale;
};
