// q.h -- state-action critics (include/gridstep.h "state-action critics"): the argument blocks of the kernels
// of kernels_q.hip, shared with abi_q.hip and abi_learner.hip, and the rules of gs_q_mlp_set checked on the host.
#pragma once
#include <stdint.h>

#include <string>

#include "policy.h"

// gs_k_q_mlp_f32: the value kernel's tile (GS_VAL_ROWS rows a workgroup, panels of at most GS_VAL_PANEL_KB blocks, its LDS sizes) over
// rows whose input is obs[row][0 .. D) normalised, then act[row][0 .. A) as stored, then zeros up to 16 L[0].kb
struct GsQArgs {
  const double* obs;          // [rows][D]
  const double* act;          // [rows][A]
  double* out;                // [rows]
  const double* shift;        // [16 L[0].kb]: obs_shift, 0 for the action columns and beyond
  const double* scale;        // [16 L[0].kb]: obs_scale, 1 for the action columns, 0 beyond D + A
  int32_t rows, D, A, n_layers, activation, obs_stride, panel_kb, reserved;
  GsPolicyLayerF32 L[GS_POLICY_MAX_LAYERS];
};

// gs_k_q_combine: q_min[src] = gb_twin_min (bootstrap.h) over the installed twins (a missing twin: NULL), q_adv = q_min[online] - values
struct GsQCombineArgs {
  const double* q[2][2];      // [src][which], [n] each
  const double* values;       // [n] (the first T rows of values[T + 1][B])
  double* q_min[2];           // [src]
  double* q_adv;
  long long n;
};

// gs_k_q_td: td[t][b] = gb_td (bootstrap.h) of the r' and vnext of gs_k_gae.  phase 0: one thread per transition, every finished one
// takes vnext = 0; phase 1: one thread per entry of the terminal list (launched over its capacity, the count read on the device),
// which gives a transition whose flag meets the mask the value of its terminal observation
struct GsQTdArgs {
  const double* values;       // [T + 1][B]
  const double* rew;          // [T][B]
  const uint8_t* done;        // [T][B]
  const double* term_values;  // [term_cap]
  const int32_t* term_count; const int32_t* term_idx;      // [1], [term_cap][2] (t, b)
  double* td;                 // [T][B]
  int32_t T, B, mask, term_cap, phase, reserved;
  double gamma, reward_shift, reward_scale;
};

// gs_k_q_gather: per sample i with transition j = gb_row(idx[i], N) (bootstrap.h): y[i] = (float)src[j]; with DA > 0 also the
// learner's input row sa[i] = obs[i][0 .. D) | (float)act[j][0 .. DA - D)
struct GsQGatherArgs {
  const int32_t* idx;         // [n]
  const double* src;          // [N]
  float* y;                   // [n]
  const float* obs;           // [n][D] or NULL
  const double* act;          // [N][DA - D]
  float* sa;                  // [n][DA]
  long long N;
  int32_t n, D, DA, reserved;
};

// gs_k_q_polyak: t = (tau * p) + (omt * t) over the n floats of a packed image
struct GsQPolyakArgs {
  const float* p; float* t;
  long long n;
  float tau, omt;
};

// empty, or why `p` with `o` breaks the rules of gs_q_mlp_set (include/gridstep.h)
std::string gs_q_check(const gs_policy_mlp* p, const gs_policy_mlp_opts* o, int32_t obs_dim, int32_t action_dim);
