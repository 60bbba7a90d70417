// refresh.h -- per-minibatch refresh of the rollout's bootstrap signals (include/gridstep.h "per-minibatch targets"; DESIGN.md section
// 27): the argument blocks of the kernels of kernels_refresh.hip, shared with abi_refresh.hip, and the host checks of
// gs_learner_refresh that need no device (refresh_check.cpp runs them under a sanitizer).
#pragma once
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/gridstep.h"

// batch row i -> transition j = idx[i] clamped into [0, N): the ONE statement of the rule, as text a host program can run
// (tests/native/refresh_check_host.cpp does).  The kernels form j through gb_row of bootstrap.h, which is this macro as a function.
#define GS_RF_CLAMP(j, N) ((j) < 0 ? 0 : ((j) >= (N) ? (N) - 1 : (j)))

// gs_k_refresh_terms, ONE workgroup of GS_RF_TERM_THREADS threads, no atomics: the batch rows whose transition ended an episode under
// the mask and has a terminal entry (done[j] & mask, map[j] >= 0), compacted in ascending i: ie[k] = (i, e), tb[k] = the entry's
// (t, b), pos[i] = k (-1 for every other row), count[0] = their number
constexpr int GS_RF_TERM_THREADS = 256;
struct GsRefreshTermsArgs {
  const int32_t* idx;         // [n]
  const uint8_t* done;        // [N]
  const int32_t* map;         // [N] transition -> terminal entry, -1: none
  const int32_t* term_idx;    // [term_cap][2] (t, b)
  int32_t* ie;                // [n][2]
  int32_t* tb;                // [n][2]
  int32_t* pos;               // [n]
  int32_t* count;             // [1]
  long long N;
  int32_t n, mask;
};

// gs_k_refresh_rows, one thread per (batch row i, column c), c < W = max(D, A, 2): the float64 rows the networks read, gathered into
// contiguous blocks.  own[i] = obs_seq[j], next[i] = obs_seq[j + B], act[i] = actions[j], tb[i] = (j / B, j % B); and, for k < count,
// term[k] = term_obs[e_k].  A NULL block is not gathered.
struct GsRefreshRowsArgs {
  const int32_t* idx;         // [n]
  const double* obs_seq;      // [T + 1][B][D]
  const double* actions;      // [N][A]
  const double* term_obs;     // [term_cap][D]
  const int32_t* ie;          // [n][2], NULL without a terminal block
  const int32_t* count;       // [1]
  double* own;                // [n][D]
  double* next;               // [n][D]
  double* act;                // [n][A]
  int32_t* tb;                // [n][2]
  double* term;               // [n][D]
  long long N;
  int32_t n, B, D, A, W, reserved;
};

// gs_k_refresh_td_policy, one thread per batch row i: gs_k_q_next_td's functions of bootstrap.h on the scratch results, scattered to
// transition j and, where pos[i] = k >= 0, to terminal entry e = ie[k][1].
//   q_min[j] = m = gb_twin_min at i;  vnext = done[j] ? 0 : gb_soft_value(m, alpha, lp[i])
//   k >= 0:  term_q_min[e] = tm = gb_twin_min at k;  term_value[e] = vnext = gb_soft_value(tm, alpha, term_lp[k])
//   td[j] = gb_td(rew[j], shift, scale, gamma, vnext)
// and the rows' pre_head / act / noise / lp / q (the terminal block's to e) are copied to their places.
struct GsRefreshTdPolicyArgs {
  const int32_t* idx; const int32_t* pos; const int32_t* ie;      // [n], [n] or NULL, [n][2]
  const float* s_pre; const double* s_act; const double* s_eps; const double* s_lp; const double* s_q[2];          // scratch, batch rows
  const float* st_pre; const double* st_act; const double* st_eps; const double* st_lp; const double* st_q[2];    // scratch, terminal block
  const double* rew; const uint8_t* done;
  float* pre; double* act; double* eps; double* lp; double* q[2]; double* q_min; double* td;                      // [N] arrays of gs_handle::QNext
  float* t_pre; double* t_act; double* t_eps; double* t_lp; double* t_q[2]; double* t_q_min; double* t_value;    // [term_cap] arrays
  long long N;
  int32_t n, A;
  double gamma, alpha, reward_shift, reward_scale;
};

// gs_k_refresh_td_value, one thread per batch row: gs_k_q_td's gb_td on the refreshed values.
//   vnext = done[j] ? (pos[i] = k >= 0 ? tv[k] : 0) : vn[i];   td[j] = gb_td(rew[j], shift, scale, gamma, vnext)
struct GsRefreshTdValueArgs {
  const int32_t* idx; const int32_t* pos;      // pos: NULL under mask 0
  const double* vn;           // [n] V(next state of j)
  const double* tv;           // [n] V(terminal observation of e_k)
  const double* rew; const uint8_t* done;
  double* td;                 // [N]
  long long N;
  int32_t n, reserved;
  double gamma, reward_shift, reward_scale;
};

// gs_k_refresh_combine, one thread per batch row: gs_k_q_combine's gb_twin_min for ONE source.  q[w][j] = s_q[w][i];
// q_min[j] = gb_twin_min at i; with `values` (the online source): q_adv[j] = q_min[j] - values[i].
struct GsRefreshCombineArgs {
  const int32_t* idx;
  const double* s_q[2];       // [n] each; NULL: that twin is not installed
  const double* values;       // [n] or NULL
  double* q[2];               // [N]
  double* q_min;              // [N]
  double* q_adv;              // [N], written with `values`
  long long N;
  int32_t n, reserved;
};

// ---- what gs_learner_refresh checks without a device ----
constexpr int32_t GS_REFRESH_ALL = GS_REFRESH_TD_POLICY | GS_REFRESH_Q_TARGET | GS_REFRESH_TD_VALUE | GS_REFRESH_Q_ADV;
constexpr int32_t GS_REFRESH_MAX_N = 1 << 24;

// empty, or why the config (with n batch rows) is GS_E_INVALID; what gae_check refuses is the caller's to add
inline std::string gs_refresh_check(const gs_refresh_config* cfg, int32_t n) {
  if (!cfg) return "config is NULL";
  if (cfg->struct_size != (int32_t)sizeof(gs_refresh_config))
    return "gs_refresh_config struct_size " + std::to_string(cfg->struct_size) + " != " + std::to_string(sizeof(gs_refresh_config));
  if (cfg->groups == 0 || (cfg->groups & ~GS_REFRESH_ALL)) return "gs_learner_refresh: groups = " + std::to_string(cfg->groups) + " names no group or an unknown one";
  if (!std::isfinite(cfg->alpha) || cfg->alpha < 0.0) return "gs_learner_refresh: alpha = " + std::to_string(cfg->alpha) + " is not a finite value >= 0";
  if (cfg->stochastic != 0 && cfg->stochastic != 1) return "gs_learner_refresh: stochastic = " + std::to_string(cfg->stochastic) + " outside {0, 1}";
  if (n <= 0 || n > GS_REFRESH_MAX_N) return "gs_learner_refresh: n = " + std::to_string(n) + " outside 1 .. 2^24";
  return std::string();
}

// the elements of each scratch block for n batch rows; every product fits a size_t for n <= 2^24 and the ABI's widths
struct GsRefreshSizes { size_t rows, pairs, obs, act, pre, twin; };
inline GsRefreshSizes gs_refresh_sizes(int32_t n, int32_t D, int32_t A) {
  const size_t r = (size_t)n;
  return GsRefreshSizes{r, 2 * r, r * (size_t)D, r * (size_t)A, 2 * r * (size_t)A, 2 * r};
}
