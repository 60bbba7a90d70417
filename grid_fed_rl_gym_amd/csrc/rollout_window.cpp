// rollout_window.cpp -- the host side of gs_rollout_continue (rollout_window.h).  Plain C++, no HIP.
#include "rollout_window.h"

#include <algorithm>
#include <climits>
#include <cstdio>

std::string gs_window_check(const gs_rollout_continue_config* c, const GsWindowState& s, int* code) {
  char buf[256];
  *code = GS_E_INVALID;
  if (!c) return "gs_rollout_continue_config is NULL";
  if (c->struct_size != (int32_t)sizeof(gs_rollout_continue_config)) {
    snprintf(buf, sizeof buf, "gs_rollout_continue_config.struct_size is %d, not %zu", c->struct_size, sizeof(gs_rollout_continue_config));
    return buf;
  }
  if (c->T <= 0) { snprintf(buf, sizeof buf, "gs_rollout_continue_config.T is %d: T <= 0", c->T); return buf; }
  if (c->keep < 0) { snprintf(buf, sizeof buf, "gs_rollout_continue_config.keep is %d: keep < 0", c->keep); return buf; }
  if (c->policy != GS_POLICY_UPLOADED && c->policy != GS_POLICY_RANDOM && c->policy != GS_POLICY_MLP) {
    snprintf(buf, sizeof buf, "unknown policy %d", c->policy);
    return buf;
  }
  if (c->policy == GS_POLICY_UPLOADED && !c->actions && s.action_dim > 0) return "GS_POLICY_UPLOADED needs actions[T][B][action_dim] for the new steps";
  if (c->keep > 0 && s.T_cur <= 0) {
    *code = GS_E_STATE;
    snprintf(buf, sizeof buf, "gs_rollout_continue: keep = %d, but the handle holds no rollout", c->keep);
    return buf;
  }
  if (c->keep > s.T_cur) {
    snprintf(buf, sizeof buf, "gs_rollout_continue_config.keep is %d: more than the %d steps of the current rollout", c->keep, s.T_cur);
    return buf;
  }
  if ((int64_t)c->keep + c->T > (int64_t)INT32_MAX - 1) {
    snprintf(buf, sizeof buf, "keep + T = %lld steps: beyond int32", (long long)c->keep + c->T);
    return buf;
  }
  *code = GS_E_STATE;
  if (c->policy == GS_POLICY_MLP && !s.policy_set) return "GS_POLICY_MLP before gs_policy_mlp_set";
  if (!s.was_reset) return "gs_rollout_continue before gs_reset";
  if (c->keep > 0 && !s.collected)
    return "gs_rollout_continue: keep > 0, but the current rollout was installed by gs_rollout_load: the environment does not stand at its last slot";
  if (c->keep > 0 && s.moved)
    return "gs_rollout_continue: keep > 0, but the environment was moved since the rollout ended (gs_reset, gs_set_state, gs_step or an upload of "
           "state): the new steps would not follow the kept ones";
  *code = GS_OK;
  return "";
}

std::vector<GsWindowMove> gs_window_schedule(int32_t T_old, int32_t keep, int32_t extra, int32_t limit, bool disjoint) {
  std::vector<GsWindowMove> out;
  const int32_t dist = T_old - keep, rows = keep + extra;
  if (keep <= 0 || dist < 0 || (!disjoint && dist == 0)) return out;
  int32_t most = disjoint ? rows : dist;
  if (limit > 0) most = std::min(most, limit);
  for (int32_t at = 0; at < rows; at += most) out.push_back(GsWindowMove{dist + at, at, std::min(most, rows - at)});
  return out;
}
