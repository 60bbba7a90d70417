// The host side of gs_rollout_continue that needs no device (csrc/rollout_window.h: gs_window_check, gs_window_schedule), run
// stand-alone: every refusal with its code, and the schedule of the shift replayed on host arrays for every (T_old <= 9, keep <= T_old,
// block limit, with and without the slot behind the last step, in place and into another buffer) against a plain copy -- with no
// entry whose source and destination overlap, none that leaves the array, and the entries ascending.  Prints "ok" lines; exit
// status 1 on a mismatch.  tests/test_rollout_window.py builds it together with csrc/rollout_window.cpp under the address and
// undefined-behaviour sanitizers (host compile only) and runs it as a process of its own.
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "rollout_window.h"

static int failures = 0;

static void verdict(const gs_rollout_continue_config* c, const GsWindowState& s, int want, const char* needle, const char* what) {
  int code = -1;
  const std::string why = gs_window_check(c, s, &code);
  const bool ok = want == GS_OK ? (why.empty() && code == GS_OK) : (code == want && why.find(needle) != std::string::npos);
  if (!ok) { std::printf("MISMATCH %s: code %d, %s\n", what, code, why.empty() ? "accepted" : why.c_str()); ++failures; }
}

// the schedule replayed with memcpy on [steps][W] ints; false on any rule broken
static bool replay(int T_old, int keep, int extra, int limit, bool disjoint) {
  const int W = 3, slots = T_old + extra;
  std::vector<int> a((size_t)slots * W), want;
  for (size_t i = 0; i < a.size(); ++i) a[i] = (int)(1000 + i);
  const std::vector<int> before = a;
  std::vector<int> other((size_t)slots * W, -1);
  std::vector<int>& dst = disjoint ? other : a;
  const std::vector<GsWindowMove> sch = gs_window_schedule(T_old, keep, extra, limit, disjoint);
  int last_src = -1;
  for (const GsWindowMove& m : sch) {
    if (m.rows <= 0 || m.src_row < 0 || m.dst_row < 0 || m.src_row + m.rows > slots || m.dst_row + m.rows > slots) return false;
    if (limit > 0 && m.rows > limit) return false;
    if (m.src_row <= last_src) return false;                                            // ascending
    if (!disjoint && !(m.dst_row + m.rows <= m.src_row || m.src_row + m.rows <= m.dst_row)) return false;      // no overlap within a launch
    last_src = m.src_row;
    std::memcpy(dst.data() + (size_t)m.dst_row * W, a.data() + (size_t)m.src_row * W, (size_t)m.rows * W * sizeof(int));      // (memcpy: the sanitizer reports an overlap)
  }
  if (keep == 0) return sch.empty();
  // the plain copy: steps T_old - keep .. T_old - 1 + extra at the front
  const int rows = keep + extra;
  return std::memcmp(dst.data(), before.data() + (size_t)(T_old - keep) * W, (size_t)rows * W * sizeof(int)) == 0;
}

int main() {
  static_assert(sizeof(gs_rollout_continue_config) == 40 && sizeof(gs_rollout_window_info_out) == 16, "the structs of include/gridstep.h");
  const double some = 0.0;
  gs_rollout_continue_config ok{};
  ok.struct_size = (int32_t)sizeof(gs_rollout_continue_config); ok.T = 5; ok.keep = 3; ok.policy = GS_POLICY_RANDOM;
  const GsWindowState st{7, 2, true, true, true, false};

  verdict(&ok, st, GS_OK, "", "the plain case");
  verdict(nullptr, st, GS_E_INVALID, "NULL", "NULL config");
  for (int sz : {0, 32, 48, -40}) { gs_rollout_continue_config c = ok; c.struct_size = sz; verdict(&c, st, GS_E_INVALID, "struct_size", "struct_size"); }
  for (int t : {0, -1, std::numeric_limits<int32_t>::min()}) { gs_rollout_continue_config c = ok; c.T = t; verdict(&c, st, GS_E_INVALID, "T <= 0", "T"); }
  for (int k : {-1, std::numeric_limits<int32_t>::min()}) { gs_rollout_continue_config c = ok; c.keep = k; verdict(&c, st, GS_E_INVALID, "keep < 0", "keep < 0"); }
  { gs_rollout_continue_config c = ok; c.keep = 8; verdict(&c, st, GS_E_INVALID, "more than the 7 steps", "keep > T"); }
  { gs_rollout_continue_config c = ok; c.keep = 7; verdict(&c, st, GS_OK, "", "keep == T"); }
  for (int p : {3, -1}) { gs_rollout_continue_config c = ok; c.policy = p; verdict(&c, st, GS_E_INVALID, "unknown policy", "policy"); }
  { gs_rollout_continue_config c = ok; c.policy = GS_POLICY_UPLOADED; verdict(&c, st, GS_E_INVALID, "needs actions", "uploaded without actions");
    c.actions = &some; verdict(&c, st, GS_OK, "", "uploaded with actions");
    c.actions = nullptr; GsWindowState s0 = st; s0.action_dim = 0; verdict(&c, s0, GS_OK, "", "uploaded, no action columns"); }
  { gs_rollout_continue_config c = ok; c.T = std::numeric_limits<int32_t>::max(); verdict(&c, st, GS_E_INVALID, "beyond int32", "keep + T"); }
  { GsWindowState s = st; s.T_cur = 0; verdict(&ok, s, GS_E_STATE, "holds no rollout", "keep without a rollout"); }
  { GsWindowState s = st; s.policy_set = false; gs_rollout_continue_config c = ok; c.policy = GS_POLICY_MLP; verdict(&c, s, GS_E_STATE, "gs_policy_mlp_set", "no policy");
    verdict(&c, st, GS_OK, "", "a policy"); }
  { GsWindowState s = st; s.was_reset = false; verdict(&ok, s, GS_E_STATE, "before gs_reset", "no reset"); }
  { GsWindowState s = st; s.collected = false; verdict(&ok, s, GS_E_STATE, "gs_rollout_load", "a loaded rollout"); }
  { GsWindowState s = st; s.moved = true; verdict(&ok, s, GS_E_STATE, "was moved", "a moved environment"); }
  // keep == 0 wherever gs_rollout is allowed: no rollout, a loaded one, a moved environment
  { GsWindowState s = st; s.T_cur = 0; s.collected = false; s.moved = true; gs_rollout_continue_config c = ok; c.keep = 0; verdict(&c, s, GS_OK, "", "keep == 0"); }
  if (failures) return 1;
  std::printf("refusals: ok\n");

  int cases = 0;
  for (int T_old = 1; T_old <= 9; ++T_old)
    for (int keep = 0; keep <= T_old; ++keep)
      for (int limit = 0; limit <= 10; ++limit)
        for (int extra = 0; extra <= 1; ++extra)
          for (int disjoint = 0; disjoint <= 1; ++disjoint) {
            ++cases;
            if (!replay(T_old, keep, extra, limit, disjoint != 0)) {
              std::printf("MISMATCH schedule T_old %d keep %d extra %d limit %d disjoint %d\n", T_old, keep, extra, limit, disjoint);
              ++failures;
            }
          }
  // what the issue names: the shift by one step (keep = T_old - 1) takes keep (+ 1) launches of one step each
  if (gs_window_schedule(7, 6, 0, 0, false).size() != 6 || gs_window_schedule(7, 6, 1, 0, false).size() != 7) { std::printf("MISMATCH the shift by one\n"); ++failures; }
  if (!gs_window_schedule(7, 7, 1, 0, false).empty() || gs_window_schedule(7, 7, 1, 0, true).size() != 1) { std::printf("MISMATCH keep == T_old\n"); ++failures; }
  if (failures) return 1;
  std::printf("schedule: ok (%d cases)\n", cases);
  return 0;
}
