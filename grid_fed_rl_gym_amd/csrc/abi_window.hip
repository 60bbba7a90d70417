// abi_window.hip -- gs_rollout_continue and gs_rollout_window_info (include/gridstep.h "a sliding window over consecutive rollouts";
// DESIGN.md section 30): the last `keep` steps of the handle's rollout move to the front on the device and T fresh steps are collected
// behind them.  The checks and the schedule of the shift are rollout_window.cpp's (no HIP there); this file owns the second terminal
// list (gs_handle::Window), queues the kernels of kernels_window.hip and then collects as gs_rollout does (abi_rollout.hip), with the
// storage index keep + i and the draw index t0 + i.
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "handle.h"
#include "rollout_window.h"

using namespace gsi;

namespace gsi __attribute__((visibility("hidden"))) {

void window_release(gs_handle* h) {
  gs_handle::Window& w = h->win;
  w.term_idx.release(); w.term_obs.release(); w.pos.release(); w.n_old.release();
}

}  // namespace gsi

namespace {

template <typename X>
void swap_bufs(DevBuf<X>& a, DevBuf<X>& b) { std::swap(a.p, b.p); std::swap(a.cap, b.cap); }

// an array of the rollout as the shift sees it: where it lies now and where the kept steps go (the same buffer in place), the bytes of
// one step, and whether it has the slot behind the last step (obs_seq)
struct ShiftArray { const void* src; void* dst; size_t step_bytes; int extra; };

// queues the launches that move the kept steps of `arr` (src == NULL: not this one) to the front
int queue_shift(gs_handle* h, const ShiftArray (&arr)[GS_WIN_ARRAYS], int T_old, int keep, bool disjoint) {
  const std::vector<GsWindowMove> sch[2] = {gs_window_schedule(T_old, keep, 0, 0, disjoint), gs_window_schedule(T_old, keep, 1, 0, disjoint)};
  const size_t launches = std::max(sch[0].size(), sch[1].size());
  for (size_t j = 0; j < launches; ++j) {
    GsWindowShiftArgs G{};
    long long most = 0;
    for (int a = 0; a < GS_WIN_ARRAYS; ++a) {
      const std::vector<GsWindowMove>& s = sch[arr[a].extra];
      if (!arr[a].src || j >= s.size()) continue;
      G.seg[a].src = (const char*)arr[a].src + (size_t)s[j].src_row * arr[a].step_bytes;
      G.seg[a].dst = (char*)arr[a].dst + (size_t)s[j].dst_row * arr[a].step_bytes;
      G.seg[a].bytes = (long long)((size_t)s[j].rows * arr[a].step_bytes);
      most = std::max(most, G.seg[a].bytes);
    }
    if (!most) continue;
    const unsigned blocks = (unsigned)std::min<long long>((most / 16 + 255) / 256 + 1, 4096);
    hipLaunchKernelGGL(gs_k_window_shift, dim3(blocks, GS_WIN_ARRAYS), dim3(256), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
  }
  return GS_OK;
}

// queues the compaction of the terminal list (idx_in, obs_in: cap_in entries, their count in ro.term_count) into (idx_out, obs_out),
// other buffers of at least as many entries: the entries with t >= drop, in their order, t -= drop; ro.term_count = how many
int queue_terms(gs_handle* h, const int32_t* idx_in, const double* obs_in, int cap_in, int32_t* idx_out, double* obs_out, int drop) {
  gs_handle::Window& w = h->win;
  GsWindowTermsArgs G{idx_in, idx_out, w.pos, h->ro.term_count, w.n_old, cap_in, drop};
  hipLaunchKernelGGL(gs_k_window_terms, dim3(1), dim3(GS_WIN_TERM_THREADS), 0, h->stream, G);
  HIPCHK(h, hipGetLastError());
  GsWindowTermRowsArgs R{obs_in, obs_out, w.pos, w.n_old, h->obs_dim};
  const unsigned blocks = (unsigned)std::min<long long>(((long long)cap_in * h->obs_dim + 255) / 256, 2048);
  hipLaunchKernelGGL(gs_k_window_term_rows, dim3(std::max(blocks, 1u)), dim3(256), 0, h->stream, R);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

// the window's buffers when keep + T steps fit the capacity: the kept steps move to the front where they lie
int shift_in_place(gs_handle* h, int keep, bool with_logp) {
  gs_handle::Rollout& ro = h->ro;
  gs_handle::Window& w = h->win;
  const int T_old = ro.T, drop = T_old - keep;
  if (drop == 0) return GS_OK;      // (the whole rollout stays where it is, and so does its terminal list)
  const size_t B = h->B, D = h->obs_dim, A = h->action_dim, cap = (size_t)ro.term_cap;
  int rc = GS_OK;
  if (w.term_idx.cap < 2 * cap || w.term_obs.cap < cap * D || w.pos.cap < cap || !w.n_old) {
    // (made before anything is queued: a refusal leaves the rollout as it was.  Nothing queued reads them, so no wait.)
    if ((rc = alloc_all(h, "the window's second terminal list", w.term_idx.want(2 * cap), w.term_obs.want(cap * D), w.pos.want(cap), w.n_old.want(1)))) return rc;
  }
  const ShiftArray arr[GS_WIN_ARRAYS] = {{ro.obs_seq.p, ro.obs_seq.p, B * D * sizeof(double), 1},
                                         {A ? ro.act.p : nullptr, ro.act.p, B * A * sizeof(double), 0},
                                         {ro.rew.p, ro.rew.p, B * sizeof(double), 0},
                                         {ro.done.p, ro.done.p, B, 0},
                                         {with_logp ? ro.logp.p : nullptr, ro.logp.p, B * sizeof(double), 0}};
  if ((rc = queue_shift(h, arr, T_old, keep, false))) return rc;
  if ((rc = queue_terms(h, ro.term_idx, ro.term_obs, ro.term_cap, w.term_idx, w.term_obs, drop))) return rc;
  swap_bufs(ro.term_idx, w.term_idx);
  swap_bufs(ro.term_obs, w.term_obs);
  return GS_OK;
}

// the window's buffers when keep + T steps outgrow the capacity: larger ones are made, the kept steps are copied there, the old ones go.
// rollout_ensure's rule for the terminal list: an instance finishes at most once per min(episode_length, 11) steps plus once, and the
// window is keep + T consecutive steps of the environment.  Waits on the host.
int shift_and_grow(gs_handle* h, int keep, int T_new, bool with_logp) {
  gs_handle::Rollout& ro = h->ro;
  gs_handle::Window& w = h->win;
  const int T_old = ro.T, drop = T_old - keep, cap_old = ro.term_cap;
  const size_t B = h->B, D = h->obs_dim, A = h->action_dim, A1 = std::max(h->action_dim, 1);
  const int min_ep = std::max(1, std::min(h->cfg.episode_length, 11));
  const size_t cap = std::max(B * ((size_t)T_new / min_ep + 1), (size_t)cap_old);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  DevBuf<double> obs_seq, act, rew, term_obs, logp; DevBuf<uint8_t> done; DevBuf<int32_t> term_idx, pos, n_old;
  int rc = alloc_all(h, "the window's buffers", obs_seq.want((size_t)(T_new + 1) * B * D), act.want((size_t)T_new * B * A1), rew.want((size_t)T_new * B),
                     done.want((size_t)T_new * B), term_idx.want(cap * 2), term_obs.want(cap * D), pos.want((size_t)cap_old), n_old.want(1));
  if (rc) return rc;
  if (with_logp && (rc = logp.alloc(h, (size_t)T_new * B, "the window's log-probabilities"))) return rc;
  // from here until the collection is queued the handle holds no rollout: every gate on ro.T refuses.  The old buffers leave the
  // handle (what is sized by their capacity goes), the new ones take their place, and the old ones go when the copies are through.
  ro.T = 0; ro.n_term = -1;
  DevBuf<double> o_obs_seq, o_act, o_rew, o_term_obs, o_logp; DevBuf<uint8_t> o_done; DevBuf<int32_t> o_term_idx;
  swap_bufs(ro.obs_seq, o_obs_seq); swap_bufs(ro.act, o_act); swap_bufs(ro.rew, o_rew); swap_bufs(ro.done, o_done);
  swap_bufs(ro.term_idx, o_term_idx); swap_bufs(ro.term_obs, o_term_obs); swap_bufs(ro.logp, o_logp);
  rollout_tracks_release(h, true);
  dataset_release(h, true);
  swap_bufs(ro.obs_seq, obs_seq); swap_bufs(ro.act, act); swap_bufs(ro.rew, rew); swap_bufs(ro.done, done);
  swap_bufs(ro.term_idx, term_idx); swap_bufs(ro.term_obs, term_obs); swap_bufs(ro.logp, logp);
  swap_bufs(w.pos, pos); swap_bufs(w.n_old, n_old);
  ro.T_cap = T_new; ro.term_cap = (int)std::min<size_t>(cap, 0x7fffffff);
  if ((rc = fill_const_columns(h))) return rc;      // (every slot; the kept ones are then overwritten whole, constants included)
  const ShiftArray arr[GS_WIN_ARRAYS] = {{o_obs_seq.p, ro.obs_seq.p, B * D * sizeof(double), 1},
                                         {A ? o_act.p : nullptr, ro.act.p, B * A * sizeof(double), 0},
                                         {o_rew.p, ro.rew.p, B * sizeof(double), 0},
                                         {o_done.p, ro.done.p, B, 0},
                                         {with_logp ? o_logp.p : nullptr, ro.logp.p, B * sizeof(double), 0}};
  if ((rc = queue_shift(h, arr, T_old, keep, true))) return rc;
  if ((rc = queue_terms(h, o_term_idx, o_term_obs, cap_old, ro.term_idx, ro.term_obs, drop))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_rollout_continue(gs_handle* h, const gs_rollout_continue_config* c) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  gs_handle::Rollout& ro = h->ro;
  const bool collected = ro.T > 0 && ro.ended_on && ro.ended_on == ro.calls;
  const GsWindowState st{ro.T, h->action_dim, h->was_reset, h->pol.set, collected, h->env_moves != ro.moves_at_end};
  int code = GS_OK;
  const std::string why = gs_window_check(c, st, &code);
  if (!why.empty()) return fail(h, code, "%s", why.c_str());
  GS_ENTER(h);
  const int T = c->T, keep = c->keep, Tw = keep + T, policy = c->policy;
  const uint64_t policy_seed = c->policy_seed;
  const size_t B = h->B, D = h->obs_dim, A = h->action_dim;
  // a stochastic policy's log-probabilities are recorded with its actions; the window has them when the kept steps have them too
  const bool stochastic = policy == GS_POLICY_MLP && (h->pol.compute == GS_COMPUTE_F32 ? h->pol.args32.stochastic : h->pol.args.stochastic);
  const bool with_logp = stochastic && ro.record_logp && (keep == 0 || ro.logp_recorded);
  int rc = GS_OK;
  if (keep == 0) {                     // gs_rollout with the draw origin t0
    if ((rc = rollout_ensure(h, T))) return rc;
    if (ro.const_dirty && (rc = fill_const_columns(h))) return rc;
    if (with_logp && (rc = ro.logp.grow(h, (size_t)ro.T_cap * B, "the rollout's log-probabilities"))) return rc;
  } else if (Tw <= ro.T_cap) {
    if ((rc = shift_in_place(h, keep, with_logp))) return rc;
  } else if ((rc = shift_and_grow(h, keep, Tw, with_logp))) {
    return rc;
  }
  ro.logp_recorded = with_logp;
  ro.T = Tw; ro.n_term = -1;
  if (keep == 0) HIPCHK(h, hipMemsetAsync(ro.term_count, 0, sizeof(int32_t), h->stream));
  double* const act0 = ro.act + (size_t)keep * B * A;
  if (A > 0) {
    if (policy == GS_POLICY_UPLOADED) {
      HIPCHK(h, hipMemcpyAsync(act0, c->actions, (size_t)T * B * A * sizeof(double), hipMemcpyHostToDevice, h->stream));
    } else if (policy == GS_POLICY_RANDOM) {
      const long long total = (long long)T * B * ((A + 3) / 4);
      hipLaunchKernelGGL(gs_k_rollout_actions, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, act0, (int)T, (int)B, (int)A, policy_seed,
                         h->EC.first_instance, c->t0);
      HIPCHK(h, hipGetLastError());
    }
  }
  // slot keep = the observation the environment stands at: with kept steps the shift has put the previous last slot there
  if (keep == 0) HIPCHK(h, hipMemcpyAsync(ro.obs_seq, h->d_obs2[h->obs_cur], B * D * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  // the steps, as gs_rollout queues them (abi_rollout.hip: which kernels do the bookkeeping, and why the policy's step is followed by
  // the small kernel): new step i is stored at s = keep + i and draws with t0 + i.  The step kernel of s > 0 looks for instances the
  // step before finished; behind a finished rollout it finds none, the small kernel after its last step having reset them.
  const bool fused = h->second_gen() && policy != GS_POLICY_MLP;
  for (int i = 0; i < T; ++i) {
    const int s = keep + i;
    double* nxt = ro.obs_seq + (size_t)(s + 1) * B * D;
    if (policy == GS_POLICY_MLP && (rc = launch_policy(h, ro.obs_seq + (size_t)s * B * D, ro.act + (size_t)s * B * A, policy_seed, (int)(c->t0 + (uint32_t)i),
                                                       with_logp ? ro.logp + (size_t)s * B : nullptr))) return rc;
    GsRolloutStep rs{ro.rew, ro.done, ro.obs_seq + (size_t)s * B * D, h->map_obs, h->d_cst, ro.term_count, ro.term_idx, ro.term_obs, ro.term_cap, h->obs_dim, s, 1};
    if ((rc = step_kernels(h, ro.act + (size_t)s * B * A, nxt, fused ? &rs : nullptr))) return rc;
    if (!fused || i == T - 1) {
      if ((rc = join_streams(h))) return rc;
      GsRolloutPostArgs pa{fused ? nullptr : ro.rew, fused ? nullptr : ro.done, nxt, h->map_obs, h->d_cst, ro.term_count, ro.term_idx, ro.term_obs, ro.term_cap, h->obs_dim, s, h->B};
      hipLaunchKernelGGL(gs_k_rollout_post, dim3(h->groups), dim3(256), 0, h->stream, h->T, h->R, h->EC, h->slab, pa);
      HIPCHK(h, hipGetLastError());
      if (h->pl && (rc = launch_load_columns(h, nxt))) return rc;
    }
  }
  if ((rc = join_streams(h))) return rc;
  // the environment now stands at slot keep + T
  if (h->gather_pending[h->obs_cur]) { HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_gather[h->obs_cur], 0)); h->gather_pending[h->obs_cur] = false; }
  HIPCHK(h, hipMemcpyAsync(h->d_obs2[h->obs_cur], ro.obs_seq + (size_t)Tw * B * D, B * D * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  if (h->rows_stale) h->last_obs = h->d_obs2[h->obs_cur];
  ro.calls += 1;
  rollout_ended(h, keep, c->t0 + (uint32_t)T);
  return GS_OK;      // asynchronous, like gs_rollout
}

int gs_rollout_window_info(gs_handle* h, gs_rollout_window_info_out* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  const gs_handle::Rollout& ro = h->ro;
  const bool collected = ro.T > 0 && ro.ended_on && ro.ended_on == ro.calls;
  out->T = ro.T; out->kept = collected ? ro.kept : 0; out->t0_next = collected ? ro.t0_next : (uint32_t)ro.T; out->T_cap = ro.T_cap;
  return GS_OK;
}

}  // extern "C"
