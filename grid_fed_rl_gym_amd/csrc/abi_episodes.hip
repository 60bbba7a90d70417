// abi_episodes.hip -- episode accounting (include/gridstep.h): gs_rollout_episodes over the last rollout (the
// four kernels of kernels_episodes.hip), the views of what it left, gs_episodes_clear.  The handle's episode track (handle.h) is made
// here and released here (episodes_release).
#include <cmath>

#include "handle.h"

using namespace gsi;

static_assert(sizeof(GsEpisodeStats) == sizeof(gs_episode_stats), "GsEpisodeStats is gs_episode_stats as the kernels write it");
static_assert(sizeof(gs_episode_config) == 24, "gs_episode_config: four int32 and a double");
static_assert(GS_EP_CONTINUE == GS_EPISODES_CONTINUE && GS_EP_UNKNOWN == GS_EPISODES_UNKNOWN && GS_EP_PARTIAL == GS_EPISODE_PARTIAL,
              "the kernels' copies of the public constants");

namespace gsi __attribute__((visibility("hidden"))) {

void episodes_release(gs_handle* h, bool keep_carries) {
  gs_handle::EpisodeTrack& ep = h->ep;
  ep.e_idx.release(); ep.e_ret.release(); ep.e_len.release(); ep.e_ord.release(); ep.e_flags.release();
  ep.e_cost.release(); ep.e_viol.release(); ep.e_anyv.release();
  ep.cap = 0;
  if (keep_carries) return;
  ep.c_ret.release(); ep.c_len.release(); ep.c_ord.release(); ep.c_partial.release(); ep.c_cost.release(); ep.c_viol.release(); ep.c_anyv.release();
  ep.seg.release(); ep.n_ep.release(); ep.stats.release();
  if (ep.ev) { (void)hipEventDestroy(ep.ev); ep.ev = nullptr; }
  ep.live = false; ep.with_costs = 0; ep.accounted_on = 0; ep.moves_at = 0;
}

}  // namespace gsi

// gs_rollout_episodes has run on the rollout the handle holds
static bool episodes_current(const gs_handle* h) { return h->ep.accounted_on && h->ep.accounted_on == h->ro.calls; }

extern "C" {

int gs_rollout_episodes(gs_handle* h, const gs_episode_config* cfg) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  gs_episode_config def{(int32_t)sizeof(gs_episode_config), GS_EPISODES_CONTINUE, 0, 0, -1000.0};
  if (!cfg) cfg = &def;
  if (cfg->struct_size != (int32_t)sizeof(gs_episode_config))
    return fail(h, GS_E_INVALID, "gs_episode_config struct_size %d != %d", cfg->struct_size, (int)sizeof(gs_episode_config));
  if (cfg->start != GS_EPISODES_CONTINUE && cfg->start != GS_EPISODES_FRESH && cfg->start != GS_EPISODES_UNKNOWN)
    return fail(h, GS_E_INVALID, "gs_episode_config start = %d outside 0 .. 2", cfg->start);
  if (std::isnan(cfg->success_return) || cfg->success_return == INFINITY)
    return fail(h, GS_E_INVALID, "gs_episode_config success_return must be finite or -inf");
  gs_handle::Rollout& ro = h->ro;
  gs_handle::EpisodeTrack& ep = h->ep;
  const int with_costs = cfg->with_costs != 0;
  if (ro.T <= 0 || ro.calls == 0) return fail(h, GS_E_STATE, "gs_rollout_episodes: no rollout has been collected on this handle");
  if (ep.live && ep.accounted_on == ro.calls) return fail(h, GS_E_STATE, "gs_rollout_episodes: the last rollout has already been accounted");
  if (cfg->start == GS_EPISODES_CONTINUE) {
    if (ro.ended_on == ro.calls && ro.kept > 0)
      return fail(h, GS_E_STATE, "gs_rollout_episodes: GS_EPISODES_CONTINUE on a window whose first %d steps were kept from the rollout before "
                                 "(gs_rollout_continue): they would be counted twice.  GS_EPISODES_FRESH accounts the window as it stands", ro.kept);
    if (!ep.live) return fail(h, GS_E_STATE, "gs_rollout_episodes: GS_EPISODES_CONTINUE without an episode track (start one with FRESH or UNKNOWN)");
    if (ro.calls != ep.accounted_on + 1)
      return fail(h, GS_E_STATE, "gs_rollout_episodes: GS_EPISODES_CONTINUE, but the rollout before the last one was not accounted (%llu rollouts since)",
                  (unsigned long long)(ro.calls - ep.accounted_on));
    if (h->env_moves != ep.moves_at)
      return fail(h, GS_E_STATE, "gs_rollout_episodes: GS_EPISODES_CONTINUE, but the environment was moved outside gs_rollout since the accounted rollout "
                                 "(gs_reset, gs_set_state, gs_step or an upload of state)");
    if (with_costs != ep.with_costs)
      return fail(h, GS_E_STATE, "gs_rollout_episodes: GS_EPISODES_CONTINUE with with_costs = %d on a track started with %d", with_costs, ep.with_costs);
  }
  if (with_costs && (!h->cc.computed_on || h->cc.computed_on != ro.calls))
    return fail(h, GS_E_STATE, "gs_rollout_episodes: with_costs, but gs_rollout_costs has not run on the last rollout");
  GS_ENTER(h);
  int rc = GS_OK;
  const size_t B = (size_t)h->B, cap = (size_t)ro.term_cap;
  // the carries and the scratch: sized by B, all or none.  (A refusal from here on is GS_E_NOMEM / GS_E_HIP, not a rule of the contract.)
  if (!ep.c_ret && (rc = alloc_all(h, "the episode track's carries", ep.c_ret.want(B), ep.c_len.want(B), ep.c_ord.want(B), ep.c_partial.want((B + 3) / 4),
                                   ep.seg.want(B), ep.n_ep.want(1), ep.stats.want(1)))) return rc;
  if (with_costs && !ep.c_cost &&
      (rc = alloc_all(h, "the episode track's cost carries", ep.c_cost.want(3 * B), ep.c_viol.want(3 * B), ep.c_anyv.want(B)))) return rc;
  // the list: sized by the rollout's terminal list, released with it; all or none
  if (!ep.e_idx || ep.cap != cap) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if ((rc = alloc_all(h, "the episode list", ep.e_idx.want(2 * cap), ep.e_ret.want(cap), ep.e_len.want(cap), ep.e_ord.want(cap), ep.e_flags.want(cap)))) {
      ep.e_cost.release(); ep.e_viol.release(); ep.e_anyv.release(); ep.cap = 0;
      return rc;
    }
    ep.e_cost.release(); ep.e_viol.release(); ep.e_anyv.release();
    ep.cap = cap;
  }
  if (with_costs && !ep.e_cost && (rc = alloc_all(h, "the episode list's costs", ep.e_cost.want(3 * cap), ep.e_viol.want(3 * cap), ep.e_anyv.want(cap)))) return rc;

  GsEpisodeArgs a{};
  a.rew = ro.rew; a.done = ro.done; a.T = ro.T; a.B = h->B; a.cap = (int32_t)cap; a.start = cfg->start;
  if (with_costs) { a.costs = h->cc.costs; a.margins = h->cc.margins; a.chan_stride = (long long)ro.T * h->B; }
  a.c_ret = ep.c_ret; a.c_len = ep.c_len; a.c_ord = ep.c_ord; a.c_partial = ep.c_partial;
  if (with_costs) { a.c_cost = ep.c_cost; a.c_viol = ep.c_viol; a.c_anyv = ep.c_anyv; a.e_cost = ep.e_cost; a.e_viol = ep.e_viol; a.e_anyv = ep.e_anyv; }
  a.seg = ep.seg; a.n_ep = ep.n_ep;
  a.e_idx = ep.e_idx; a.e_ret = ep.e_ret; a.e_len = ep.e_len; a.e_ord = ep.e_ord; a.e_flags = ep.e_flags;
  a.stats = ep.stats; a.success_return = cfg->success_return;
  ep.accounted_on = 0;      // (until every launch is queued: a failure below leaves a track that only FRESH / UNKNOWN can restart)
  const dim3 per_instance((unsigned)((B + 255) / 256));
  hipLaunchKernelGGL(gs_k_ep_count, per_instance, dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(gs_k_ep_offsets, dim3(1), dim3(GS_EP_SCAN_THREADS), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  if (with_costs) hipLaunchKernelGGL(gs_k_ep_accumulate_costs, per_instance, dim3(256), 0, h->stream, a);
  else hipLaunchKernelGGL(gs_k_ep_accumulate, per_instance, dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(gs_k_ep_stats, dim3(1), dim3(GS_EP_STAT_THREADS), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  ep.live = true; ep.with_costs = with_costs; ep.accounted_on = ro.calls; ep.moves_at = h->env_moves;
  return GS_OK;
}

int gs_rollout_episodes_view(gs_handle* h, gs_rollout_episodes_dev* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Rollout& ro = h->ro;
  gs_handle::EpisodeTrack& ep = h->ep;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  if (!episodes_current(h)) return fail(h, GS_E_STATE, "gs_rollout_episodes has not run on the last rollout");
  int rc = rollout_finish(h);
  if (rc) return rc;
  if ((rc = publish(h, h->stream, ep.ev, consumer_stream))) return rc;
  *out = gs_rollout_episodes_dev{};
  out->n_episodes = ro.n_term; out->B = h->B; out->with_costs = ep.with_costs; out->cost_stride = (int32_t)ep.cap;
  out->episode_index = ep.e_idx; out->episode_return = ep.e_ret; out->episode_length = ep.e_len; out->episode_ordinal = ep.e_ord;
  out->episode_flags = ep.e_flags; out->stats = (const gs_episode_stats*)ep.stats.p;
  out->ep_return = ep.c_ret; out->ep_length = ep.c_len; out->ep_ordinal = ep.c_ord; out->ep_partial = (const uint8_t*)ep.c_partial.p;
  if (ep.with_costs) {
    out->episode_cost = ep.e_cost; out->episode_violating = ep.e_viol; out->episode_any_violating = ep.e_anyv;
    out->ep_cost = ep.c_cost; out->ep_violating = ep.c_viol; out->ep_any_violating = ep.c_anyv;
  }
  return GS_OK;
}

int gs_rollout_episodes_download(gs_handle* h, const gs_rollout_episodes_host* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Rollout& ro = h->ro;
  gs_handle::EpisodeTrack& ep = h->ep;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  if (!episodes_current(h)) return fail(h, GS_E_STATE, "gs_rollout_episodes has not run on the last rollout");
  const bool cost_asked = out->episode_cost || out->episode_violating || out->episode_any_violating || out->ep_cost || out->ep_violating || out->ep_any_violating;
  if (cost_asked && !ep.with_costs) return fail(h, GS_E_STATE, "gs_rollout_episodes ran without costs on the last rollout");
  int rc = rollout_finish(h);
  if (rc) return rc;
  const size_t n = (size_t)ro.n_term, B = (size_t)h->B, cap = ep.cap;
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  auto copy = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, d2h, h->stream) : hipSuccess;
  };
  if (out->n_episodes) *out->n_episodes = ro.n_term;
  HIPCHK(h, copy(out->episode_index, ep.e_idx, 2 * n * sizeof(int32_t)));
  HIPCHK(h, copy(out->episode_return, ep.e_ret, n * sizeof(double)));
  HIPCHK(h, copy(out->episode_length, ep.e_len, n * sizeof(int32_t)));
  HIPCHK(h, copy(out->episode_ordinal, ep.e_ord, n * sizeof(int32_t)));
  HIPCHK(h, copy(out->episode_flags, ep.e_flags, n * sizeof(int32_t)));
  for (size_t c = 0; c < 3 && ep.with_costs; ++c) {
    HIPCHK(h, copy(out->episode_cost ? out->episode_cost + c * n : nullptr, ep.e_cost + c * cap, n * sizeof(double)));
    HIPCHK(h, copy(out->episode_violating ? out->episode_violating + c * n : nullptr, ep.e_viol + c * cap, n * sizeof(int32_t)));
  }
  if (ep.with_costs) HIPCHK(h, copy(out->episode_any_violating, ep.e_anyv, n * sizeof(int32_t)));
  HIPCHK(h, copy(out->stats, ep.stats, sizeof(gs_episode_stats)));
  HIPCHK(h, copy(out->ep_return, ep.c_ret, B * sizeof(double)));
  HIPCHK(h, copy(out->ep_length, ep.c_len, B * sizeof(int32_t)));
  HIPCHK(h, copy(out->ep_ordinal, ep.c_ord, B * sizeof(int32_t)));
  HIPCHK(h, copy(out->ep_partial, ep.c_partial, B));
  if (ep.with_costs) {
    HIPCHK(h, copy(out->ep_cost, ep.c_cost, 3 * B * sizeof(double)));
    HIPCHK(h, copy(out->ep_violating, ep.c_viol, 3 * B * sizeof(int32_t)));
    HIPCHK(h, copy(out->ep_any_violating, ep.c_anyv, B * sizeof(int32_t)));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

int gs_episodes_clear(gs_handle* h) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));      // (what is queued may still write the track)
  episodes_release(h);
  return GS_OK;
}

}  // extern "C"
