// abi_q_next.hip -- policy-action TD targets (include/gridstep.h "policy-action TD targets"): what
// gs_rollout_evaluate_q_next makes of the last rollout (the installed policy's action and log-probability at every next state, the
// target twins' values of it, their minimum and the Bellman target), its view and download, and which target the Q learner reads
// (gs_q_set_target_source).  The arrays over the rollout are made here and released here.
#include <cmath>

#include "handle.h"

using namespace gsi;

static_assert(sizeof(gs_q_next_config) == 64, "gs_q_next_config: four int32, four doubles, a uint64, two uint32");

namespace gsi __attribute__((visibility("hidden"))) {

void q_next_rollout_release(gs_handle* h) {
  gs_handle::QNext& t = h->qn;
  t.pre.release(); t.act.release(); t.eps.release(); t.lp.release(); t.q.release(); t.q_min.release(); t.td.release();
  t.t_pre.release(); t.t_act.release(); t.t_eps.release(); t.t_lp.release(); t.t_q.release(); t.t_q_min.release(); t.t_value.release();
  t.evaluated_on = 0; t.with_terms = false;
  if (t.ev) { (void)hipEventDestroy(t.ev); t.ev = nullptr; }
}

}  // namespace gsi

extern "C" {

int gs_rollout_evaluate_q_next(gs_handle* h, const gs_q_next_config* cfg) {
  if (!h || !cfg) return fail(h, GS_E_INVALID, "handle / config is NULL");
  if (cfg->struct_size != (int32_t)sizeof(gs_q_next_config))
    return fail(h, GS_E_INVALID, "gs_q_next_config struct_size %d != %d", cfg->struct_size, (int)sizeof(gs_q_next_config));
  int rc = gae_check(h, cfg->bootstrap_mask, cfg->gamma, 0.0, cfg->reward_shift, cfg->reward_scale, "reward");
  if (rc) return rc;
  if (!std::isfinite(cfg->alpha) || cfg->alpha < 0.0) return fail(h, GS_E_INVALID, "gs_rollout_evaluate_q_next: alpha = %g is not a finite value >= 0", cfg->alpha);
  if (cfg->stochastic != 0 && cfg->stochastic != 1) return fail(h, GS_E_INVALID, "gs_rollout_evaluate_q_next: stochastic = %d outside {0, 1}", cfg->stochastic);
  gs_handle::Rollout& ro = h->ro;
  gs_handle::QNext& t = h->qn;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "gs_rollout_evaluate_q_next: no rollout has been collected on this handle");
  if (!h->qnet[0].net.set && !h->qnet[1].net.set) return fail(h, GS_E_STATE, "gs_rollout_evaluate_q_next before gs_q_mlp_set");
  if (!policy_rows_ready(h))
    return fail(h, GS_E_STATE, "gs_rollout_evaluate_q_next: it needs an installed policy with GS_COMPUTE_F32 and GS_HEAD_GAUSSIAN_TANH");
  GS_ENTER(h);
  const size_t B = h->B, D = h->obs_dim, A = h->action_dim, cap = (size_t)ro.T_cap * B, TB = (size_t)ro.T * B, tc = (size_t)ro.term_cap;
  t.evaluated_on = 0;        // (until every launch is queued)
  if (!t.pre && (rc = alloc_all(h, "the policy-action targets' arrays over the rollout", t.pre.want(cap * 2 * A), t.act.want(cap * A), t.eps.want(cap * A), t.lp.want(cap),
                                t.q.want(2 * cap), t.q_min.want(cap), t.td.want(cap), t.t_pre.want(tc * 2 * A), t.t_act.want(tc * A), t.t_eps.want(tc * A), t.t_lp.want(tc),
                                t.t_q.want(2 * tc), t.t_q_min.want(tc), t.t_value.want(tc))))
    return rc;
  if ((rc = rows_kernels_lds_cap(h))) return rc;
  const bool terms = cfg->bootstrap_mask && ro.term_cap > 0;
  const double* const next_obs = ro.obs_seq + B * D;      // row (t + 1, b) for transition (t, b)
  GsQNextTdArgs G{};
  const PolicyNoise noise{cfg->stochastic, cfg->draw, cfg->seed};
  if ((rc = launch_policy_rows(h, noise, next_obs, (long long)TB, nullptr, nullptr, GS_QN_ROLLOUT_TAG, t.pre, t.act, t.eps, t.lp))) return rc;
  if (terms && (rc = launch_policy_rows(h, noise, ro.term_obs, ro.term_cap, ro.term_count, ro.term_idx, GS_QN_TERMINAL_TAG, t.t_pre, t.t_act, t.t_eps, t.t_lp))) return rc;
  for (int w = 0; w < 2; ++w) {
    const gs_handle::QNet& Q = h->qnet[w];
    if (!Q.net.set) continue;
    G.q[w] = t.q + (size_t)w * cap; G.term_q[w] = t.t_q + (size_t)w * tc;
    if ((rc = launch_q_rows(h, Q, Q.TL, next_obs, t.act, (long long)TB, nullptr, t.q + (size_t)w * cap))) return rc;
    if (terms && (rc = launch_q_rows(h, Q, Q.TL, ro.term_obs, t.t_act, ro.term_cap, ro.term_count, t.t_q + (size_t)w * tc))) return rc;
  }
  G.lp = t.lp; G.rew = ro.rew; G.done = ro.done; G.term_lp = t.t_lp; G.term_count = ro.term_count; G.term_idx = ro.term_idx;
  G.q_min = t.q_min; G.term_q_min = t.t_q_min; G.term_value = t.t_value; G.td = t.td;
  G.T = (int32_t)ro.T; G.B = h->B; G.mask = cfg->bootstrap_mask; G.term_cap = ro.term_cap; G.phase = 0;
  G.gamma = cfg->gamma; G.alpha = cfg->alpha; G.reward_shift = cfg->reward_shift; G.reward_scale = cfg->reward_scale;
  hipLaunchKernelGGL(gs_k_q_next_td, dim3((unsigned)((TB + 255) / 256)), dim3(256), 0, h->stream, G);
  HIPCHK(h, hipGetLastError());
  if (terms) {
    G.phase = 1;
    hipLaunchKernelGGL(gs_k_q_next_td, dim3((unsigned)((tc + 255) / 256)), dim3(256), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
  }
  t.with_terms = terms;
  t.mask = cfg->bootstrap_mask;
  t.evaluated_on = ro.calls;
  return GS_OK;
}

int gs_rollout_q_next_view(gs_handle* h, gs_rollout_q_next* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Rollout& ro = h->ro;
  gs_handle::QNext& t = h->qn;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  if (!q_next_current(h)) return fail(h, GS_E_STATE, "gs_rollout_evaluate_q_next has not run on the last rollout");
  GS_ENTER(h);
  int rc = publish(h, h->stream, t.ev, consumer_stream);
  if (rc) return rc;
  const size_t cap = (size_t)ro.T_cap * h->B, tc = (size_t)ro.term_cap;
  *out = gs_rollout_q_next{};
  out->T = ro.T; out->B = h->B; out->rows_per_tile = GS_VAL_ROWS; out->action_dim = h->action_dim; out->terminal_capacity = ro.term_cap;
  out->next_pre_head = t.pre; out->next_actions = t.act; out->next_noise = t.eps; out->next_log_probs = t.lp; out->q_next_min = t.q_min; out->td_target = t.td;
  if (t.with_terms) { out->term_pre_head = t.t_pre; out->term_actions = t.t_act; out->term_noise = t.t_eps; out->term_log_probs = t.t_lp; out->term_q_min = t.t_q_min; out->term_value = t.t_value; }
  for (int w = 0; w < 2; ++w) {
    if (!h->qnet[w].net.set) continue;
    out->installed |= 1 << w;
    out->q_next[w] = t.q + (size_t)w * cap;
    if (t.with_terms) out->term_q[w] = t.t_q + (size_t)w * tc;
  }
  return GS_OK;
}

int gs_rollout_q_next_download(gs_handle* h, const gs_rollout_q_next_host* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Rollout& ro = h->ro;
  gs_handle::QNext& t = h->qn;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  if (!q_next_current(h)) return fail(h, GS_E_STATE, "gs_rollout_evaluate_q_next has not run on the last rollout");
  GS_ENTER(h);
  int rc = rollout_finish(h);      // (ro.n_term: how many entries the terminal list holds)
  if (rc) return rc;
  const size_t A = h->action_dim, cap = (size_t)ro.T_cap * h->B, tc = (size_t)ro.term_cap, TB = (size_t)ro.T * h->B;
  const size_t nt = t.with_terms ? (size_t)std::max(ro.n_term, 0) : 0;
  auto copy = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
  };
  HIPCHK(h, copy(out->next_pre_head, t.pre, TB * 2 * A * sizeof(float)));
  HIPCHK(h, copy(out->next_actions, t.act, TB * A * sizeof(double)));
  HIPCHK(h, copy(out->next_noise, t.eps, TB * A * sizeof(double)));
  HIPCHK(h, copy(out->next_log_probs, t.lp, TB * sizeof(double)));
  HIPCHK(h, copy(out->q_next_min, t.q_min, TB * sizeof(double)));
  HIPCHK(h, copy(out->td_target, t.td, TB * sizeof(double)));
  HIPCHK(h, copy(out->term_pre_head, t.t_pre, nt * 2 * A * sizeof(float)));
  HIPCHK(h, copy(out->term_actions, t.t_act, nt * A * sizeof(double)));
  HIPCHK(h, copy(out->term_noise, t.t_eps, nt * A * sizeof(double)));
  HIPCHK(h, copy(out->term_log_probs, t.t_lp, nt * sizeof(double)));
  HIPCHK(h, copy(out->term_q_min, t.t_q_min, nt * sizeof(double)));
  HIPCHK(h, copy(out->term_value, t.t_value, nt * sizeof(double)));
  for (int w = 0; w < 2; ++w) {
    if (!h->qnet[w].net.set) continue;
    HIPCHK(h, copy(out->q_next[w], t.q + (size_t)w * cap, TB * sizeof(double)));
    HIPCHK(h, copy(out->term_q[w], t.t_q + (size_t)w * tc, nt * sizeof(double)));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

int gs_q_set_target_source(gs_handle* h, int32_t source) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (source != GS_Q_TARGET_VALUE && source != GS_Q_TARGET_POLICY) return fail(h, GS_E_INVALID, "gs_q_set_target_source: unknown source %d", source);
  h->qn.target_source = source;
  return GS_OK;
}

int gs_q_get_target_source(gs_handle* h, int32_t* source) {
  if (!h || !source) return fail(h, GS_E_INVALID, "handle / source is NULL");
  *source = h->qn.target_source;
  return GS_OK;
}

}  // extern "C"
