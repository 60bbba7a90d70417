// abi_refresh.hip -- per-minibatch targets (include/gridstep.h "per-minibatch targets"): gs_learner_refresh
// re-evaluates the selected bootstrap signals for the transitions of one minibatch under the images as they are now and writes them
// into the arrays of gs_rollout_evaluate_q_next (abi_q_next.hip) and gs_rollout_evaluate_q (abi_q.hip) at those transitions.  The
// transition -> terminal-entry map and the scratch blocks are made here and released here; the networks are the existing kernels.
#include <cmath>

#include "handle.h"

using namespace gsi;

static_assert(sizeof(gs_refresh_config) == 72, "gs_refresh_config: four int32, four doubles, a uint64, two uint32, a reserved uint64");
static_assert(sizeof(gs_refresh_config) % 8 == 0, "gs_refresh_config is padded to whole doubles");

namespace gsi __attribute__((visibility("hidden"))) {

void refresh_release(gs_handle* h) {
  gs_handle::Refresh& r = h->rfr;
  r.map.release(); r.tb.release(); r.ie.release(); r.t_tb.release(); r.pos.release(); r.count.release();
  r.own.release(); r.next.release(); r.tobs.release(); r.act.release(); r.nact.release(); r.neps.release(); r.nlp.release();
  r.t_nact.release(); r.t_neps.release(); r.t_nlp.release(); r.q.release(); r.t_q.release(); r.v.release(); r.t_v.release();
  r.pre.release(); r.t_pre.release();
  r.map_on = 0; r.n_cap = 0;
  if (r.ev) { (void)hipEventDestroy(r.ev); r.ev = nullptr; }
}

}  // namespace gsi

extern "C" {

int gs_learner_refresh(gs_handle* h, const gs_onpolicy_batch_out* batch, int32_t n, const gs_refresh_config* cfg, void* consumer_stream) {
  const char* const who = "gs_learner_refresh";
  if (!h || !batch || !cfg) return fail(h, GS_E_INVALID, "handle / batch / config is NULL");
  const std::string why = gs_refresh_check(cfg, n);
  if (!why.empty()) return fail(h, GS_E_INVALID, "%s", why.c_str());
  int rc = gae_check(h, cfg->bootstrap_mask, cfg->gamma, 0.0, cfg->reward_shift, cfg->reward_scale, "reward");
  if (rc) return rc;
  if (!batch->indices) return fail(h, GS_E_INVALID, "%s: the batch holds no indices", who);
  gs_handle::Rollout& ro = h->ro;
  gs_handle::Refresh& r = h->rfr;
  gs_handle::QNext& qn = h->qn;
  gs_handle::QTrack& qt = h->qt;
  const gs_handle::Value& val = h->critic[0].net;
  const int groups = cfg->groups;
  const bool g_pol = groups & GS_REFRESH_TD_POLICY, g_tgt = groups & GS_REFRESH_Q_TARGET, g_tdv = groups & GS_REFRESH_TD_VALUE, g_adv = groups & GS_REFRESH_Q_ADV;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "%s: no rollout has been collected on this handle", who);
  if (!h->qnet[0].net.set && !h->qnet[1].net.set) return fail(h, GS_E_STATE, "%s before gs_q_mlp_set", who);
  if (g_pol) {
    if (!policy_rows_ready(h))
      return fail(h, GS_E_STATE, "%s: GS_REFRESH_TD_POLICY needs an installed policy with GS_COMPUTE_F32 and GS_HEAD_GAUSSIAN_TANH", who);
    if (!q_next_current(h)) return fail(h, GS_E_STATE, "%s: GS_REFRESH_TD_POLICY replaces rows of gs_rollout_evaluate_q_next, which has not run on the last rollout", who);
    if (qn.mask != cfg->bootstrap_mask)
      return fail(h, GS_E_STATE, "%s: GS_REFRESH_TD_POLICY under bootstrap_mask %d, the last gs_rollout_evaluate_q_next ran under %d", who, cfg->bootstrap_mask, qn.mask);
  }
  if ((g_tgt || g_tdv || g_adv) && !q_current(h))
    return fail(h, GS_E_STATE, "%s: the groups replace rows of gs_rollout_evaluate_q, which has not run on the last rollout", who);
  if ((g_tdv || g_adv) && !h->critic[0].net.set) return fail(h, GS_E_STATE, "%s: GS_REFRESH_TD_VALUE / GS_REFRESH_Q_ADV before gs_value_mlp_set", who);
  GS_ENTER(h);
  const int B = h->B, D = h->obs_dim, A = h->action_dim;
  const long long N = (long long)ro.T * B;
  const size_t cap = (size_t)ro.T_cap * B, tc = (size_t)ro.term_cap;
  const GsRefreshSizes S = gs_refresh_sizes(n, D, A);
  const bool terms = cfg->bootstrap_mask && ro.term_cap > 0 && (g_pol || g_tdv);
  // scratch for n rows, all or none; the map of this rollout
  if (S.rows > r.n_cap) {
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (what is queued may still read the old blocks)
    r.n_cap = 0;
    if ((rc = alloc_all(h, "the refresh's scratch over a minibatch", r.tb.want(S.pairs), r.ie.want(S.pairs), r.t_tb.want(S.pairs), r.pos.want(S.rows), r.count.want(1),
                        r.own.want(S.obs), r.next.want(S.obs), r.tobs.want(S.obs), r.act.want(S.act), r.nact.want(S.act), r.neps.want(S.act), r.nlp.want(S.rows),
                        r.t_nact.want(S.act), r.t_neps.want(S.act), r.t_nlp.want(S.rows), r.q.want(S.twin), r.t_q.want(S.twin), r.v.want(S.rows), r.t_v.want(S.rows),
                        r.pre.want(S.pre), r.t_pre.want(S.pre))))
      return rc;
    r.n_cap = S.rows;
  }
  if (r.map_on != ro.calls) {
    r.map_on = 0;
    if ((rc = r.map.grow(h, cap, "the refresh's terminal map"))) return rc;
    if ((rc = terminal_map_fill(h, r.map.p, N))) return rc;
    r.map_on = ro.calls;
  }
  const int32_t* const idx = batch->indices;
  if (terms) {
    GsRefreshTermsArgs T{idx, ro.done, r.map, ro.term_idx, r.ie, r.t_tb, r.pos, r.count, N, n, cfg->bootstrap_mask};
    hipLaunchKernelGGL(gs_k_refresh_terms, dim3(1), dim3(GS_RF_TERM_THREADS), 0, h->stream, T);
    HIPCHK(h, hipGetLastError());
  }
  {
    GsRefreshRowsArgs G{};
    G.idx = idx; G.obs_seq = ro.obs_seq; G.actions = ro.act; G.term_obs = ro.term_obs; G.N = N;
    G.ie = terms ? r.ie.p : nullptr; G.count = terms ? r.count.p : nullptr; G.term = terms ? r.tobs.p : nullptr;
    G.own = (g_tgt || g_adv) ? r.own.p : nullptr; G.next = (g_pol || g_tdv) ? r.next.p : nullptr;
    G.act = (g_tgt || g_adv) ? r.act.p : nullptr; G.tb = g_pol ? r.tb.p : nullptr;
    G.n = n; G.B = B; G.D = D; G.A = A; G.W = std::max(std::max(D, A), 2);
    const long long threads = (long long)n * G.W;
    hipLaunchKernelGGL(gs_k_refresh_rows, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
  }
  const unsigned row_blocks = (unsigned)((n + 255) / 256);
  if (g_pol) {
    if ((rc = rows_kernels_lds_cap(h))) return rc;
    const PolicyNoise noise{cfg->stochastic, cfg->draw, cfg->seed};
    if ((rc = launch_policy_rows(h, noise, r.next, n, nullptr, r.tb, GS_QN_ROLLOUT_TAG, r.pre, r.nact, r.neps, r.nlp))) return rc;
    if (terms && (rc = launch_policy_rows(h, noise, r.tobs, n, r.count, r.t_tb, GS_QN_TERMINAL_TAG, r.t_pre, r.t_nact, r.t_neps, r.t_nlp))) return rc;
    GsRefreshTdPolicyArgs G{};
    for (int w = 0; w < 2; ++w) {
      const gs_handle::QNet& Q = h->qnet[w];
      if (!Q.net.set) continue;
      if ((rc = launch_q_rows(h, Q, Q.TL, r.next, r.nact, n, nullptr, r.q + (size_t)w * n))) return rc;
      G.s_q[w] = r.q + (size_t)w * n; G.q[w] = qn.q + (size_t)w * cap;
      if (terms) {
        if ((rc = launch_q_rows(h, Q, Q.TL, r.tobs, r.t_nact, n, r.count, r.t_q + (size_t)w * n))) return rc;
        G.st_q[w] = r.t_q + (size_t)w * n; G.t_q[w] = qn.t_q + (size_t)w * tc;
      }
    }
    G.idx = idx; G.pos = terms ? r.pos.p : nullptr; G.ie = r.ie;
    G.s_pre = r.pre; G.s_act = r.nact; G.s_eps = r.neps; G.s_lp = r.nlp;
    G.st_pre = r.t_pre; G.st_act = r.t_nact; G.st_eps = r.t_neps; G.st_lp = r.t_nlp;
    G.rew = ro.rew; G.done = ro.done;
    G.pre = qn.pre; G.act = qn.act; G.eps = qn.eps; G.lp = qn.lp; G.q_min = qn.q_min; G.td = qn.td;
    G.t_pre = qn.t_pre; G.t_act = qn.t_act; G.t_eps = qn.t_eps; G.t_lp = qn.t_lp; G.t_q_min = qn.t_q_min; G.t_value = qn.t_value;
    G.N = N; G.n = n; G.A = A;
    G.gamma = cfg->gamma; G.alpha = cfg->alpha; G.reward_shift = cfg->reward_shift; G.reward_scale = cfg->reward_scale;
    hipLaunchKernelGGL(gs_k_refresh_td_policy, dim3(row_blocks), dim3(256), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
  }
  // the twins on the stored (s_j, a_j) under image `src` (0 online, 1 target), combined into q[src] / q_min[src] (and q_adv with `values`)
  auto twins_on_own = [&](int src, const double* values) -> int {
    GsRefreshCombineArgs C{};
    for (int w = 0; w < 2; ++w) {
      const gs_handle::QNet& Q = h->qnet[w];
      if (!Q.net.set) continue;
      if (int rc2 = launch_q_rows(h, Q, src ? Q.TL : Q.qargs.L, r.own, r.act, n, nullptr, r.q + (size_t)w * n)) return rc2;
      C.s_q[w] = r.q + (size_t)w * n; C.q[w] = qt.q + (size_t)(2 * src + w) * cap;
    }
    C.idx = idx; C.values = values; C.q_min = qt.q_min + (size_t)src * cap; C.q_adv = qt.q_adv; C.N = N; C.n = n;
    hipLaunchKernelGGL(gs_k_refresh_combine, dim3(row_blocks), dim3(256), 0, h->stream, C);
    HIPCHK(h, hipGetLastError());
    return GS_OK;
  };
  if (g_tgt && (rc = twins_on_own(1, nullptr))) return rc;
  if (g_tdv) {
    if ((rc = launch_value_rows(h, val, r.next, r.v, n))) return rc;
    if (terms && (rc = launch_value_rows(h, val, r.tobs, r.t_v, n, r.count))) return rc;
    GsRefreshTdValueArgs G{idx, terms ? r.pos.p : nullptr, r.v, r.t_v, ro.rew, ro.done, qt.td, N, n, 0, cfg->gamma, cfg->reward_shift, cfg->reward_scale};
    hipLaunchKernelGGL(gs_k_refresh_td_value, dim3(row_blocks), dim3(256), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
  }
  if (g_adv) {
    if ((rc = launch_value_rows(h, val, r.own, r.v, n))) return rc;
    if ((rc = twins_on_own(0, r.v))) return rc;
  }
  return publish(h, h->stream, r.ev, consumer_stream);
}

}  // extern "C"
