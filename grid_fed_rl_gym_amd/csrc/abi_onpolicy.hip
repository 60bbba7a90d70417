// abi_onpolicy.hip -- on-policy rollouts (include/gridstep.h): the value network (gs_value_mlp_*), the critic track (a value
// network's values, advantages and returns over the last rollout: gs_rollout_evaluate here, gs_rollout_evaluate_costs in
// abi_costs.hip) and the views of what the reward critic and the policy kernels' log-probability output left.  The value networks
// and every critic's arrays are made here and released here (the log-probabilities are allocated by gs_rollout, abi_rollout.hip,
// which writes them).
#include <cmath>
#include <string>

#include "handle.h"

using namespace gsi;

namespace gsi __attribute__((visibility("hidden"))) {

void value_release(gs_handle* h) {
  for (gs_handle::Critic& c : h->critic) { c.net.blob.release(); c.net.out.release(); c.net.set = false; }
}

void onpolicy_release(gs_handle* h) {
  h->ro.logp.release();
  for (gs_handle::Critic& c : h->critic) { c.values.release(); c.term_values.release(); c.adv.release(); c.ret.release(); c.evaluated_on = 0; }
  if (h->ro.ev_eval) { (void)hipEventDestroy(h->ro.ev_eval); h->ro.ev_eval = nullptr; }
  h->ro.logp_recorded = false;
}

// what gs_value_mlp_set and gs_cost_value_mlp_set (abi_costs.hip) share: `p` has passed gs_value_check; NULL removes the network
int value_install(gs_handle* h, gs_handle::Value& val, const gs_policy_mlp* p, const gs_policy_mlp_opts* o, bool want_out) {
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k <= GS_COST_CHANNELS; ++k)
    if (&h->critic[k].net == &val) learner_drop(h, 1 + k);      // (a learner trains the network it was created on)
  val.blob.release();
  val.set = false;
  if (!p) return GS_OK;
  int rc = want_out ? val.out.grow(h, (size_t)h->B, "the value network's output") : GS_OK;
  if (rc) return rc;
  ScalarNet net;
  if ((rc = scalar_net_install(h, val, (const void*)gs_k_value_mlp_f32, *p, *o, net))) return rc;
  val.args = GsValueArgs{};
  scalar_net_args(val.args, *p, net);
  val.args.D = h->obs_dim;
  val.set = true;
  return GS_OK;
}

int gae_check(gs_handle* h, int bootstrap_mask, double gamma, double lambda, double shift, double scale, const char* signal) {
  if (bootstrap_mask < 0 || bootstrap_mask > 3) return fail(h, GS_E_INVALID, "bootstrap_mask %d outside 0 .. 3", bootstrap_mask);
  if (!std::isfinite(gamma) || !std::isfinite(lambda) || !std::isfinite(shift) || !std::isfinite(scale))
    return fail(h, GS_E_INVALID, "gamma / lambda / %s_shift / %s_scale must be finite", signal, signal);
  return GS_OK;
}

int critic_evaluate(gs_handle* h, gs_handle::Critic& c, const double* signal, int bootstrap_mask, double gamma, double lambda, double shift, double scale) {
  gs_handle::Rollout& ro = h->ro;
  const size_t B = h->B, T = ro.T, cap = ro.T_cap;
  int rc = GS_OK;
  // all four or none: a later call must not find `values` and launch on the others
  if (!c.values && (rc = alloc_all(h, "a critic's arrays over the rollout", c.values.want((cap + 1) * B), c.term_values.want((size_t)ro.term_cap),
                                   c.adv.want(cap * B), c.ret.want(cap * B)))) return rc;
  if ((rc = launch_value_rows(h, c.net, ro.obs_seq, c.values, (long long)((T + 1) * B)))) return rc;
  // the terminal rows: launched over the list's capacity, the count read on the device; every value also goes to its (t, b) in
  // `ret`, where gs_k_gae looks for it before it writes the return there
  if ((rc = launch_value_rows(h, c.net, ro.term_obs, c.term_values, ro.term_cap, ro.term_count, ro.term_idx, c.ret, (int)T))) return rc;
  GsGaeArgs g{c.values, signal, ro.done, c.adv, c.ret, (int32_t)T, h->B, bootstrap_mask, 0, gamma, lambda, shift, scale};
  hipLaunchKernelGGL(gs_k_gae, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, g);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

int critic_download(gs_handle* h, const gs_handle::Critic& c, double* values, double* term_values, double* adv, double* ret) {
  const gs_handle::Rollout& ro = h->ro;
  const size_t TB = (size_t)ro.T * h->B * sizeof(double), B8 = (size_t)h->B * sizeof(double);
  if (values) HIPCHK(h, hipMemcpyAsync(values, c.values, TB + B8, hipMemcpyDeviceToHost, h->stream));
  if (term_values && ro.n_term) HIPCHK(h, hipMemcpyAsync(term_values, c.term_values, (size_t)ro.n_term * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (adv) HIPCHK(h, hipMemcpyAsync(adv, c.adv, TB, hipMemcpyDeviceToHost, h->stream));
  if (ret) HIPCHK(h, hipMemcpyAsync(ret, c.ret, TB, hipMemcpyDeviceToHost, h->stream));
  return GS_OK;
}

}  // namespace gsi

extern "C" {
int gs_rollout_set_log_probs(gs_handle* h, int32_t on) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  h->ro.record_logp = on != 0;
  return GS_OK;
}

// ---- the value network (policy.h, kernels_value.hip) -----------------------------------------------------------------------------
int gs_value_mlp_check(const gs_policy_mlp* p, const gs_policy_mlp_opts* o, int32_t obs_dim) {
  const std::string why = gs_value_check(p, o, obs_dim);
  return why.empty() ? GS_OK : fail(nullptr, GS_E_INVALID, "%s", why.c_str());
}

int gs_value_mlp_set(gs_handle* h, const gs_policy_mlp* p, const gs_policy_mlp_opts* o) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (p) {         // (a refused network leaves the installed one in place)
    const std::string why = gs_value_check(p, o, h->obs_dim);
    if (!why.empty()) return fail(h, GS_E_INVALID, "%s", why.c_str());
  }
  return value_install(h, h->critic[0].net, p, o, true);
}

int gs_value_mlp_eval(gs_handle* h, double* values_host) {
  if (!h || !values_host) return fail(h, GS_E_INVALID, "handle / values_host is NULL");
  const gs_handle::Value& val = h->critic[0].net;
  if (!val.set) return fail(h, GS_E_STATE, "gs_value_mlp_eval before gs_value_mlp_set");
  if (!h->was_reset) return fail(h, GS_E_STATE, "gs_value_mlp_eval before gs_reset");
  GS_ENTER(h);
  int rc = launch_value_rows(h, val, h->d_obs2[h->obs_cur], val.out, h->B);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(values_host, val.out, (size_t)h->B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

// ---- values, advantages and returns of the last rollout --------------------------------------------------------------------------
int gs_rollout_evaluate(gs_handle* h, const gs_gae_config* cfg) {
  if (!h || !cfg) return fail(h, GS_E_INVALID, "handle / config is NULL");
  if (cfg->struct_size != (int32_t)sizeof(gs_gae_config)) return fail(h, GS_E_INVALID, "gs_gae_config struct_size %d != %d", cfg->struct_size, (int)sizeof(gs_gae_config));
  int rc = gae_check(h, cfg->bootstrap_mask, cfg->gamma, cfg->lambda, cfg->reward_shift, cfg->reward_scale, "reward");
  if (rc) return rc;
  gs_handle::Rollout& ro = h->ro;
  gs_handle::Critic& c = h->critic[0];
  if (ro.T <= 0) return fail(h, GS_E_STATE, "gs_rollout_evaluate: no rollout has been collected on this handle");
  if (!c.net.set) return fail(h, GS_E_STATE, "gs_rollout_evaluate before gs_value_mlp_set");
  GS_ENTER(h);
  c.evaluated_on = 0;        // (until every launch is queued)
  if ((rc = critic_evaluate(h, c, ro.rew, cfg->bootstrap_mask, cfg->gamma, cfg->lambda, cfg->reward_shift, cfg->reward_scale))) return rc;
  c.evaluated_on = ro.calls;
  return GS_OK;
}

int gs_rollout_onpolicy_view(gs_handle* h, gs_rollout_onpolicy* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Rollout& ro = h->ro;
  const gs_handle::Critic& c = h->critic[0];
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  if (!critic_current(h, c)) return fail(h, GS_E_STATE, "gs_rollout_evaluate has not run on the last rollout");
  int rc = rollout_finish(h);      // (waits for the rollout, not for the evaluation)
  if (rc) return rc;
  if ((rc = publish(h, h->stream, ro.ev_eval, consumer_stream))) return rc;
  out->T = ro.T; out->B = h->B; out->n_terminal = ro.n_term; out->rows_per_tile = GS_VAL_ROWS;
  out->log_probs = ro.logp_recorded ? ro.logp.p : nullptr;
  out->values = c.values; out->terminal_values = c.term_values; out->advantages = c.adv; out->returns = c.ret;
  return GS_OK;
}

int gs_rollout_onpolicy_download(gs_handle* h, const gs_rollout_onpolicy_host* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Rollout& ro = h->ro;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  if ((out->values || out->terminal_values || out->advantages || out->returns) && !critic_current(h, h->critic[0]))
    return fail(h, GS_E_STATE, "gs_rollout_evaluate has not run on the last rollout");
  if (out->log_probs && !ro.logp_recorded) return fail(h, GS_E_STATE, "the last rollout recorded no log-probabilities (a stochastic GS_POLICY_MLP rollout does)");
  int rc = rollout_finish(h);
  if (rc) return rc;
  if (out->log_probs) HIPCHK(h, hipMemcpyAsync(out->log_probs, ro.logp, (size_t)ro.T * h->B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if ((rc = critic_download(h, h->critic[0], out->values, out->terminal_values, out->advantages, out->returns))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

}  // extern "C"
