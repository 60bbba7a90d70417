// abi_onpolicy.hip -- on-policy rollouts (include/gridstep.h): the value network (gs_value_mlp_*), gs_rollout_evaluate and the
// views of what it and the policy kernels' log-probability output left.  The value network's buffers and the rollout's on-policy
// arrays are made here and released here (the log-probabilities are allocated by gs_rollout, abi_rollout.hip, which writes them).
// The cost critics of abi_costs.hip are value networks too: installed and launched through value_install / launch_value, released here.
#include <cmath>
#include <string>

#include "handle.h"

using namespace gsi;

namespace gsi __attribute__((visibility("hidden"))) {

void value_release(gs_handle* h) {
  dev_free(h->val.blob);
  dev_free(h->val.out);
  h->val.set = false;
  for (gs_handle::Value& v : h->cost_val) { dev_free(v.blob); dev_free(v.out); v.set = false; }
}

void onpolicy_release(gs_handle* h) {
  gs_handle::Rollout& ro = h->ro;
  dev_free(ro.logp); dev_free(ro.values); dev_free(ro.term_values); dev_free(ro.adv); dev_free(ro.ret);
  if (ro.ev_eval) { (void)hipEventDestroy(ro.ev_eval); ro.ev_eval = nullptr; }
  ro.logp_recorded = false; ro.evaluated_on = 0;
}

// what gs_value_mlp_set and gs_cost_value_mlp_set (abi_costs.hip) share: `p` has passed gs_value_check; NULL removes the network
int value_install(gs_handle* h, gs_handle::Value& val, const gs_policy_mlp* p, const gs_policy_mlp_opts* o, bool want_out) {
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  dev_free(val.blob);
  val.set = false;
  if (!p) return GS_OK;
  if (want_out && !val.out) HIPCHK(h, hipMalloc((void**)&val.out, (size_t)h->B * sizeof(double)));
  const GsPolicyImageF32 im = gs_policy_pack_f32(*p, *o);
  val.lds = gs_val_lds_bytes(im.kb[0]);
  HIPCHK(h, hipFuncSetAttribute((const void*)gs_k_value_mlp_f32, hipFuncAttributeMaxDynamicSharedMemorySize, GS_VAL_LDS_MAX));
  // one allocation: the float image (a multiple of 16 floats), then shift and scale
  const size_t image_bytes = im.blob.size() * sizeof(float), norm_bytes = im.norm.size() * sizeof(double);
  HIPCHK(h, hipMalloc((void**)&val.blob, image_bytes + norm_bytes));
  const float* image = val.blob;
  const double* norm = (const double*)((const char*)val.blob + image_bytes);
  HIPCHK(h, hipMemcpy((void*)image, im.blob.data(), image_bytes, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy((void*)norm, im.norm.data(), norm_bytes, hipMemcpyHostToDevice));
  GsValueArgs& a = val.args;
  a = GsValueArgs{};
  a.shift = norm; a.scale = norm + 16 * im.kb[0];
  a.D = h->obs_dim; a.n_layers = p->n_layers; a.activation = p->activation;
  a.panel_kb = gs_val_panel_kb(im.kb[0]); a.obs_stride = gs_val_obs_stride(im.kb[0]);
  for (int l = 0; l < p->n_layers; ++l) a.L[l] = GsPolicyLayerF32{image + im.w_off[l], image + im.b_off[l], im.kb[l], im.nt[l]};
  val.set = true;
  return GS_OK;
}

// one launch over `rows` rows of obs (device pointers) on the handle's main stream; rows_dev / scatter_*: GsValueArgs
int launch_value(gs_handle* h, const gs_handle::Value& val, const double* obs, double* out, long long rows, const int32_t* rows_dev,
                 const int32_t* scatter_idx, double* scatter_out, int scatter_T) {
  if (rows <= 0) return GS_OK;
  if (rows > 0x7fffffffLL - GS_VAL_ROWS) return fail(h, GS_E_INVALID, "%lld rows exceed the value kernel's 32-bit row index", rows);
  GsValueArgs a = val.args;
  a.obs = obs; a.out = out; a.rows = (int32_t)rows; a.rows_dev = rows_dev;
  a.scatter_idx = scatter_idx; a.scatter_out = scatter_out; a.scatter_T = scatter_T; a.scatter_B = h->B;
  hipLaunchKernelGGL(gs_k_value_mlp_f32, dim3((unsigned)((rows + GS_VAL_ROWS - 1) / GS_VAL_ROWS)), dim3(64 * GS_POL_WAVES), val.lds, h->stream, a);
  HIPCHK(h, hipGetLastError());
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
  return value_install(h, h->val, p, o, true);
}

int gs_value_mlp_eval(gs_handle* h, double* values_host) {
  if (!h || !values_host) return fail(h, GS_E_INVALID, "handle / values_host is NULL");
  if (!h->val.set) return fail(h, GS_E_STATE, "gs_value_mlp_eval before gs_value_mlp_set");
  if (!h->was_reset) return fail(h, GS_E_STATE, "gs_value_mlp_eval before gs_reset");
  GS_ENTER(h);
  int rc = launch_value(h, h->val, h->d_obs2[h->obs_cur], h->val.out, h->B);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(values_host, h->val.out, (size_t)h->B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

// ---- values, advantages and returns of the last rollout --------------------------------------------------------------------------
int gs_rollout_evaluate(gs_handle* h, const gs_gae_config* cfg) {
  if (!h || !cfg) return fail(h, GS_E_INVALID, "handle / config is NULL");
  if (cfg->struct_size != (int32_t)sizeof(gs_gae_config)) return fail(h, GS_E_INVALID, "gs_gae_config struct_size %d != %d", cfg->struct_size, (int)sizeof(gs_gae_config));
  if (cfg->bootstrap_mask < 0 || cfg->bootstrap_mask > 3) return fail(h, GS_E_INVALID, "bootstrap_mask %d outside 0 .. 3", cfg->bootstrap_mask);
  if (!std::isfinite(cfg->gamma) || !std::isfinite(cfg->lambda) || !std::isfinite(cfg->reward_shift) || !std::isfinite(cfg->reward_scale))
    return fail(h, GS_E_INVALID, "gamma / lambda / reward_shift / reward_scale must be finite");
  gs_handle::Rollout& ro = h->ro;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "gs_rollout_evaluate: no rollout has been collected on this handle");
  if (!h->val.set) return fail(h, GS_E_STATE, "gs_rollout_evaluate before gs_value_mlp_set");
  GS_ENTER(h);
  const size_t B = h->B, T = ro.T;
  if (!ro.values) {          // sized by the rollout's capacity; released with it (onpolicy_release)
    if (hipMalloc((void**)&ro.values, (size_t)(ro.T_cap + 1) * B * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&ro.term_values, (size_t)std::max(ro.term_cap, 1) * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&ro.adv, (size_t)ro.T_cap * B * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&ro.ret, (size_t)ro.T_cap * B * sizeof(double)) != hipSuccess) {
      // all four or none: a later call must not find `values` and launch on the others
      dev_free(ro.values); dev_free(ro.term_values); dev_free(ro.adv); dev_free(ro.ret);
      return fail(h, GS_E_NOMEM, "on-policy arrays for T = %d do not fit", ro.T_cap);
    }
  }
  int rc = launch_value(h, h->val, ro.obs_seq, ro.values, (long long)((T + 1) * B));
  if (rc) return rc;
  // the terminal rows: launched over the list's capacity, the count read on the device; every value also goes to its (t, b) in
  // `ret`, where gs_k_gae looks for it before it writes the return there
  if ((rc = launch_value(h, h->val, ro.term_obs, ro.term_values, ro.term_cap, ro.term_count, ro.term_idx, ro.ret, (int)T))) return rc;
  GsGaeArgs g{ro.values, ro.rew, ro.done, ro.adv, ro.ret, (int32_t)T, h->B, cfg->bootstrap_mask, 0, cfg->gamma, cfg->lambda, cfg->reward_shift, cfg->reward_scale};
  hipLaunchKernelGGL(gs_k_gae, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, g);
  HIPCHK(h, hipGetLastError());
  ro.evaluated_on = ro.calls;
  return GS_OK;
}

int gs_rollout_onpolicy_view(gs_handle* h, gs_rollout_onpolicy* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Rollout& ro = h->ro;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  if (!ro.evaluated_on || ro.evaluated_on != ro.calls) return fail(h, GS_E_STATE, "gs_rollout_evaluate has not run on the last rollout");
  int rc = rollout_finish(h);      // (waits for the rollout, not for the evaluation)
  if (rc) return rc;
  if (consumer_stream) {
    if (!ro.ev_eval) HIPCHK(h, hipEventCreateWithFlags(&ro.ev_eval, hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(ro.ev_eval, h->stream));
    HIPCHK(h, hipStreamWaitEvent(peer_stream(consumer_stream), ro.ev_eval, 0));
  } else {
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  out->T = ro.T; out->B = h->B; out->n_terminal = ro.n_term; out->rows_per_tile = GS_VAL_ROWS;
  out->log_probs = ro.logp_recorded ? ro.logp : nullptr;
  out->values = ro.values; out->terminal_values = ro.term_values; out->advantages = ro.adv; out->returns = ro.ret;
  return GS_OK;
}

int gs_rollout_onpolicy_download(gs_handle* h, const gs_rollout_onpolicy_host* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Rollout& ro = h->ro;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  const bool evaluated = ro.evaluated_on && ro.evaluated_on == ro.calls;
  if ((out->values || out->terminal_values || out->advantages || out->returns) && !evaluated)
    return fail(h, GS_E_STATE, "gs_rollout_evaluate has not run on the last rollout");
  if (out->log_probs && !ro.logp_recorded) return fail(h, GS_E_STATE, "the last rollout recorded no log-probabilities (a stochastic GS_POLICY_MLP rollout does)");
  int rc = rollout_finish(h);
  if (rc) return rc;
  const size_t TB = (size_t)ro.T * h->B * sizeof(double), B8 = (size_t)h->B * sizeof(double);
  if (out->log_probs) HIPCHK(h, hipMemcpyAsync(out->log_probs, ro.logp, TB, hipMemcpyDeviceToHost, h->stream));
  if (out->values) HIPCHK(h, hipMemcpyAsync(out->values, ro.values, TB + B8, hipMemcpyDeviceToHost, h->stream));
  if (out->terminal_values && ro.n_term) HIPCHK(h, hipMemcpyAsync(out->terminal_values, ro.term_values, (size_t)ro.n_term * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->advantages) HIPCHK(h, hipMemcpyAsync(out->advantages, ro.adv, TB, hipMemcpyDeviceToHost, h->stream));
  if (out->returns) HIPCHK(h, hipMemcpyAsync(out->returns, ro.ret, TB, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

}  // extern "C"
