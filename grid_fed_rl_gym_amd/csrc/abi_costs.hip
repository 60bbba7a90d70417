// abi_costs.hip -- constraint costs of a rollout (include/gridstep.h): gs_cost_config_*, gs_rollout_costs and
// gs_costs_eval (gs_k_costs, kernels_costs.hip), the cost critics (gs_cost_value_mlp_set, gs_rollout_evaluate_costs: critics
// 1 .. 3 of abi_onpolicy.hip's critic track, which owns their networks and arrays) and the views of what they left.  The rollout's
// constraint arrays are made here and released here (costs_release).
#include <cmath>
#include <string>

#include "handle.h"

using namespace gsi;

namespace gsi __attribute__((visibility("hidden"))) {

void costs_release(gs_handle* h) {
  gs_handle::Costs& cs = h->cc;
  cs.margins.release(); cs.counts.release(); cs.costs.release(); cs.n_viol.release();
  if (cs.ev) { (void)hipEventDestroy(cs.ev); cs.ev = nullptr; }
  cs.computed_on = 0;
}

}  // namespace gsi

// empty, or why `c` breaks the rules of gs_cost_config (include/gridstep.h)
static std::string cost_config_why(const gs_cost_config* c) {
  if (!c) return "gs_cost_config is NULL";
  if (c->struct_size != (int32_t)sizeof(gs_cost_config))
    return "gs_cost_config struct_size " + std::to_string(c->struct_size) + " != " + std::to_string(sizeof(gs_cost_config));
  for (int k = 0; k < GS_COST_CHANNELS; ++k)
    if (c->kind[k] < GS_COSTKIND_EXCESS || c->kind[k] > GS_COSTKIND_COUNT)
      return "kind[" + std::to_string(k) + "] = " + std::to_string(c->kind[k]) + " outside 0 .. 2";
  if (!std::isfinite(c->voltage_limits[0]) || !std::isfinite(c->voltage_limits[1]) || !std::isfinite(c->frequency_limits[0]) ||
      !std::isfinite(c->frequency_limits[1]) || !std::isfinite(c->line_loading_limit))
    return "voltage_limits / frequency_limits / line_loading_limit must be finite";
  if (c->voltage_limits[0] > c->voltage_limits[1]) return "voltage_limits: lo > hi";
  if (c->frequency_limits[0] > c->frequency_limits[1]) return "frequency_limits: lo > hi";
  return "";
}

static void cost_config_default(const gs_handle* h, gs_cost_config* out) {
  *out = gs_cost_config{};
  out->struct_size = (int32_t)sizeof(gs_cost_config);
  for (int k = 0; k < GS_COST_CHANNELS; ++k) out->kind[k] = GS_COSTKIND_EXCESS;
  out->voltage_limits[0] = h->cfg.v_min; out->voltage_limits[1] = h->cfg.v_max;
  out->frequency_limits[0] = h->cfg.f_min; out->frequency_limits[1] = h->cfg.f_max;
  out->line_loading_limit = 0.8;          // grid_env.py get_reward's threshold, safe.py thermal_constraint's default
}

// the argument block of gs_k_costs for this handle's observation layout and `c`, everything but the rows and the outputs
static GsCostArgs cost_args(const gs_handle* h, const gs_cost_config& c) {
  GsCostArgs a{};
  a.D = h->obs_dim; a.n = h->n; a.m = h->m;
  const int cols = 2 * h->n + 2 * h->m;
  a.lanes = gs_cost_lanes(cols);
  for (int k = 0; k < GS_COST_CHANNELS; ++k) a.kind[k] = c.kind[k];
  a.vlo = c.voltage_limits[0]; a.vhi = c.voltage_limits[1]; a.flo = c.frequency_limits[0]; a.fhi = c.frequency_limits[1];
  a.lim = c.line_loading_limit;
  return a;
}

static int launch_costs(gs_handle* h, GsCostArgs a, long long rows) {
  if (rows <= 0) return GS_OK;
  if (rows > 0x7fffffffLL) return fail(h, GS_E_INVALID, "%lld rows exceed the cost kernel's 32-bit row count", rows);
  a.rows = (int32_t)rows;
  const long long per_wave = GS_COST_ROWS * (64 / a.lanes);
  // one wavefront per workgroup, at most 32 per compute unit's worth of them; the kernel strides over the rest
  const long long groups = std::min<long long>((rows + per_wave - 1) / per_wave, 256 * 32);
  hipLaunchKernelGGL(gs_k_costs, dim3((unsigned)groups), dim3(64), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

static int cost_layout_check(gs_handle* h) {
  if (h->n <= 0 || 2 * h->n + 2 * h->m + 1 > h->obs_dim)
    return fail(h, GS_E_INVALID, "the observation (%d columns) does not start with 2 n + 2 m + 1 = %d grid columns", h->obs_dim, 2 * h->n + 2 * h->m + 1);
  return GS_OK;
}

extern "C" {

int gs_cost_config_default(const gs_handle* h, gs_cost_config* out) {
  if (!h || !out) return fail(nullptr, GS_E_INVALID, "handle / out is NULL");
  cost_config_default(h, out);
  return GS_OK;
}

int gs_cost_config_check(const gs_cost_config* c) {
  const std::string why = cost_config_why(c);
  return why.empty() ? GS_OK : fail(nullptr, GS_E_INVALID, "%s", why.c_str());
}

int gs_rollout_costs(gs_handle* h, const gs_cost_config* c) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  gs_cost_config def;
  if (!c) { cost_config_default(h, &def); c = &def; }
  const std::string why = cost_config_why(c);
  if (!why.empty()) return fail(h, GS_E_INVALID, "%s", why.c_str());
  gs_handle::Rollout& ro = h->ro;
  if (ro.T <= 0 || ro.calls == 0) return fail(h, GS_E_STATE, "gs_rollout_costs: no rollout has been collected on this handle");
  int rc = cost_layout_check(h);
  if (rc) return rc;
  GS_ENTER(h);
  gs_handle::Costs& cs = h->cc;
  const size_t B = h->B, T = ro.T, TB = T * B;
  if (!cs.margins) {         // sized by the rollout's capacity; released with it (costs_release); all four or none
    const size_t cap = (size_t)GS_COST_CHANNELS * ro.T_cap * B;
    if ((rc = alloc_all(h, "the rollout's constraint arrays", cs.margins.want(cap), cs.counts.want(cap), cs.costs.want(cap), cs.n_viol.want(GS_COST_CHANNELS)))) return rc;
  }
  cs.computed_on = 0;        // (until both launches are queued)
  HIPCHK(h, hipMemsetAsync(cs.n_viol, 0, GS_COST_CHANNELS * sizeof(unsigned long long), h->stream));
  GsCostArgs a = cost_args(h, *c);
  a.margins = cs.margins; a.counts = cs.counts; a.costs = cs.costs; a.n_violating = cs.n_viol;
  a.chan_stride = (long long)TB; a.row_stride = 1;
  // the ordinary transitions: row t * B + b of obs_seq[1 ..] is the observation r_t was computed on unless the transition ended an
  // episode (its done flag: that slot holds the fresh observation after the in-place reset)
  GsCostArgs o = a;
  o.obs = ro.obs_seq + B * (size_t)h->obs_dim; o.skip = ro.done;
  if ((rc = launch_costs(h, o, (long long)TB))) return rc;
  // the terminal rows: launched over the list's capacity, the count read on the device, every result filed at its (t, b) -- the
  // entries the first launch left out, so the two need no order between them
  GsCostArgs t = a;
  t.obs = ro.term_obs; t.rows_dev = ro.term_count; t.scatter_idx = ro.term_idx; t.scatter_T = (int32_t)T; t.scatter_B = h->B;
  if ((rc = launch_costs(h, t, ro.term_cap))) return rc;
  cs.computed_on = ro.calls;
  return GS_OK;
}

int gs_costs_eval(gs_handle* h, const gs_cost_config* c, const double* obs_host, int32_t rows, double* margins_host, int32_t* counts_host,
                  double* costs_host) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (!obs_host || rows <= 0) return fail(h, GS_E_INVALID, "gs_costs_eval: obs_host is NULL or rows <= 0");
  gs_cost_config def;
  if (!c) { cost_config_default(h, &def); c = &def; }
  const std::string why = cost_config_why(c);
  if (!why.empty()) return fail(h, GS_E_INVALID, "%s", why.c_str());
  int rc = cost_layout_check(h);
  if (rc) return rc;
  GS_ENTER(h);
  const size_t R = (size_t)rows, obs_bytes = R * h->obs_dim * sizeof(double), out8 = R * GS_COST_CHANNELS * sizeof(double);
  // one allocation for the call: the rows, then margins, costs and counts [rows][3]
  DevBuf<char> buf;
  if ((rc = buf.alloc(h, obs_bytes + 2 * out8 + out8 / 2, "gs_costs_eval's rows"))) return rc;
  GsCostArgs a = cost_args(h, *c);
  a.obs = (const double*)buf.p;
  a.margins = (double*)(buf + obs_bytes); a.costs = (double*)(buf + obs_bytes + out8); a.counts = (int32_t*)(buf + obs_bytes + 2 * out8);
  a.chan_stride = 1; a.row_stride = GS_COST_CHANNELS;
  hipError_t e = hipMemcpyAsync(buf, obs_host, obs_bytes, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) rc = launch_costs(h, a, rows);
  if (e == hipSuccess && !rc && margins_host) e = hipMemcpyAsync(margins_host, a.margins, out8, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && !rc && costs_host) e = hipMemcpyAsync(costs_host, a.costs, out8, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && !rc && counts_host) e = hipMemcpyAsync(counts_host, a.counts, out8 / 2, hipMemcpyDeviceToHost, h->stream);
  const hipError_t es = hipStreamSynchronize(h->stream);      // (before `buf` goes)
  if (rc) return rc;
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(h, GS_E_HIP, "gs_costs_eval failed: %s", hipGetErrorString(e));
  return GS_OK;
}

// ---- the cost critics ---------------------------------------------------------------------------------------------------------------
int gs_cost_value_mlp_set(gs_handle* h, int32_t channel, const gs_policy_mlp* p, const gs_policy_mlp_opts* o) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (channel < 0 || channel >= GS_COST_CHANNELS) return fail(h, GS_E_INVALID, "cost channel %d outside 0 .. 2", channel);
  if (p) {         // (a refused network leaves the installed one in place)
    const std::string why = gs_value_check(p, o, h->obs_dim);
    if (!why.empty()) return fail(h, GS_E_INVALID, "%s", why.c_str());
  }
  return value_install(h, h->critic[1 + channel].net, p, o, false);
}

int gs_rollout_evaluate_costs(gs_handle* h, const gs_cost_gae_config* cfg) {
  if (!h || !cfg) return fail(h, GS_E_INVALID, "handle / config is NULL");
  if (cfg->struct_size != (int32_t)sizeof(gs_cost_gae_config))
    return fail(h, GS_E_INVALID, "gs_cost_gae_config struct_size %d != %d", cfg->struct_size, (int)sizeof(gs_cost_gae_config));
  int rc = GS_OK;
  for (int c = 0; c < GS_COST_CHANNELS; ++c)
    if ((rc = gae_check(h, cfg->bootstrap_mask, cfg->gamma[c], cfg->lambda[c], cfg->cost_shift[c], cfg->cost_scale[c], "cost"))) return rc;
  gs_handle::Rollout& ro = h->ro;
  gs_handle::Costs& cs = h->cc;
  gs_handle::Critic* const critic = h->critic + 1;      // [channel]
  if (ro.T <= 0 || ro.calls == 0) return fail(h, GS_E_STATE, "gs_rollout_evaluate_costs: no rollout has been collected on this handle");
  if (!cs.computed_on || cs.computed_on != ro.calls) return fail(h, GS_E_STATE, "gs_rollout_evaluate_costs: gs_rollout_costs has not run on the last rollout");
  bool any = false;
  for (int c = 0; c < GS_COST_CHANNELS; ++c) any = any || critic[c].net.set;
  if (!any) return fail(h, GS_E_STATE, "gs_rollout_evaluate_costs before gs_cost_value_mlp_set");
  GS_ENTER(h);
  // no channel counts as evaluated until every launch of this call is queued -- one whose critic has been removed never again
  for (int c = 0; c < GS_COST_CHANNELS; ++c) critic[c].evaluated_on = 0;
  const size_t TB = (size_t)ro.T * h->B;
  for (int c = 0; c < GS_COST_CHANNELS; ++c)
    if (critic[c].net.set && (rc = critic_evaluate(h, critic[c], cs.costs + c * TB, cfg->bootstrap_mask, cfg->gamma[c], cfg->lambda[c],
                                                   cfg->cost_shift[c], cfg->cost_scale[c]))) return rc;
  for (int c = 0; c < GS_COST_CHANNELS; ++c) if (critic[c].net.set) critic[c].evaluated_on = ro.calls;
  return GS_OK;
}

// ---- what the two calls left --------------------------------------------------------------------------------------------------------
int gs_rollout_costs_view(gs_handle* h, gs_rollout_costs_dev* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Rollout& ro = h->ro;
  gs_handle::Costs& cs = h->cc;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  if (!cs.computed_on || cs.computed_on != ro.calls) return fail(h, GS_E_STATE, "gs_rollout_costs has not run on the last rollout");
  int rc = rollout_finish(h);      // (waits for the rollout, not for the costs)
  if (rc) return rc;
  if ((rc = publish(h, h->stream, cs.ev, consumer_stream))) return rc;
  *out = gs_rollout_costs_dev{};
  out->T = ro.T; out->B = h->B;
  out->margins = cs.margins; out->counts = cs.counts; out->costs = cs.costs; out->n_violating = (const int64_t*)cs.n_viol.p;
  for (int c = 0; c < GS_COST_CHANNELS; ++c) {
    const gs_handle::Critic& k = h->critic[1 + c];
    if (!critic_current(h, k)) continue;
    out->values[c] = k.values; out->terminal_values[c] = k.term_values; out->advantages[c] = k.adv; out->returns[c] = k.ret;
  }
  return GS_OK;
}

int gs_rollout_costs_download(gs_handle* h, const gs_rollout_costs_host* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Rollout& ro = h->ro;
  gs_handle::Costs& cs = h->cc;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  if (!cs.computed_on || cs.computed_on != ro.calls) return fail(h, GS_E_STATE, "gs_rollout_costs has not run on the last rollout");
  for (int c = 0; c < GS_COST_CHANNELS; ++c)
    if ((out->values[c] || out->terminal_values[c] || out->advantages[c] || out->returns[c]) && !critic_current(h, h->critic[1 + c]))
      return fail(h, GS_E_STATE, "gs_rollout_evaluate_costs has not run on the last rollout with a critic for channel %d", c);
  int rc = rollout_finish(h);
  if (rc) return rc;
  const size_t TB = (size_t)ro.T * h->B, TB8 = TB * sizeof(double);
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  if (out->margins) HIPCHK(h, hipMemcpyAsync(out->margins, cs.margins, GS_COST_CHANNELS * TB8, d2h, h->stream));
  if (out->counts) HIPCHK(h, hipMemcpyAsync(out->counts, cs.counts, GS_COST_CHANNELS * TB * sizeof(int32_t), d2h, h->stream));
  if (out->costs) HIPCHK(h, hipMemcpyAsync(out->costs, cs.costs, GS_COST_CHANNELS * TB8, d2h, h->stream));
  if (out->n_violating) HIPCHK(h, hipMemcpyAsync(out->n_violating, cs.n_viol, GS_COST_CHANNELS * sizeof(int64_t), d2h, h->stream));
  for (int c = 0; c < GS_COST_CHANNELS; ++c)
    if ((rc = critic_download(h, h->critic[1 + c], out->values[c], out->terminal_values[c], out->advantages[c], out->returns[c]))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

}  // extern "C"
