// abi_q.hip -- state-action critics (include/gridstep.h "state-action critics"): the twin Q networks and their
// target images (gs_q_mlp_*, gs_q_target_*), and what gs_rollout_evaluate_q makes of the last rollout (the twins' values under both
// images, their minimum, IQL's advantage and the one-step TD target) with its view and download.  The Q networks' images and the
// arrays over the rollout are made here and released here; the Q learner and the signals are abi_learner.hip's.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "handle.h"

using namespace gsi;

static_assert(sizeof(gs_q_eval_config) == 32, "gs_q_eval_config: two int32, three doubles");

// the options with shift / scale extended over the action columns (shift 0, scale 1): what gs_policy_pack_f32 and the rules of
// gs_policy_mlp_opts take for an input of obs_dim + action_dim columns
namespace {
struct QOpts {
  gs_policy_mlp_opts o{}; std::vector<double> shift, scale;
  QOpts(const gs_policy_mlp_opts& in, int D, int A) : shift((size_t)D + A, 0.0), scale((size_t)D + A, 1.0) {
    o = in;
    for (int i = 0; i < D; ++i) { if (in.obs_shift) shift[i] = in.obs_shift[i]; if (in.obs_scale) scale[i] = in.obs_scale[i]; }
    o.obs_shift = shift.data(); o.obs_scale = scale.data();
  }
};
}  // namespace

std::string gs_q_check(const gs_policy_mlp* p, const gs_policy_mlp_opts* o, int32_t obs_dim, int32_t action_dim) {
  if (!p) return "Q network is NULL";
  if (action_dim <= 0) return "a Q network needs action_dim > 0 (have " + std::to_string(action_dim) + ")";
  if (obs_dim <= 0) return "a Q network needs obs_dim > 0 (have " + std::to_string(obs_dim) + ")";
  const bool sized = p->struct_size == (int32_t)sizeof(gs_policy_mlp) && o && o->struct_size == (int32_t)sizeof(gs_policy_mlp_opts);
  if (!sized) return gs_value_check(p, o, obs_dim + action_dim);      // (refused before shift / scale are read)
  if (p->dims[0] != obs_dim + action_dim)
    return "dims[0] = " + std::to_string(p->dims[0]) + " != obs_dim + action_dim = " + std::to_string(obs_dim + action_dim);
  const QOpts q(*o, obs_dim, action_dim);
  return gs_value_check(p, &q.o, obs_dim + action_dim);
}

namespace gsi __attribute__((visibility("hidden"))) {

void q_rollout_release(gs_handle* h) {
  gs_handle::QTrack& t = h->qt;
  t.q.release(); t.q_min.release(); t.q_adv.release(); t.td.release();
  t.evaluated_on = 0;
  if (t.ev) { (void)hipEventDestroy(t.ev); t.ev = nullptr; }
}

void q_release(gs_handle* h) {
  q_rollout_release(h);
  for (gs_handle::QNet& Q : h->qnet) { Q.net.blob.release(); Q.target.release(); Q.net.set = false; Q.image_floats = 0; }
}

}  // namespace gsi

extern "C" {

int gs_q_mlp_check(const gs_policy_mlp* p, const gs_policy_mlp_opts* o, int32_t obs_dim, int32_t action_dim) {
  const std::string why = gs_q_check(p, o, obs_dim, action_dim);
  return why.empty() ? GS_OK : fail(nullptr, GS_E_INVALID, "%s", why.c_str());
}

int gs_q_mlp_set(gs_handle* h, int32_t which, const gs_policy_mlp* p, const gs_policy_mlp_opts* o) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (which < 0 || which > 1) return fail(h, GS_E_INVALID, "gs_q_mlp_set: which = %d outside 0 .. 1", which);
  if (p) {         // (a refused network leaves the installed one in place)
    const std::string why = gs_q_check(p, o, h->obs_dim, h->action_dim);
    if (!why.empty()) return fail(h, GS_E_INVALID, "%s", why.c_str());
  }
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  gs_handle::QNet& Q = h->qnet[which];
  gs_handle::Value& val = Q.net;
  learner_drop(h, GS_LEARNER_Q + which);     // (a learner trains the network it was created on)
  val.blob.release(); Q.target.release();
  val.set = false; Q.image_floats = 0;
  h->qt.evaluated_on = 0;                    // (what the last evaluation left belongs to the networks that were installed then)
  h->qn.evaluated_on = 0;
  if (!p) return GS_OK;
  const int D = h->obs_dim, A = h->action_dim;
  const QOpts q(*o, D, A);                   // (packed, shift and scale are 0 beyond D + A: a padded column normalises to 0)
  ScalarNet net;
  int rc = scalar_net_install(h, val, (const void*)gs_k_q_mlp_f32, *p, q.o, net);
  if (rc) return rc;
  const GsPolicyImageF32& im = net.im;
  if ((rc = Q.target.alloc(h, im.blob.size(), "the Q network's target image"))) { val.blob.release(); return rc; }
  HIPCHK(h, hipMemcpy(Q.target, im.blob.data(), im.blob.size() * sizeof(float), hipMemcpyHostToDevice));
  Q.image_floats = im.blob.size();
  val.args = GsValueArgs{};
  val.args.n_layers = p->n_layers; val.args.activation = p->activation;
  GsQArgs& a = Q.qargs;
  a = GsQArgs{};
  scalar_net_args(a, *p, net);
  a.D = D; a.A = A;
  for (int l = 0; l < p->n_layers; ++l) {
    val.args.L[l] = a.L[l];
    Q.TL[l] = GsPolicyLayerF32{Q.target.p + im.w_off[l], Q.target.p + im.b_off[l], im.kb[l], im.nt[l]};
  }
  val.set = true;
  return GS_OK;
}

int gs_rollout_evaluate_q(gs_handle* h, const gs_q_eval_config* cfg) {
  if (!h || !cfg) return fail(h, GS_E_INVALID, "handle / config is NULL");
  if (cfg->struct_size != (int32_t)sizeof(gs_q_eval_config))
    return fail(h, GS_E_INVALID, "gs_q_eval_config struct_size %d != %d", cfg->struct_size, (int)sizeof(gs_q_eval_config));
  int rc = gae_check(h, cfg->bootstrap_mask, cfg->gamma, 0.0, cfg->reward_shift, cfg->reward_scale, "reward");
  if (rc) return rc;
  gs_handle::Rollout& ro = h->ro;
  gs_handle::QTrack& t = h->qt;
  const gs_handle::Critic& c = h->critic[0];
  if (ro.T <= 0) return fail(h, GS_E_STATE, "gs_rollout_evaluate_q: no rollout has been collected on this handle");
  if (!h->qnet[0].net.set && !h->qnet[1].net.set) return fail(h, GS_E_STATE, "gs_rollout_evaluate_q before gs_q_mlp_set");
  if (!critic_current(h, c)) return fail(h, GS_E_STATE, "gs_rollout_evaluate_q: gs_rollout_evaluate has not run on the last rollout (values and terminal values are its)");
  GS_ENTER(h);
  const size_t B = h->B, cap = (size_t)ro.T_cap * B, TB = (size_t)ro.T * B;
  t.evaluated_on = 0;        // (until every launch is queued)
  if (!t.q && (rc = alloc_all(h, "the Q networks' arrays over the rollout", t.q.want(4 * cap), t.q_min.want(2 * cap), t.q_adv.want(cap), t.td.want(cap))))
    return rc;
  GsQCombineArgs C{};
  for (int w = 0; w < 2; ++w) {
    const gs_handle::QNet& Q = h->qnet[w];
    if (!Q.net.set) continue;
    for (int s = 0; s < 2; ++s) {
      double* out = t.q + (size_t)(2 * s + w) * cap;
      if ((rc = launch_q_rows(h, Q, s ? Q.TL : Q.qargs.L, ro.obs_seq, ro.act, (long long)TB, nullptr, out))) return rc;
      C.q[s][w] = out;
    }
  }
  C.values = c.values; C.q_min[0] = t.q_min; C.q_min[1] = t.q_min + cap; C.q_adv = t.q_adv; C.n = (long long)TB;
  hipLaunchKernelGGL(gs_k_q_combine, dim3((unsigned)((TB + 255) / 256)), dim3(256), 0, h->stream, C);
  HIPCHK(h, hipGetLastError());
  GsQTdArgs G{c.values, ro.rew, ro.done, c.term_values, ro.term_count, ro.term_idx, t.td, (int32_t)ro.T, h->B, cfg->bootstrap_mask, ro.term_cap, 0, 0,
              cfg->gamma, cfg->reward_shift, cfg->reward_scale};
  hipLaunchKernelGGL(gs_k_q_td, dim3((unsigned)((TB + 255) / 256)), dim3(256), 0, h->stream, G);
  HIPCHK(h, hipGetLastError());
  if (cfg->bootstrap_mask && ro.term_cap > 0) {
    G.phase = 1;
    hipLaunchKernelGGL(gs_k_q_td, dim3((unsigned)(((size_t)ro.term_cap + 255) / 256)), dim3(256), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
  }
  t.evaluated_on = ro.calls;
  return GS_OK;
}

int gs_rollout_q_view(gs_handle* h, gs_rollout_q* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Rollout& ro = h->ro;
  gs_handle::QTrack& t = h->qt;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  if (!q_current(h)) return fail(h, GS_E_STATE, "gs_rollout_evaluate_q has not run on the last rollout");
  GS_ENTER(h);
  int rc = publish(h, h->stream, t.ev, consumer_stream);
  if (rc) return rc;
  const size_t cap = (size_t)ro.T_cap * h->B;
  *out = gs_rollout_q{};
  out->T = ro.T; out->B = h->B; out->rows_per_tile = GS_VAL_ROWS;
  for (int w = 0; w < 2; ++w) {
    if (!h->qnet[w].net.set) continue;
    out->installed |= 1 << w;
    for (int s = 0; s < 2; ++s) out->q[s][w] = t.q + (size_t)(2 * s + w) * cap;
  }
  out->q_min[0] = t.q_min; out->q_min[1] = t.q_min + cap; out->q_adv = t.q_adv; out->td_target = t.td;
  return GS_OK;
}

int gs_rollout_q_download(gs_handle* h, const gs_rollout_q_host* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Rollout& ro = h->ro;
  gs_handle::QTrack& t = h->qt;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  if (!q_current(h)) return fail(h, GS_E_STATE, "gs_rollout_evaluate_q has not run on the last rollout");
  GS_ENTER(h);
  const size_t cap = (size_t)ro.T_cap * h->B, bytes = (size_t)ro.T * h->B * sizeof(double);
  for (int s = 0; s < 2; ++s) {
    for (int w = 0; w < 2; ++w)
      if (out->q[s][w] && h->qnet[w].net.set) HIPCHK(h, hipMemcpyAsync(out->q[s][w], t.q + (size_t)(2 * s + w) * cap, bytes, hipMemcpyDeviceToHost, h->stream));
    if (out->q_min[s]) HIPCHK(h, hipMemcpyAsync(out->q_min[s], t.q_min + (size_t)s * cap, bytes, hipMemcpyDeviceToHost, h->stream));
  }
  if (out->q_adv) HIPCHK(h, hipMemcpyAsync(out->q_adv, t.q_adv, bytes, hipMemcpyDeviceToHost, h->stream));
  if (out->td_target) HIPCHK(h, hipMemcpyAsync(out->td_target, t.td, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

int gs_q_target_update(gs_handle* h, double tau) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (!std::isfinite(tau) || tau < 0.0 || tau > 1.0) return fail(h, GS_E_INVALID, "gs_q_target_update: tau = %g outside [0, 1]", tau);
  if (!h->qnet[0].net.set && !h->qnet[1].net.set) return fail(h, GS_E_STATE, "gs_q_target_update before gs_q_mlp_set");
  GS_ENTER(h);
  for (gs_handle::QNet& Q : h->qnet) {
    if (!Q.net.set) continue;
    GsQPolyakArgs a{(const float*)Q.net.blob.p, Q.target.p, (long long)Q.image_floats, (float)tau, (float)(1.0 - tau)};
    hipLaunchKernelGGL(gs_k_q_polyak, dim3((unsigned)((Q.image_floats + 255) / 256)), dim3(256), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
  }
  return GS_OK;
}

int gs_q_target_download(gs_handle* h, int32_t which, float* params) {
  if (!h || !params) return fail(h, GS_E_INVALID, "handle / params is NULL");
  if (which < 0 || which > 1) return fail(h, GS_E_INVALID, "gs_q_target_download: which = %d outside 0 .. 1", which);
  const gs_handle::QNet& Q = h->qnet[which];
  if (!Q.net.set) return fail(h, GS_E_STATE, "gs_q_target_download: Q network %d is not installed", which);
  GS_ENTER(h);
  std::vector<float> img(Q.image_floats);
  HIPCHK(h, hipMemcpyAsync(img.data(), Q.target, Q.image_floats * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // the packed image into torch order
  float* dst = params;
  for (int l = 0; l < Q.qargs.n_layers; ++l) {
    const int n_out = Q.net.dims[l + 1], n_in = Q.net.dims[l];
    const GsPolicyLayerF32 host{img.data() + (Q.TL[l].w - Q.target.p), img.data() + (Q.TL[l].b - Q.target.p), Q.TL[l].kb, Q.TL[l].nt};
    gs_policy_unpack_f32(host, n_out, n_in, dst, nullptr);
    dst += (size_t)n_out * (n_in + 1);
  }
  return GS_OK;
}

}  // extern "C"
