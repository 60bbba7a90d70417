// abi_anchor.hip -- parameter anchors (include/gridstep.h "parameter anchors"): the PROX centre and the EWC slot
// of a learner (gs_learner_anchor_*), the Fisher diagonal of a task (gs_learner_fisher_*: gs_learner_step's passes through
// learner_backprop of abi_learner.hip, then the squared weight-gradient product), and anchor_queue, the one launch the steps gain
// while a coefficient is non-zero.  The buffers are gs_handle::Learner::an's, made here on first use; learner_drop releases them.
#include <cmath>
#include <vector>

#include "handle.h"

using namespace gsi;

static_assert(sizeof(gs_learner_anchor_config) == 24, "gs_learner_anchor_config: two int32, two doubles");
static_assert(sizeof(gs_fisher_config) == 24, "gs_fisher_config: two int32, two doubles");
static_assert(sizeof(gs_learner_anchor_stats_out) == 56, "gs_learner_anchor_stats_out: five doubles, two int64");

namespace {

// the value rules of a gs_learner_anchor_config; empty: none broken
const char* anchor_config_why(const gs_learner_anchor_config* c) {
  if (!c) return "gs_learner_anchor_config is NULL";
  if (c->struct_size != (int32_t)sizeof(gs_learner_anchor_config)) return "gs_learner_anchor_config struct_size is not sizeof(gs_learner_anchor_config)";
  if (!std::isfinite(c->prox_mu) || c->prox_mu < 0.0 || !std::isfinite(c->ewc_lambda) || c->ewc_lambda < 0.0)
    return "gs_learner_anchor_config: prox_mu and ewc_lambda must be finite and >= 0";
  return nullptr;
}

// the live learner `net` of `h`, or the refusal under the entry's name
int learner_of(gs_handle* h, int32_t net, const char* who, gs_handle::Learner** out) {
  if (!h) return fail(nullptr, GS_E_INVALID, "%s: handle is NULL", who);
  if (net < 0 || net >= GS_LEARNER_COUNT) return fail(h, GS_E_INVALID, "%s: unknown net %d", who, net);
  gs_handle::Learner& Ln = h->learner[net];
  if (!Ln.live) return fail(h, GS_E_STATE, "%s: no learner for %s", who, net_name(net));
  *out = &Ln;
  return GS_OK;
}

// gs_learner_fisher_accumulate's own precondition, run by learner_backprop behind gs_learner_step's checks
int fisher_open(gs_handle* h, int32_t net) {
  if (!h->learner[net].an.open) return fail(h, GS_E_STATE, "gs_learner_fisher_accumulate: no task is open for %s (gs_learner_fisher_begin)", net_name(net));
  return GS_OK;
}

// the sum of v[0 .. count) in the order gs_k_train_stats adds the gradient norm's workgroup sums: thread t of 1024 over entries t,
// t + 1024, ... ascending from 0.0, then the balanced tree of block_reduce.h (partners at 32, ..., 1 lanes, then at 8, 4, 2, 1
// over the sixteen wavefronts)
double stat_tree_sum(const double* v, int count) {
  double t[GS_TR_STAT_THREADS];
  for (int k = 0; k < GS_TR_STAT_THREADS; ++k) t[k] = 0.0;
  for (int k = 0; k < count; ++k) t[k % GS_TR_STAT_THREADS] = t[k % GS_TR_STAT_THREADS] + v[k];
  double u[GS_TR_STAT_THREADS];
  for (int off = 32; off > 0; off >>= 1) {
    for (int k = 0; k < GS_TR_STAT_THREADS; ++k) u[k] = t[k] + t[k ^ off];
    for (int k = 0; k < GS_TR_STAT_THREADS; ++k) t[k] = u[k];
  }
  constexpr int W = GS_TR_STAT_THREADS / 64;
  double w[W], x[W];
  for (int k = 0; k < W; ++k) w[k] = t[64 * k];
  for (int off = W / 2; off > 0; off >>= 1) {
    for (int k = 0; k < W; ++k) x[k] = w[k] + w[k ^ off];
    for (int k = 0; k < W; ++k) w[k] = x[k];
  }
  return w[0];
}

}  // namespace

int gsi::anchor_queue(gs_handle* h, gs_handle::Learner& Ln) {
  gs_handle::Learner::Anchor& an = Ln.an;
  const int blocks = gs_tr_red_blocks(Ln.net.P);
  int rc = an.sums.grow(h, (size_t)3 * blocks, "the anchors' workgroup sums");      // (gs_learner_anchor_set made them: nothing to do)
  if (rc) return rc;
  GsAnchorArgs A{};
  A.grad = Ln.grad; A.params = Ln.params; A.prox = an.prox; A.importance = an.importance; A.centre = an.centre;
  A.blocksum = Ln.blocksum; A.sum_loss = an.sums; A.sum_prox = an.sums + blocks; A.sum_ewc = an.sums + 2 * (size_t)blocks;
  A.P = Ln.net.P; A.mu = (float)an.mu; A.lambda = (float)an.lambda;
  hipLaunchKernelGGL(gs_k_train_anchor, dim3(blocks), dim3(GS_TR_RED_THREADS), 0, h->stream, A);
  HIPCHK(h, hipGetLastError());
  an.stepped = true; an.step_mu = an.mu; an.step_lambda = an.lambda;
  return GS_OK;
}

extern "C" {

int gs_learner_anchor_check(const gs_learner_anchor_config* cfg) {
  const char* why = anchor_config_why(cfg);
  return why ? fail(nullptr, GS_E_INVALID, "%s", why) : GS_OK;
}

int gs_learner_anchor_here(gs_handle* h, int32_t net, const float* params_host) {
  gs_handle::Learner* Ln = nullptr;
  int rc = learner_of(h, net, "gs_learner_anchor_here", &Ln);
  if (rc) return rc;
  GS_ENTER(h);
  gs_handle::Learner::Anchor& an = Ln->an;
  const size_t P = (size_t)Ln->net.P;
  if ((rc = an.prox.grow(h, P, "the PROX centre"))) return rc;
  if (params_host) {
    HIPCHK(h, hipMemcpyAsync(an.prox, params_host, P * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (the caller's array is its own again)
  } else {
    HIPCHK(h, hipMemcpyAsync(an.prox, Ln->params, P * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  }
  an.have_prox = true;
  return GS_OK;
}

int gs_learner_anchor_set(gs_handle* h, int32_t net, const gs_learner_anchor_config* cfg) {
  gs_handle::Learner* Ln = nullptr;
  int rc = learner_of(h, net, "gs_learner_anchor_set", &Ln);
  if (rc) return rc;
  const char* why = anchor_config_why(cfg);
  if (why) return fail(h, GS_E_INVALID, "%s", why);
  gs_handle::Learner::Anchor& an = Ln->an;
  if (cfg->prox_mu > 0.0 && !an.have_prox)
    return fail(h, GS_E_STATE, "gs_learner_anchor_set: prox_mu > 0 but %s has no PROX centre (gs_learner_anchor_here)", net_name(net));
  if (cfg->ewc_lambda > 0.0 && !an.tasks)
    return fail(h, GS_E_STATE, "gs_learner_anchor_set: ewc_lambda > 0 but no task has been committed for %s (gs_learner_fisher_commit)", net_name(net));
  if (cfg->prox_mu > 0.0 || cfg->ewc_lambda > 0.0) {
    GS_ENTER(h);
    if ((rc = an.sums.grow(h, (size_t)3 * gs_tr_red_blocks(Ln->net.P), "the anchors' workgroup sums"))) return rc;
  }
  an.mu = cfg->prox_mu; an.lambda = cfg->ewc_lambda;      // (a queued step took its arguments by value: it keeps the ones it was queued with)
  return GS_OK;
}

int gs_learner_anchor_get(gs_handle* h, int32_t net, gs_learner_anchor_config* out) {
  gs_handle::Learner* Ln = nullptr;
  int rc = learner_of(h, net, "gs_learner_anchor_get", &Ln);
  if (rc) return rc;
  if (!out) return fail(h, GS_E_INVALID, "gs_learner_anchor_get: out is NULL");
  *out = gs_learner_anchor_config{(int32_t)sizeof(gs_learner_anchor_config), 0, Ln->an.mu, Ln->an.lambda};
  return GS_OK;
}

int gs_learner_fisher_begin(gs_handle* h, int32_t net) {
  gs_handle::Learner* Ln = nullptr;
  int rc = learner_of(h, net, "gs_learner_fisher_begin", &Ln);
  if (rc) return rc;
  GS_ENTER(h);
  gs_handle::Learner::Anchor& an = Ln->an;
  const size_t P = (size_t)Ln->net.P;
  if ((rc = an.pending.grow(h, P, "the pending Fisher sum"))) return rc;
  HIPCHK(h, hipMemsetAsync(an.pending, 0, P * sizeof(double), h->stream));
  an.samples = 0; an.open = true;
  return GS_OK;
}

int gs_learner_fisher_accumulate(gs_handle* h, int32_t net, const gs_onpolicy_batch_out* batch, int32_t n, void* consumer_stream) {
  if (!h || !batch) return fail(h, GS_E_INVALID, "handle / batch is NULL");
  LearnerPass ps{};
  int rc = learner_backprop(h, "gs_learner_fisher_accumulate", net, batch, n, fisher_open, ps);
  if (rc) return rc;
  gs_handle::Learner& Ln = h->learner[net];
  gs_handle::Learner::Anchor& an = Ln.an;
  const GsTrainNet& N = Ln.net;
  const int segments = gs_tr_segments(n);
  GsTrainGradArgs G{};
  const int blocks = train_grad_args(h, N, ps.rows, n, ps.Din, G);
  hipLaunchKernelGGL(gs_k_train_grad_sq, dim3(blocks, segments), dim3(64), 0, h->stream, G);
  HIPCHK(h, hipGetLastError());
  GsFisherAccArgs F{h->tr.partial, an.pending, N.P, segments};
  hipLaunchKernelGGL(gs_k_fisher_accumulate, dim3((N.P + 255) / 256), dim3(256), 0, h->stream, F);
  HIPCHK(h, hipGetLastError());
  an.samples += n; Ln.n_last = n;      // (gs_learner_view shows this pass's per-sample arrays: the clip flags the Fisher was taken under)
  return publish(h, h->stream, Ln.ev, consumer_stream);
}

int gs_learner_fisher_commit(gs_handle* h, int32_t net, const gs_fisher_config* cfg) {
  gs_handle::Learner* Ln = nullptr;
  int rc = learner_of(h, net, "gs_learner_fisher_commit", &Ln);
  if (rc) return rc;
  if (!cfg) return fail(h, GS_E_INVALID, "gs_learner_fisher_commit: config is NULL");
  if (cfg->struct_size != (int32_t)sizeof(gs_fisher_config))
    return fail(h, GS_E_INVALID, "gs_fisher_config struct_size %d != %d", cfg->struct_size, (int)sizeof(gs_fisher_config));
  if (!std::isfinite(cfg->min_importance) || cfg->min_importance < 0.0) return fail(h, GS_E_INVALID, "gs_fisher_config: min_importance must be finite and >= 0");
  if (!(cfg->decay > 0.0 && cfg->decay <= 1.0)) return fail(h, GS_E_INVALID, "gs_fisher_config: decay must lie in (0, 1]");
  gs_handle::Learner::Anchor& an = Ln->an;
  if (!an.open) return fail(h, GS_E_STATE, "gs_learner_fisher_commit: no task is open for %s (gs_learner_fisher_begin)", net_name(net));
  if (an.samples <= 0) return fail(h, GS_E_STATE, "gs_learner_fisher_commit: the task of %s holds no samples (gs_learner_fisher_accumulate)", net_name(net));
  GS_ENTER(h);
  const int P = Ln->net.P;
  if (!an.tasks && (rc = alloc_all(h, "the consolidated importance and centre", an.importance.want((size_t)P), an.centre.want((size_t)P)))) return rc;
  GsFisherCommitArgs C{};
  C.pending = an.pending; C.params = Ln->params; C.importance = an.importance; C.centre = an.centre;
  C.samples = (double)an.samples; C.decay = cfg->decay; C.min_importance = (float)cfg->min_importance; C.first = an.tasks == 0; C.P = P;
  hipLaunchKernelGGL(gs_k_fisher_commit, dim3((P + 255) / 256), dim3(256), 0, h->stream, C);
  HIPCHK(h, hipGetLastError());
  an.tasks += 1; an.open = false;
  return GS_OK;
}

int gs_learner_anchor_clear(gs_handle* h, int32_t net, int32_t which) {
  gs_handle::Learner* Ln = nullptr;
  int rc = learner_of(h, net, "gs_learner_anchor_clear", &Ln);
  if (rc) return rc;
  if (which < 1 || which > (GS_ANCHOR_PROX | GS_ANCHOR_EWC)) return fail(h, GS_E_INVALID, "gs_learner_anchor_clear: which = %d is not GS_ANCHOR_PROX, GS_ANCHOR_EWC or both", which);
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));      // (a queued step still reads the arrays)
  if (which & GS_ANCHOR_PROX) Ln->an.drop_prox();
  if (which & GS_ANCHOR_EWC) Ln->an.drop_ewc();
  return GS_OK;
}

int gs_learner_anchor_stats(gs_handle* h, int32_t net, gs_learner_anchor_stats_out* out) {
  gs_handle::Learner* Ln = nullptr;
  int rc = learner_of(h, net, "gs_learner_anchor_stats", &Ln);
  if (rc) return rc;
  if (!out) return fail(h, GS_E_INVALID, "gs_learner_anchor_stats: out is NULL");
  gs_handle::Learner::Anchor& an = Ln->an;
  if (!an.stepped) return fail(h, GS_E_STATE, "gs_learner_anchor_stats: %s has taken no step with a non-zero coefficient", net_name(net));
  GS_ENTER(h);
  const int blocks = gs_tr_red_blocks(Ln->net.P);
  std::vector<double> s((size_t)3 * blocks);
  HIPCHK(h, hipMemcpyAsync(s.data(), an.sums, s.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  double prox = 0.0, ewc = 0.0;
  for (int k = 0; k < blocks; ++k) { prox = prox + s[(size_t)blocks + k]; ewc = ewc + s[(size_t)2 * blocks + k]; }
  *out = gs_learner_anchor_stats_out{};
  out->penalty_prox = (an.step_mu / 2.0) * prox; out->penalty_ewc = (an.step_lambda / 2.0) * ewc;
  out->grad_norm_loss = std::sqrt(stat_tree_sum(s.data(), blocks));
  out->prox_mu = an.step_mu; out->ewc_lambda = an.step_lambda;
  out->tasks = an.tasks; out->fisher_samples = an.samples;
  return GS_OK;
}

int gs_learner_anchor_download(gs_handle* h, int32_t net, float* prox, float* ewc_importance, float* ewc_centre, double* fisher_pending) {
  gs_handle::Learner* Ln = nullptr;
  int rc = learner_of(h, net, "gs_learner_anchor_download", &Ln);
  if (rc) return rc;
  const gs_handle::Learner::Anchor& an = Ln->an;
  if (prox && !an.have_prox) return fail(h, GS_E_STATE, "gs_learner_anchor_download: %s has no PROX centre", net_name(net));
  if ((ewc_importance || ewc_centre) && !an.tasks) return fail(h, GS_E_STATE, "gs_learner_anchor_download: no task has been committed for %s", net_name(net));
  if (fisher_pending && !an.pending.p) return fail(h, GS_E_STATE, "gs_learner_anchor_download: %s holds no pending Fisher sum", net_name(net));
  GS_ENTER(h);
  const size_t P = (size_t)Ln->net.P;
  if (prox) HIPCHK(h, hipMemcpyAsync(prox, an.prox, P * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (ewc_importance) HIPCHK(h, hipMemcpyAsync(ewc_importance, an.importance, P * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (ewc_centre) HIPCHK(h, hipMemcpyAsync(ewc_centre, an.centre, P * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (fisher_pending) HIPCHK(h, hipMemcpyAsync(fisher_pending, an.pending, P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

}  // extern "C"
