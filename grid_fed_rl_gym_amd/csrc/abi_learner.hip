// abi_learner.hip -- the learner (include/gridstep.h "the learner"): gs_learner_create snapshots an installed
// network into master parameters, gs_learner_step queues one update on the minibatch gs_onpolicy_batch left (the kernels of
// kernels_train.hip; with gs_learner_set_loss the head and its statistics are those of kernels_train_offline.hip, DESIGN.md section
// 21; a Q learner's input rows and targets, and the heads' Q-based signals of gs_learner_set_signal, are gathered first by
// gs_k_q_gather of kernels_q.hip, section 22), gs_learner_stats / _info / _download / _view read what it left.  gs_learner_step_pathwise is the
// policy's step whose gradient flows through the twins (kernels_pathwise.hip, section 23), gs_learner_step_conservative a twin's step
// with the logsumexp penalty over 3 n rows (kernels_conservative.hip, section 26).  All steps run one pipeline: the checks on
// the minibatches, the growth of h->tr and every launch of kernels_train.hip (queue_*) are file-local helpers, stated once; a step adds
// its head and statistics.  gs_learner_step's own part from its checks through the backward-data pass is learner_backprop (handle.h),
// which gs_learner_fisher_accumulate of abi_anchor.hip calls too; queue_grad_reduce queues abi_anchor.hip's term on the parameters behind
// the reduction while a coefficient is non-zero (section 31).  The table of the learners' networks (net_name, installed; handle.h) is defined here.  The learners' buffers
// are made and released here: parameters with the learner (learner_drop), what is sized by n with the rollout's (learner_scratch_release).
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"

using namespace gsi;

static_assert(sizeof(gs_learner_config) == 72, "gs_learner_config: two int32, eight doubles");
static_assert(sizeof(gs_learner_loss) == 32, "gs_learner_loss: two int32, three doubles");
static_assert(sizeof(gs_pathwise_config) == 40, "gs_pathwise_config: two int32, two doubles, a uint64, two uint32");
static_assert(sizeof(gs_conservative_config) == 32, "gs_conservative_config: two int32, a double, a uint64, two uint32");
static_assert(GS_POLICY_MAX_LAYERS == 4, "gs_learner_info_out::dims holds five widths");

namespace gsi __attribute__((visibility("hidden"))) {

static void learner_scratch_release_one(gs_handle::Learner& L) {
  L.lp_new.release(); L.ratio.release(); L.term0.release(); L.term1.release(); L.clipped.release();
  L.n_last = 0;
}

void learner_drop(gs_handle* h, int k) {
  gs_handle::Learner& L = h->learner[k];
  if (L.live) (void)hipStreamSynchronize(h->stream);      // (a queued step still reads and writes the parameters)
  L.params.release(); L.grad.release(); L.m.release(); L.v.release(); L.wt.release(); L.stats.release(); L.blocksum.release();
  learner_scratch_release_one(L);
  L.an.release();      // (the anchors are the learner's: DESIGN.md section 31)
  if (L.ev) { (void)hipEventDestroy(L.ev); L.ev = nullptr; }
  L.live = false; L.steps = 0; L.loss = gs_learner_loss{}; L.signal = GS_SIGNAL_BATCH;
  if (k == GS_LEARNER_POLICY || k == h->cq.net) h->cq.n_last = 0;      // (the conservative step's view names both learners)
}

void learner_scratch_release(gs_handle* h) {
  for (gs_handle::Learner& L : h->learner) learner_scratch_release_one(L);
  h->tr.acts.release(); h->tr.deltas.release(); h->tr.partial.release(); h->tr.qsa.release(); h->tr.qy.release();
  gs_handle::Pathwise& pw = h->pw;
  pw.acts.release(); pw.deltas.release(); pw.qsa.release(); pw.dqda.release(); pw.actions.release(); pw.noise.release(); pw.logp.release();
  pw.q.release(); pw.qmin.release(); pw.bc.release(); pw.terms.release(); pw.which.release();
  pw.n_last = 0;
  gs_handle::Conservative& cq = h->cq;
  cq.random.release(); cq.actions.release(); cq.noise.release(); cq.logp.release(); cq.q.release(); cq.weights.release(); cq.terms.release();
  cq.scalars.release(); cq.y.release();
  cq.n_last = 0;
}

void learner_release(gs_handle* h) {
  for (int k = 0; k < GS_LEARNER_COUNT; ++k) learner_drop(h, k);
  learner_scratch_release(h);
}

int train_grad_args(gs_handle* h, const GsTrainNet& N, const float* obs, int n, int D, GsTrainGradArgs& G) {
  const gs_handle::TrainScratch& tr = h->tr;
  G.N = N; G.obs = obs; G.acts = tr.acts; G.deltas = tr.deltas; G.partial = tr.partial; G.n = n; G.D = D;
  const int wide_in = 16 * GS_TR_WT, wide_out = 16 * GS_TR_WT_OUT;
  int blocks = 0;
  for (int l = 0; l < N.n_layers; ++l) {
    G.blk0[l] = blocks;
    G.in_blocks[l] = (N.dims[l] + wide_in - 1) / wide_in;
    blocks += ((N.dims[l + 1] + wide_out - 1) / wide_out) * G.in_blocks[l];
  }
  G.blk0[N.n_layers] = blocks;
  return blocks;
}

const char* net_name(int net) {
  static const char* names[] = {"the policy", "the value network", "the cost critic of channel 0", "the cost critic of channel 1", "the cost critic of channel 2",
                                 "Q network 0", "Q network 1"};
  return names[net];
}

bool installed(const gs_handle* h, int net, Installed& I) {
  if (net == GS_LEARNER_POLICY) {
    const gs_handle::Policy& p = h->pol;
    if (!p.set || p.compute != GS_COMPUTE_F32) return false;
    I = Installed{p.args32.L, p.dims, p.args32.n_layers, p.args32.activation, &p.h_norm, &p.blob};
    return true;
  }
  const gs_handle::Value& v = net >= GS_LEARNER_Q ? h->qnet[net - GS_LEARNER_Q].net : h->critic[net - 1].net;
  if (!v.set) return false;
  I = Installed{v.args.L, v.dims, v.args.n_layers, v.args.activation, &v.h_norm, &v.blob};
  return true;
}

}  // namespace gsi

namespace {

bool net_ok(int net) { return net >= 0 && net < GS_LEARNER_COUNT; }
bool net_is_q(int net) { return net >= GS_LEARNER_Q; }

// ---- the stages the two steps share, each stated once; `who` is the entry's name, for the message ----
// gs_onpolicy_prepare has run on the last rollout, in float32
int check_batches(gs_handle* h, const char* who) {
  const gs_handle::OnPolicyBatches& ob = h->opb;
  if (!ob.prepared_on || ob.prepared_on != h->ro.calls) return fail(h, GS_E_STATE, "%s: gs_onpolicy_prepare has not run on the last rollout", who);
  if (ob.cfg.dtype != GS_COMPUTE_F32) return fail(h, GS_E_STATE, "%s: the minibatches must be prepared with dtype GS_COMPUTE_F32", who);
  return GS_OK;
}

// the minibatches' shift and scale are, bit for bit, the normalisation learner `net`'s network `I` was installed with
int check_norm(gs_handle* h, const char* who, int net, const Installed& I) {
  const gs_handle::OnPolicyBatches& ob = h->opb;
  const int D = h->obs_dim, D16 = 16 * I.L[0].kb;
  const size_t Ds = (size_t)((D + 1) & ~1);
  for (int c = 0; c < D; ++c) {
    const double shift = ob.have_norm ? ob.h_norm[c] : 0.0, scale = ob.have_norm ? ob.h_norm[Ds + c] : 1.0;
    if (memcmp(&shift, &(*I.norm)[c], sizeof(double)) || memcmp(&scale, &(*I.norm)[D16 + c], sizeof(double)))
      return fail(h, GS_E_STATE, "%s: the minibatches' obs_shift / obs_scale differ from the normalisation of %s (column %d)", who, net_name(net), c);
  }
  return GS_OK;
}

// h->tr holds network N's saved activations, backward pass and partial gradients over n rows
int grow_scratch(gs_handle* h, const GsTrainNet& N, int n) {
  gs_handle::TrainScratch& tr = h->tr;
  int rc = GS_OK;
  if ((rc = tr.acts.grow(h, (size_t)n * N.row_stride, "the learner's saved activations"))) return rc;
  if ((rc = tr.deltas.grow(h, (size_t)n * N.row_stride, "the learner's backward pass"))) return rc;
  return tr.partial.grow(h, (size_t)gs_tr_segments(n) * N.P, "the learner's partial gradients");
}

int queue_forward(gs_handle* h, const GsTrainNet& N, const float* obs, float* acts, int n, int D) {
  GsTrainFwdArgs F{};
  F.N = N; F.obs = obs; F.acts = acts; F.n = n; F.D = D;
  F.obs_stride = gs_val_obs_stride(N.L[0].kb); F.panel_kb = gs_val_panel_kb(N.L[0].kb);
  hipLaunchKernelGGL(gs_k_train_forward, dim3((n + GS_TR_ROWS - 1) / GS_TR_ROWS), dim3(64 * GS_POL_WAVES), gs_tr_lds_bytes(N.L[0].kb), h->stream, F);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

// from the head gradient in the last layer's block of `deltas` down to layer 0; a one-layer network has nothing to pass back
int queue_bwd_data(gs_handle* h, const GsTrainNet& N, const float* acts, float* deltas, int n) {
  if (N.n_layers < 2) return GS_OK;
  GsTrainBwdArgs B{};
  B.N = N; B.acts = acts; B.deltas = deltas; B.n = n;
  hipLaunchKernelGGL(gs_k_train_bwd_data, dim3((n + GS_TR_ROWS - 1) / GS_TR_ROWS), dim3(64 * GS_POL_WAVES), 0, h->stream, B);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

// the weight gradients of h->tr's passes over the input rows `obs`, then their sum into Ln.grad.  Returns the reduction's workgroup
// count, which the statistics kernel needs, or (negative) the code of a failure
int queue_grad_reduce(gs_handle* h, gs_handle::Learner& Ln, const float* obs, int n, int D) {
  const GsTrainNet& N = Ln.net;
  gs_handle::TrainScratch& tr = h->tr;
  const int segments = gs_tr_segments(n);
  GsTrainGradArgs G{};
  const int blocks = train_grad_args(h, N, obs, n, D, G);
  hipLaunchKernelGGL(gs_k_train_grad, dim3(blocks, segments), dim3(64), 0, h->stream, G);
  HIPCHK(h, hipGetLastError());
  GsTrainReduceArgs R{tr.partial, Ln.grad, Ln.blocksum, N.P, segments};
  hipLaunchKernelGGL(gs_k_train_reduce, dim3(gs_tr_red_blocks(N.P)), dim3(GS_TR_RED_THREADS), 0, h->stream, R);
  HIPCHK(h, hipGetLastError());
  // the terms on the parameters (abi_anchor.hip): one more launch, only while a coefficient is non-zero
  if (Ln.an.mu != 0.0 || Ln.an.lambda != 0.0) {
    const int rc = anchor_queue(h, Ln);
    if (rc) return rc;
  }
  return gs_tr_red_blocks(N.P);
}

// Adam's step Ln.steps + 1 on Ln.grad and the norm in Ln.stats; the scalars in float64, each rounded once to float32
int queue_adam(gs_handle* h, gs_handle::Learner& Ln) {
  const gs_learner_config& cfg = Ln.cfg;
  const double t = (double)(Ln.steps + 1);
  GsTrainAdamArgs A{};
  A.N = Ln.net; A.params = Ln.params; A.grad = Ln.grad; A.m = Ln.m; A.v = Ln.v; A.stats = Ln.stats; A.max_grad_norm = cfg.max_grad_norm;
  A.wd = (float)cfg.weight_decay; A.b1 = (float)cfg.beta1; A.omb1 = (float)(1.0 - cfg.beta1); A.b2 = (float)cfg.beta2; A.omb2 = (float)(1.0 - cfg.beta2);
  A.bc2s = (float)std::sqrt(1.0 - std::pow(cfg.beta2, t)); A.eps = (float)cfg.eps; A.step = (float)(cfg.lr / (1.0 - std::pow(cfg.beta1, t)));
  hipLaunchKernelGGL(gs_k_train_adam, dim3((Ln.net.P + 255) / 256), dim3(256), 0, h->stream, A);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_learner_create(gs_handle* h, int32_t net, const gs_learner_config* cfg) {
  if (!h || !cfg) return fail(h, GS_E_INVALID, "handle / config is NULL");
  if (!net_ok(net)) return fail(h, GS_E_INVALID, "gs_learner_create: unknown net %d", net);
  if (cfg->struct_size != (int32_t)sizeof(gs_learner_config))
    return fail(h, GS_E_INVALID, "gs_learner_config struct_size %d != %d", cfg->struct_size, (int)sizeof(gs_learner_config));
  const double vals[] = {cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, cfg->weight_decay, cfg->max_grad_norm};
  for (double x : vals)
    if (!std::isfinite(x) || x < 0.0) return fail(h, GS_E_INVALID, "gs_learner_config: lr, beta1, beta2, eps, weight_decay and max_grad_norm must be finite and >= 0");
  if (cfg->beta1 >= 1.0 || cfg->beta2 >= 1.0) return fail(h, GS_E_INVALID, "gs_learner_config: beta1 and beta2 must lie in [0, 1)");
  if (net == GS_LEARNER_POLICY && (!std::isfinite(cfg->clip) || cfg->clip < 0.0 || !std::isfinite(cfg->ent_coef)))
    return fail(h, GS_E_INVALID, "gs_learner_config: clip must be finite and >= 0, ent_coef finite");
  Installed I{};
  if (!installed(h, net, I))
    return fail(h, GS_E_STATE, "gs_learner_create: %s is not installed%s", net_name(net), net == GS_LEARNER_POLICY ? " with GS_COMPUTE_F32" : "");
  if (net == GS_LEARNER_POLICY && !policy_rows_ready(h))
    return fail(h, GS_E_STATE, "gs_learner_create: the policy needs the Gaussian head (GS_HEAD_GAUSSIAN_TANH)");
  GS_ENTER(h);
  learner_drop(h, net);
  gs_handle::Learner& Ln = h->learner[net];
  GsTrainNet& N = Ln.net;
  N = GsTrainNet{};
  N.n_layers = I.n_layers; N.activation = I.activation;
  int stride = 0; long long P = 0; size_t wt_floats = 0;
  size_t wt_off[GS_POLICY_MAX_LAYERS] = {};
  for (int l = 0; l <= I.n_layers; ++l) N.dims[l] = I.dims[l];
  for (int l = 0; l < I.n_layers; ++l) {
    N.L[l] = I.L[l];
    N.col_off[l] = stride; stride += 16 * I.L[l].nt;
    N.p_off[l] = (int32_t)P; P += (long long)N.dims[l + 1] * (N.dims[l] + 1);
    if (l) { wt_off[l] = wt_floats; wt_floats += (size_t)I.L[l].kb * I.L[l].nt * 256; }
  }
  N.row_stride = stride; N.P = (int32_t)P;
  Ln.A = net == GS_LEARNER_POLICY ? h->action_dim : 0;
  int rc = alloc_all(h, "the learner's parameters", Ln.params.want((size_t)P), Ln.grad.want((size_t)P), Ln.m.want((size_t)P), Ln.v.want((size_t)P),
                     Ln.wt.want(wt_floats), Ln.stats.want(GS_TR_STAT_COUNT), Ln.blocksum.want((size_t)gs_tr_red_blocks(N.P)));
  if (rc) return rc;
  // the installed image, unpacked into torch order (the image holds float32 values: the snapshot is exact), and its transposes
  const float* const image = (const float*)I.blob->p;
  size_t image_floats = 0;
  for (int l = 0; l < I.n_layers; ++l) image_floats = std::max(image_floats, (size_t)(I.L[l].b - image) + 16 * (size_t)I.L[l].nt);
  std::vector<float> img(image_floats), flat((size_t)P), wt(std::max<size_t>(wt_floats, 1), 0.0f);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(img.data(), image, image_floats * sizeof(float), hipMemcpyDeviceToHost));
  for (int l = 0; l < I.n_layers; ++l) {
    const int kb = I.L[l].kb, nt = I.L[l].nt;
    const GsPolicyLayerF32 host{img.data() + (I.L[l].w - image), img.data() + (I.L[l].b - image), kb, nt};
    gs_policy_unpack_f32(host, N.dims[l + 1], N.dims[l], flat.data() + N.p_off[l], l ? wt.data() + wt_off[l] : nullptr);
    if (l) N.T[l] = GsPolicyLayerF32{Ln.wt.p + wt_off[l], nullptr, nt, kb};
  }
  HIPCHK(h, hipMemcpy(Ln.params, flat.data(), (size_t)P * sizeof(float), hipMemcpyHostToDevice));
  if (wt_floats) HIPCHK(h, hipMemcpy(Ln.wt, wt.data(), wt_floats * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemset(Ln.grad, 0, (size_t)P * sizeof(float)));
  HIPCHK(h, hipMemset(Ln.m, 0, (size_t)P * sizeof(float)));
  HIPCHK(h, hipMemset(Ln.v, 0, (size_t)P * sizeof(float)));
  HIPCHK(h, hipFuncSetAttribute((const void*)gs_k_train_forward, hipFuncAttributeMaxDynamicSharedMemorySize, GS_TR_LDS_MAX));
  Ln.cfg = *cfg; Ln.steps = 0; Ln.n_last = 0; Ln.loss = gs_learner_loss{};      // (GS_LOSS_DEFAULT)
  Ln.signal = GS_SIGNAL_BATCH;
  Ln.gen += 1;             // (a federation created on the learner before this one refuses it: abi_fed.hip)
  Ln.live = true;
  return GS_OK;
}

int gs_learner_step(gs_handle* h, int32_t net, const gs_onpolicy_batch_out* batch, int32_t n, void* consumer_stream) {
  if (!h || !batch) return fail(h, GS_E_INVALID, "handle / batch is NULL");
  LearnerPass ps{};
  int rc = learner_backprop(h, "gs_learner_step", net, batch, n, nullptr, ps);
  if (rc) return rc;
  gs_handle::Learner& Ln = h->learner[net];
  const gs_handle::OnPolicyBatches& ob = h->opb;
  const gs_handle::Rollout& ro = h->ro;
  const gs_learner_config& cfg = Ln.cfg;
  const bool policy = net == GS_LEARNER_POLICY;
  const int red_blocks = queue_grad_reduce(h, Ln, ps.rows, n, ps.Din);
  if (red_blocks < 0) return red_blocks;

  if (ps.loss == GS_LOSS_AWR) {
    GsTrainAwrStatArgs W{};
    W.term0 = Ln.term0; W.term1 = Ln.term1; W.lp_new = Ln.lp_new; W.logp = ro.logp_recorded ? ro.logp.p : nullptr; W.idx = batch->indices; W.capped = Ln.clipped;
    W.blocksum = Ln.blocksum; W.stats = Ln.stats; W.N = ob.N; W.n = n; W.blocks = red_blocks; W.ent_coef = cfg.ent_coef;
    hipLaunchKernelGGL(gs_k_train_stats_awr, dim3(1), dim3(GS_TR_STAT_THREADS), 0, h->stream, W);
  } else {                                   // (an expectile critic: a critic's sum of term0)
    GsTrainStatArgs S{};
    S.term0 = Ln.term0; S.term1 = Ln.term1; S.lp_new = Ln.lp_new; S.logp = ro.logp; S.idx = batch->indices; S.clipped = Ln.clipped;
    S.blocksum = Ln.blocksum; S.stats = Ln.stats; S.N = ob.N; S.n = n; S.blocks = red_blocks; S.policy = policy; S.ent_coef = cfg.ent_coef;
    hipLaunchKernelGGL(gs_k_train_stats, dim3(1), dim3(GS_TR_STAT_THREADS), 0, h->stream, S);
  }
  HIPCHK(h, hipGetLastError());

  if ((rc = queue_adam(h, Ln))) return rc;
  Ln.steps += 1; Ln.n_last = n;
  return publish(h, h->stream, Ln.ev, consumer_stream);
}

}  // extern "C"

// ---- gs_learner_step from its checks through the backward-data pass (handle.h): what the step and gs_learner_fisher_accumulate
// (abi_anchor.hip) share.  `who`: the entry's name, for the messages; `extra`: a check of the caller's that runs behind the step's own
// and before anything is launched (NULL: none).  Leaves Ln.n_last at 0: the step sets it once every launch is queued ----
int gsi::learner_backprop(gs_handle* h, const char* who, int32_t net, const gs_onpolicy_batch_out* batch, int32_t n, int (*extra)(gs_handle*, int32_t),
                          LearnerPass& ps) {
  if (!net_ok(net)) return fail(h, GS_E_INVALID, "%s: unknown net %d", who, net);
  if (n <= 0 || n > (1 << 24)) return fail(h, GS_E_INVALID, "%s: n = %d outside 1 .. 2^24", who, n);
  gs_handle::Learner& Ln = h->learner[net];
  Installed I{};
  if (!Ln.live || !installed(h, net, I)) return fail(h, GS_E_STATE, "%s: no learner for %s (gs_learner_create after the network was installed)", who, net_name(net));
  const gs_handle::OnPolicyBatches& ob = h->opb;
  const gs_handle::Rollout& ro = h->ro;
  int rc = GS_OK;
  if ((rc = check_batches(h, who))) return rc;
  if ((rc = check_norm(h, who, net, I))) return rc;
  const int D = h->obs_dim;
  const bool policy = net == GS_LEARNER_POLICY, qnet = net_is_q(net);
  // what the head regresses on or weights with: a field of the batch, or (a Q learner, GS_SIGNAL_Q) an array of gs_rollout_evaluate_q
  // gathered through the indices into tr.qy
  const bool gathered = qnet || Ln.signal == GS_SIGNAL_Q;
  const void* target = gathered ? nullptr : policy ? batch->advantages : net == GS_LEARNER_VALUE ? batch->returns : batch->cost_returns[net - GS_LEARNER_COST_VALUE];
  // (a Q learner under GS_Q_TARGET_POLICY regresses on gs_rollout_evaluate_q_next's target: DESIGN.md section 25)
  const bool policy_target = qnet && h->qn.target_source == GS_Q_TARGET_POLICY;
  if (policy_target && !q_next_current(h))
    return fail(h, GS_E_STATE, "%s: gs_rollout_evaluate_q_next has not run on the last rollout (%s reads its td_target under GS_Q_TARGET_POLICY)", who, net_name(net));
  if (gathered && !policy_target && !q_current(h)) return fail(h, GS_E_STATE, "%s: gs_rollout_evaluate_q has not run on the last rollout (%s reads its arrays)", who, net_name(net));
  const int loss = Ln.loss.kind;
  if (policy && loss == GS_LOSS_DEFAULT && !ro.logp_recorded) return fail(h, GS_E_STATE, "%s: the last rollout recorded no log-probabilities (a stochastic GS_POLICY_MLP rollout does)", who);
  if (!batch->observations || (!gathered && !target) || ((policy || gathered) && !batch->indices))
    return fail(h, GS_E_INVALID, "%s: the batch lacks %s", who, !batch->observations ? "observations" : (!gathered && !target) ? (policy ? "advantages" : "returns") : "indices");
  if (extra && (rc = extra(h, net))) return rc;
  GS_ENTER(h);
  const GsTrainNet& N = Ln.net;
  gs_handle::TrainScratch& tr = h->tr;
  if ((rc = grow_scratch(h, N, n))) return rc;
  if ((rc = Ln.term0.grow(h, (size_t)n, "the learner's loss terms"))) return rc;
  if (policy) {
    if ((rc = Ln.term1.grow(h, (size_t)n, "the learner's entropy terms"))) return rc;
    if ((rc = Ln.lp_new.grow(h, (size_t)n, "the learner's log-probabilities"))) return rc;
    if ((rc = Ln.ratio.grow(h, (size_t)n, "the learner's ratios"))) return rc;
    if ((rc = Ln.clipped.grow(h, (size_t)n, "the learner's clip flags"))) return rc;
  }
  const int Din = qnet ? D + h->action_dim : D;      // the width of an input row
  if (gathered && (rc = tr.qy.grow(h, (size_t)n, "the learner's gathered targets"))) return rc;
  if (qnet && (rc = tr.qsa.grow(h, (size_t)n * Din, "the Q learner's input rows"))) return rc;
  Ln.n_last = 0;           // (until every launch is queued)
  const int last = N.n_layers - 1;
  const gs_learner_config& cfg = Ln.cfg;

  if (gathered) {
    const size_t cap = (size_t)ro.T_cap * h->B;
    GsQGatherArgs Q{};
    Q.idx = batch->indices; Q.y = tr.qy; Q.N = ob.N; Q.n = n;
    Q.src = policy_target ? h->qn.td.p : qnet ? h->qt.td.p : policy ? h->qt.q_adv.p : h->qt.q_min.p + cap;      // td_target; q_adv; q_min[target]
    if (qnet) { Q.obs = (const float*)batch->observations; Q.act = ro.act; Q.sa = tr.qsa; Q.D = D; Q.DA = Din; }
    const long long total = (long long)n * (qnet ? Din : 1);
    hipLaunchKernelGGL(gs_k_q_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, Q);
    HIPCHK(h, hipGetLastError());
    target = tr.qy.p;
  }

  const float* const rows = qnet ? tr.qsa.p : (const float*)batch->observations;
  if ((rc = queue_forward(h, N, rows, tr.acts, n, Din))) return rc;

  // the head: one thread per sample on the pre-head values, dL/d(pre-head) into the last layer's block of deltas
  const float* const pre = tr.acts + N.col_off[last];
  float* const ghead = tr.deltas + N.col_off[last];
  const int width16 = 16 * N.L[last].nt;
  if (loss == GS_LOSS_AWR) {                 // (the heads of kernels_train_offline.hip: the same grid, the same arrays; AWR is the policy's)
    GsTrainAwrHeadArgs W{};
    W.pre = pre; W.ghead = ghead; W.n = n; W.row_stride = N.row_stride; W.width16 = width16; W.A = Ln.A;
    W.idx = batch->indices; W.act = ro.act; W.adv = (const float*)target; W.N = ob.N;
    W.temperature = Ln.loss.temperature; W.weight_max = Ln.loss.weight_max; W.ent_coef = cfg.ent_coef;
    W.lp_new = Ln.lp_new; W.weight = Ln.ratio; W.capped = Ln.clipped; W.term0 = Ln.term0; W.term1 = Ln.term1;
    hipLaunchKernelGGL(gs_k_train_head_awr, dim3((n + 63) / 64), dim3(64), 0, h->stream, W);
  } else if (loss == GS_LOSS_EXPECTILE) {    // (a critic's)
    GsTrainExpectileArgs E{};
    E.pre = pre; E.ghead = ghead; E.ret = (const float*)target; E.term0 = Ln.term0; E.n = n; E.row_stride = N.row_stride; E.width16 = width16;
    E.tau = Ln.loss.expectile;
    hipLaunchKernelGGL(gs_k_train_head_expectile, dim3((n + 63) / 64), dim3(64), 0, h->stream, E);
  } else {
    GsTrainHeadArgs H{};
    H.pre = pre; H.ghead = ghead; H.n = n; H.row_stride = N.row_stride; H.width16 = width16; H.A = Ln.A;
    H.term0 = Ln.term0;
    if (policy) {
      H.idx = batch->indices; H.act = ro.act; H.logp = ro.logp; H.adv = (const float*)target; H.N = ob.N;
      H.clip = cfg.clip; H.ent_coef = cfg.ent_coef;
      H.lp_new = Ln.lp_new; H.ratio = Ln.ratio; H.clipped = Ln.clipped; H.term1 = Ln.term1;
    } else {
      H.ret = (const float*)target;
    }
    hipLaunchKernelGGL(gs_k_train_head, dim3((n + 63) / 64), dim3(64), 0, h->stream, H);
  }
  HIPCHK(h, hipGetLastError());

  if ((rc = queue_bwd_data(h, N, tr.acts, tr.deltas, n))) return rc;
  ps.rows = rows; ps.Din = Din; ps.loss = loss;
  return GS_OK;
}

extern "C" {

int gs_learner_stats(gs_handle* h, int32_t net, gs_learner_stats_out* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  if (!net_ok(net)) return fail(h, GS_E_INVALID, "gs_learner_stats: unknown net %d", net);
  gs_handle::Learner& Ln = h->learner[net];
  if (!Ln.live || !Ln.steps) return fail(h, GS_E_STATE, "gs_learner_stats: %s has taken no step", net_name(net));
  GS_ENTER(h);
  double st[GS_TR_STAT_COUNT];
  HIPCHK(h, hipMemcpyAsync(st, Ln.stats, sizeof(st), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  out->loss = st[GS_TR_STAT_LOSS]; out->surrogate = st[GS_TR_STAT_SURR]; out->entropy = st[GS_TR_STAT_ENT]; out->approx_kl = st[GS_TR_STAT_KL];
  out->clip_fraction = st[GS_TR_STAT_CLIPFRAC]; out->value_loss = st[GS_TR_STAT_VLOSS]; out->grad_norm = st[GS_TR_STAT_GNORM];
  out->step = (double)Ln.steps;
  return GS_OK;
}

int gs_learner_info(gs_handle* h, int32_t net, gs_learner_info_out* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  if (!net_ok(net)) return fail(h, GS_E_INVALID, "gs_learner_info: unknown net %d", net);
  const gs_handle::Learner& Ln = h->learner[net];
  if (!Ln.live) return fail(h, GS_E_STATE, "gs_learner_info: no learner for %s", net_name(net));
  *out = gs_learner_info_out{};
  out->n_layers = Ln.net.n_layers; out->activation = Ln.net.activation;
  for (int l = 0; l <= Ln.net.n_layers; ++l) out->dims[l] = Ln.net.dims[l];
  out->rows_per_segment = GS_TR_SEG; out->param_count = Ln.net.P; out->step = (int64_t)Ln.steps;
  return GS_OK;
}

int gs_learner_download(gs_handle* h, int32_t net, float* params, float* grads, float* m, float* v) {
  if (!h) return fail(h, GS_E_INVALID, "handle is NULL");
  if (!net_ok(net)) return fail(h, GS_E_INVALID, "gs_learner_download: unknown net %d", net);
  const gs_handle::Learner& Ln = h->learner[net];
  if (!Ln.live) return fail(h, GS_E_STATE, "gs_learner_download: no learner for %s", net_name(net));
  GS_ENTER(h);
  const size_t bytes = (size_t)Ln.net.P * sizeof(float);
  if (params) HIPCHK(h, hipMemcpyAsync(params, Ln.params, bytes, hipMemcpyDeviceToHost, h->stream));
  if (grads) HIPCHK(h, hipMemcpyAsync(grads, Ln.grad, bytes, hipMemcpyDeviceToHost, h->stream));
  if (m) HIPCHK(h, hipMemcpyAsync(m, Ln.m, bytes, hipMemcpyDeviceToHost, h->stream));
  if (v) HIPCHK(h, hipMemcpyAsync(v, Ln.v, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

int gs_learner_view(gs_handle* h, int32_t net, gs_learner_view_out* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  if (!net_ok(net)) return fail(h, GS_E_INVALID, "gs_learner_view: unknown net %d", net);
  gs_handle::Learner& Ln = h->learner[net];
  if (!Ln.live || !Ln.n_last) return fail(h, GS_E_STATE, "gs_learner_view: %s holds no step's arrays", net_name(net));
  GS_ENTER(h);
  int rc = publish(h, h->stream, Ln.ev, consumer_stream);
  if (rc) return rc;
  const bool policy = net == GS_LEARNER_POLICY;
  *out = gs_learner_view_out{};
  out->n = Ln.n_last; out->loss_terms = Ln.term0;
  if (policy) { out->log_probs_new = Ln.lp_new; out->ratio = Ln.ratio; out->clipped = Ln.clipped; out->entropy_terms = Ln.term1; }
  return GS_OK;
}

// ---- the pathwise actor step (include/gridstep.h "the pathwise actor step"): the policy's forward pass, the
// kernels of kernels_pathwise.hip around one forward and one backward-data pass per installed twin (in the scratch of h->pw: the
// policy's saved activations in h->tr survive them), then the policy's backward pass, reduction, statistics and Adam as above ----
int gs_learner_step_pathwise(gs_handle* h, const gs_onpolicy_batch_out* batch, int32_t n, const gs_pathwise_config* cfg, void* consumer_stream) {
  if (!h || !batch || !cfg) return fail(h, GS_E_INVALID, "handle / batch / config is NULL");
  if (cfg->struct_size != (int32_t)sizeof(gs_pathwise_config))
    return fail(h, GS_E_INVALID, "gs_pathwise_config struct_size %d != %d", cfg->struct_size, (int)sizeof(gs_pathwise_config));
  if (!std::isfinite(cfg->alpha) || cfg->alpha < 0.0 || !std::isfinite(cfg->bc_coef) || cfg->bc_coef < 0.0)
    return fail(h, GS_E_INVALID, "gs_pathwise_config: alpha and bc_coef must be finite and >= 0");
  if (cfg->stochastic != 0 && cfg->stochastic != 1) return fail(h, GS_E_INVALID, "gs_pathwise_config: stochastic = %d outside 0 .. 1", cfg->stochastic);
  if (n <= 0 || n > (1 << 24)) return fail(h, GS_E_INVALID, "gs_learner_step_pathwise: n = %d outside 1 .. 2^24", n);
  gs_handle::Learner& Ln = h->learner[GS_LEARNER_POLICY];
  Installed I{};
  if (!Ln.live || !installed(h, GS_LEARNER_POLICY, I))
    return fail(h, GS_E_STATE, "gs_learner_step_pathwise: no learner for the policy (gs_learner_create after the network was installed)");
  const int D = h->obs_dim, A = h->action_dim, DA = D + A;
  if (A <= 0 || A > GS_PW_MAX_A) return fail(h, GS_E_STATE, "gs_learner_step_pathwise: action_dim = %d outside 1 .. %d", A, GS_PW_MAX_A);
  Installed IQ[2]{};
  bool have[2] = {false, false};
  for (int w = 0; w < 2; ++w) {
    if (!h->qnet[w].net.set) continue;
    if (!h->learner[GS_LEARNER_Q + w].live || !installed(h, GS_LEARNER_Q + w, IQ[w]))
      return fail(h, GS_E_STATE, "gs_learner_step_pathwise: no learner for %s (the backward pass reads its transposed images)", net_name(GS_LEARNER_Q + w));
    have[w] = true;
  }
  if (!have[0] && !have[1]) return fail(h, GS_E_STATE, "gs_learner_step_pathwise before gs_q_mlp_set: no Q network is installed");
  const gs_handle::OnPolicyBatches& ob = h->opb;
  const gs_handle::Rollout& ro = h->ro;
  int rc = GS_OK;
  if ((rc = check_batches(h, "gs_learner_step_pathwise"))) return rc;
  if ((rc = check_norm(h, "gs_learner_step_pathwise", GS_LEARNER_POLICY, I))) return rc;
  for (int w = 0; w < 2; ++w)
    if (have[w] && (rc = check_norm(h, "gs_learner_step_pathwise", GS_LEARNER_Q + w, IQ[w]))) return rc;
  const bool with_bc = cfg->bc_coef != 0.0;
  if (!batch->observations || (with_bc && !batch->indices))
    return fail(h, GS_E_INVALID, "gs_learner_step_pathwise: the batch lacks %s", !batch->observations ? "observations" : "indices (bc_coef != 0 reads the stored actions)");
  GS_ENTER(h);
  const GsTrainNet& N = Ln.net;
  gs_handle::TrainScratch& tr = h->tr;
  gs_handle::Pathwise& pw = h->pw;
  int q_stride = 0;
  for (int w = 0; w < 2; ++w)
    if (have[w]) q_stride = std::max(q_stride, (int)h->learner[GS_LEARNER_Q + w].net.row_stride);
  if ((rc = grow_scratch(h, N, n))) return rc;
  if ((rc = pw.acts.grow(h, (size_t)n * q_stride, "the actor step's saved activations of a twin"))) return rc;
  if ((rc = pw.deltas.grow(h, (size_t)n * q_stride, "the actor step's backward pass of a twin"))) return rc;
  if ((rc = pw.qsa.grow(h, (size_t)n * DA, "the actor step's input rows"))) return rc;
  if ((rc = pw.dqda.grow(h, (size_t)2 * n * A, "the actor step's dQ/da"))) return rc;
  if ((rc = pw.actions.grow(h, (size_t)n * A, "the actor step's actions"))) return rc;
  if ((rc = pw.noise.grow(h, (size_t)n * A, "the actor step's noise"))) return rc;
  if ((rc = pw.logp.grow(h, (size_t)n, "the actor step's log-probabilities"))) return rc;
  if ((rc = pw.q.grow(h, (size_t)2 * n, "the actor step's Q values"))) return rc;
  if ((rc = pw.qmin.grow(h, (size_t)n, "the actor step's minimum"))) return rc;
  if ((rc = pw.bc.grow(h, (size_t)n, "the actor step's cloning terms"))) return rc;
  if ((rc = pw.terms.grow(h, (size_t)n, "the actor step's loss terms"))) return rc;
  if ((rc = pw.which.grow(h, (size_t)n, "the actor step's choices"))) return rc;
  Ln.n_last = 0; pw.n_last = 0;              // (until every launch is queued; gs_learner_view's arrays are gs_learner_step's)
  const int last = N.n_layers - 1;
  const float* const obs = (const float*)batch->observations;

  // the policy's forward pass: its saved activations stay in tr.acts until its backward pass
  if ((rc = queue_forward(h, N, obs, tr.acts, n, D))) return rc;

  GsPwSampleArgs S{};
  S.pre = tr.acts + N.col_off[last]; S.actions = pw.actions; S.noise = pw.noise; S.logp = pw.logp; S.sa = pw.qsa;
  S.n = n; S.row_stride = N.row_stride; S.A = A; S.D = D; S.stochastic = cfg->stochastic; S.draw = cfg->draw; S.seed = cfg->seed;
  hipLaunchKernelGGL(gs_k_pw_sample, dim3((n + 63) / 64), dim3(64), 0, h->stream, S);
  HIPCHK(h, hipGetLastError());
  GsPwRowsArgs RW{obs, pw.qsa, n, D, DA, 0};
  hipLaunchKernelGGL(gs_k_pw_rows, dim3((unsigned)(((long long)n * D + 255) / 256)), dim3(256), 0, h->stream, RW);
  HIPCHK(h, hipGetLastError());

  // every installed twin: forward with saved activations, 1.0f at the head, backward to delta0, then through W0's action columns
  for (int w = 0; w < 2; ++w) {
    if (!have[w]) continue;
    const gs_handle::Learner& Lq = h->learner[GS_LEARNER_Q + w];
    const GsTrainNet& Q = Lq.net;
    const int qlast = Q.n_layers - 1;
    if ((rc = queue_forward(h, Q, pw.qsa, pw.acts, n, DA))) return rc;
    GsPwSeedArgs SD{pw.deltas + Q.col_off[qlast], n, Q.row_stride, 16 * Q.L[qlast].nt, 0};
    hipLaunchKernelGGL(gs_k_pw_seed, dim3((n + 63) / 64), dim3(64), 0, h->stream, SD);
    HIPCHK(h, hipGetLastError());
    if ((rc = queue_bwd_data(h, Q, pw.acts, pw.deltas, n))) return rc;
    GsPwInputGradArgs IG{};
    IG.delta0 = pw.deltas + Q.col_off[0]; IG.qpre = pw.acts + Q.col_off[qlast]; IG.W0 = Lq.params.p + Q.p_off[0];
    IG.dqda = pw.dqda + (size_t)w * n * A; IG.q = pw.q + (size_t)w * n;
    IG.n = n; IG.row_stride = Q.row_stride; IG.H0 = Q.dims[1]; IG.D = D; IG.A = A;
    hipLaunchKernelGGL(gs_k_pw_input_grad, dim3((unsigned)(((long long)n * A + GS_PW_THREADS - 1) / GS_PW_THREADS)), dim3(GS_PW_THREADS), 0, h->stream, IG);
    HIPCHK(h, hipGetLastError());
  }

  GsPwHeadArgs H{};
  H.pre = S.pre; H.ghead = tr.deltas + N.col_off[last]; H.actions = pw.actions; H.noise = pw.noise; H.logp = pw.logp;
  for (int w = 0; w < 2; ++w) { H.q[w] = have[w] ? pw.q.p + (size_t)w * n : nullptr; H.dqda[w] = have[w] ? pw.dqda.p + (size_t)w * n * A : nullptr; }
  H.idx = with_bc ? batch->indices : nullptr; H.act = ro.act; H.N = ob.N;
  H.n = n; H.row_stride = N.row_stride; H.width16 = 16 * N.L[last].nt; H.A = A; H.alpha = cfg->alpha; H.bc_coef = cfg->bc_coef;
  H.which = pw.which; H.qmin = pw.qmin; H.bc = pw.bc; H.terms = pw.terms;
  hipLaunchKernelGGL(gs_k_pw_head, dim3((n + 63) / 64), dim3(64), 0, h->stream, H);
  HIPCHK(h, hipGetLastError());

  // the policy's backward pass, reduction, statistics and Adam, as gs_learner_step's
  if ((rc = queue_bwd_data(h, N, tr.acts, tr.deltas, n))) return rc;
  const int red_blocks = queue_grad_reduce(h, Ln, obs, n, D);
  if (red_blocks < 0) return red_blocks;
  GsPwStatArgs ST{pw.terms, pw.qmin, pw.logp, Ln.blocksum, Ln.stats, n, red_blocks};
  hipLaunchKernelGGL(gs_k_pw_stats, dim3(1), dim3(GS_TR_STAT_THREADS), 0, h->stream, ST);
  HIPCHK(h, hipGetLastError());
  if ((rc = queue_adam(h, Ln))) return rc;
  Ln.steps += 1; pw.n_last = n; pw.installed = (have[0] ? 1 : 0) | (have[1] ? 2 : 0);
  return publish(h, h->stream, Ln.ev, consumer_stream);
}

int gs_learner_pathwise_view(gs_handle* h, gs_pathwise_view_out* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Learner& Ln = h->learner[GS_LEARNER_POLICY];
  gs_handle::Pathwise& pw = h->pw;
  if (!Ln.live || !pw.n_last) return fail(h, GS_E_STATE, "gs_learner_pathwise_view: the policy holds no pathwise step's arrays");
  GS_ENTER(h);
  int rc = publish(h, h->stream, Ln.ev, consumer_stream);
  if (rc) return rc;
  const size_t n = (size_t)pw.n_last, A = (size_t)h->action_dim;
  *out = gs_pathwise_view_out{};
  out->n = pw.n_last; out->action_dim = h->action_dim;
  out->pre_head = h->tr.acts + Ln.net.col_off[Ln.net.n_layers - 1]; out->pre_head_stride = Ln.net.row_stride;
  out->actions = pw.actions; out->noise = pw.noise; out->log_probs = pw.logp; out->q_min = pw.qmin; out->bc_terms = pw.bc; out->loss_terms = pw.terms;
  out->which = pw.which;
  out->installed = pw.installed;
  for (int w = 0; w < 2; ++w) {
    if (!(pw.installed >> w & 1)) continue;
    out->q[w] = pw.q + w * n; out->dq_da[w] = pw.dqda + w * n * A;
  }
  return GS_OK;
}

// ---- the conservative critic step (include/gridstep.h "the conservative critic step"): the policy's forward
// pass gives the policy block's actions, gs_k_q_gather the data block and the targets, gs_k_cql_rows the rest of the 3 n input rows;
// then the twin's forward pass, the logsumexp and the head of kernels_conservative.hip, and the twin's backward pass, reduction,
// statistics and Adam as above.  The policy's saved activations lie BEHIND the twin's 3 n rows in tr.acts (cq.pre_off): the view's
// pre-head values outlive the twin's passes ----
int gs_learner_step_conservative(gs_handle* h, int32_t net, const gs_onpolicy_batch_out* batch, int32_t n, const gs_conservative_config* cfg,
                                 void* consumer_stream) {
  const char* const who = "gs_learner_step_conservative";
  if (!h || !batch || !cfg) return fail(h, GS_E_INVALID, "handle / batch / config is NULL");
  if (cfg->struct_size != (int32_t)sizeof(gs_conservative_config))
    return fail(h, GS_E_INVALID, "gs_conservative_config struct_size %d != %d", cfg->struct_size, (int)sizeof(gs_conservative_config));
  if (net != GS_LEARNER_Q && net != GS_LEARNER_Q + 1) return fail(h, GS_E_INVALID, "%s: net %d is not GS_LEARNER_Q + {0, 1}", who, net);
  if (!std::isfinite(cfg->conservative_weight) || cfg->conservative_weight < 0.0)
    return fail(h, GS_E_INVALID, "gs_conservative_config: conservative_weight must be finite and >= 0");
  if (cfg->stochastic != 0 && cfg->stochastic != 1) return fail(h, GS_E_INVALID, "gs_conservative_config: stochastic = %d outside 0 .. 1", cfg->stochastic);
  if (n <= 0 || n > GS_CQL_MAX_N) return fail(h, GS_E_INVALID, "%s: n = %d outside 1 .. 2^24 / 3", who, n);
  gs_handle::Learner& Ln = h->learner[net];
  gs_handle::Learner& Lp = h->learner[GS_LEARNER_POLICY];
  Installed I{}, IP{};
  if (!Ln.live || !installed(h, net, I)) return fail(h, GS_E_STATE, "%s: no learner for %s (gs_learner_create after the network was installed)", who, net_name(net));
  if (Ln.loss.kind != GS_LOSS_DEFAULT) return fail(h, GS_E_STATE, "%s: the loss of %s must be GS_LOSS_DEFAULT (the penalty joins the squared error)", who, net_name(net));
  if (!Lp.live || !installed(h, GS_LEARNER_POLICY, IP) || !policy_rows_ready(h))
    return fail(h, GS_E_STATE, "%s: no learner for the policy (GS_COMPUTE_F32, GS_HEAD_GAUSSIAN_TANH: its forward pass gives the policy block's actions)", who);
  const int D = h->obs_dim, A = h->action_dim, DA = D + A;
  if (A <= 0 || A > GS_PW_MAX_A) return fail(h, GS_E_STATE, "%s: action_dim = %d outside 1 .. %d", who, A, GS_PW_MAX_A);
  const gs_handle::OnPolicyBatches& ob = h->opb;
  const gs_handle::Rollout& ro = h->ro;
  int rc = GS_OK;
  if ((rc = check_batches(h, who))) return rc;
  if ((rc = check_norm(h, who, GS_LEARNER_POLICY, IP))) return rc;
  if ((rc = check_norm(h, who, net, I))) return rc;
  const bool policy_target = h->qn.target_source == GS_Q_TARGET_POLICY;
  if (policy_target && !q_next_current(h))
    return fail(h, GS_E_STATE, "%s: gs_rollout_evaluate_q_next has not run on the last rollout (%s reads its td_target under GS_Q_TARGET_POLICY)", who, net_name(net));
  if (!policy_target && !q_current(h)) return fail(h, GS_E_STATE, "%s: gs_rollout_evaluate_q has not run on the last rollout (%s reads its td_target)", who, net_name(net));
  if (!batch->observations || !batch->indices) return fail(h, GS_E_INVALID, "%s: the batch lacks %s", who, !batch->observations ? "observations" : "indices");
  GS_ENTER(h);
  const GsTrainNet& N = Ln.net;
  const GsTrainNet& NP = Lp.net;
  gs_handle::TrainScratch& tr = h->tr;
  gs_handle::Conservative& cq = h->cq;
  const int rows = 3 * n;
  const size_t pre_off = (size_t)rows * N.row_stride;      // (a multiple of 16 floats: the policy's rows keep their alignment)
  if ((rc = tr.acts.grow(h, pre_off + (size_t)n * NP.row_stride, "the learner's saved activations"))) return rc;
  if ((rc = grow_scratch(h, N, rows))) return rc;
  if ((rc = tr.qsa.grow(h, (size_t)rows * DA, "the Q learner's input rows"))) return rc;
  if ((rc = cq.random.grow(h, (size_t)n * A, "the conservative step's uniform actions"))) return rc;
  if ((rc = cq.actions.grow(h, (size_t)n * A, "the conservative step's policy actions"))) return rc;
  if ((rc = cq.noise.grow(h, (size_t)n * A, "the conservative step's noise"))) return rc;
  if ((rc = cq.logp.grow(h, (size_t)n, "the conservative step's log-probabilities"))) return rc;
  if ((rc = cq.y.grow(h, (size_t)n, "the conservative step's targets"))) return rc;
  if ((rc = cq.q.grow(h, (size_t)rows, "the conservative step's values"))) return rc;
  if ((rc = cq.weights.grow(h, (size_t)rows, "the conservative step's softmax weights"))) return rc;
  if ((rc = cq.terms.grow(h, (size_t)n, "the conservative step's loss terms"))) return rc;
  if ((rc = cq.scalars.grow(h, 4, "the conservative step's scalars"))) return rc;
  Ln.n_last = 0; cq.n_last = 0;              // (until every launch is queued; gs_learner_view's arrays are gs_learner_step's)
  const float* const obs = (const float*)batch->observations;
  const int plast = NP.n_layers - 1, last = N.n_layers - 1;

  // the policy block's actions: the policy's forward pass, then section 23's sampling head under this step's tag
  float* const pacts = tr.acts + pre_off;
  if ((rc = queue_forward(h, NP, obs, pacts, n, D))) return rc;
  GsPwSampleArgs S{};
  S.pre = pacts + NP.col_off[plast]; S.actions = cq.actions; S.noise = cq.noise; S.logp = cq.logp; S.sa = tr.qsa + (size_t)2 * n * DA;
  S.n = n; S.row_stride = NP.row_stride; S.A = A; S.D = D; S.stochastic = cfg->stochastic; S.draw = cfg->draw; S.tag = GS_CQL_NOISE_TAG; S.seed = cfg->seed;
  hipLaunchKernelGGL(gs_k_pw_sample, dim3((n + 63) / 64), dim3(64), 0, h->stream, S);
  HIPCHK(h, hipGetLastError());

  // the data block and the targets (gs_learner_step's gather), then the other blocks' observations and the uniform actions
  GsQGatherArgs Q{};
  Q.idx = batch->indices; Q.y = cq.y; Q.N = ob.N; Q.n = n; Q.src = policy_target ? h->qn.td.p : h->qt.td.p;
  Q.obs = obs; Q.act = ro.act; Q.sa = tr.qsa; Q.D = D; Q.DA = DA;
  const unsigned elem_blocks = (unsigned)(((long long)n * DA + 255) / 256);
  hipLaunchKernelGGL(gs_k_q_gather, dim3(elem_blocks), dim3(256), 0, h->stream, Q);
  HIPCHK(h, hipGetLastError());
  GsCqlRowsArgs RW{obs, tr.qsa, cq.random, n, D, A, cfg->draw, cfg->seed};
  hipLaunchKernelGGL(gs_k_cql_rows, dim3(elem_blocks), dim3(256), 0, h->stream, RW);
  HIPCHK(h, hipGetLastError());

  if ((rc = queue_forward(h, N, tr.qsa, tr.acts, rows, DA))) return rc;
  const float* const qpre = tr.acts + N.col_off[last];
  GsCqlLseArgs LS{qpre, cq.scalars, n, N.row_stride};
  hipLaunchKernelGGL(gs_k_cql_lse, dim3(1), dim3(GS_TR_STAT_THREADS), 0, h->stream, LS);
  HIPCHK(h, hipGetLastError());
  GsCqlHeadArgs H{};
  H.qpre = qpre; H.ghead = tr.deltas + N.col_off[last]; H.y = cq.y; H.scalars = cq.scalars; H.q = cq.q; H.weights = cq.weights; H.terms = cq.terms;
  H.n = n; H.row_stride = N.row_stride; H.width16 = 16 * N.L[last].nt; H.cw = cfg->conservative_weight;
  hipLaunchKernelGGL(gs_k_cql_head, dim3((rows + 63) / 64), dim3(64), 0, h->stream, H);
  HIPCHK(h, hipGetLastError());

  if ((rc = queue_bwd_data(h, N, tr.acts, tr.deltas, rows))) return rc;
  const int red_blocks = queue_grad_reduce(h, Ln, tr.qsa, rows, DA);
  if (red_blocks < 0) return red_blocks;
  GsCqlStatArgs ST{cq.terms, cq.scalars, Ln.blocksum, Ln.stats, n, red_blocks, cfg->conservative_weight};
  hipLaunchKernelGGL(gs_k_cql_stats, dim3(1), dim3(GS_TR_STAT_THREADS), 0, h->stream, ST);
  HIPCHK(h, hipGetLastError());
  if ((rc = queue_adam(h, Ln))) return rc;
  Ln.steps += 1; cq.n_last = n; cq.net = net; cq.pre_off = pre_off;
  return publish(h, h->stream, Ln.ev, consumer_stream);
}

int gs_learner_conservative_view(gs_handle* h, gs_conservative_view_out* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::Conservative& cq = h->cq;
  if (!cq.n_last || !h->learner[cq.net].live || !h->learner[GS_LEARNER_POLICY].live)
    return fail(h, GS_E_STATE, "gs_learner_conservative_view: no Q learner holds a conservative step's arrays");
  gs_handle::Learner& Ln = h->learner[cq.net];
  const GsTrainNet& NP = h->learner[GS_LEARNER_POLICY].net;
  GS_ENTER(h);
  int rc = publish(h, h->stream, Ln.ev, consumer_stream);
  if (rc) return rc;
  *out = gs_conservative_view_out{};
  out->net = cq.net; out->n = cq.n_last; out->action_dim = h->action_dim;
  out->pre_head = h->tr.acts + cq.pre_off + NP.col_off[NP.n_layers - 1]; out->pre_head_stride = NP.row_stride;
  out->random_actions = cq.random; out->policy_actions = cq.actions; out->policy_noise = cq.noise; out->policy_log_probs = cq.logp;
  out->targets = cq.y; out->q = cq.q; out->weights = cq.weights; out->loss_terms = cq.terms; out->scalars = cq.scalars;
  return GS_OK;
}

// ---- the learner's loss (include/gridstep.h "the learner's loss"): host state only, read by the next step ----
int gs_learner_set_loss(gs_handle* h, int32_t net, const gs_learner_loss* loss) {
  if (!h || !loss) return fail(h, GS_E_INVALID, "handle / loss is NULL");
  if (!net_ok(net)) return fail(h, GS_E_INVALID, "gs_learner_set_loss: unknown net %d", net);
  if (loss->struct_size != (int32_t)sizeof(gs_learner_loss))
    return fail(h, GS_E_INVALID, "gs_learner_loss struct_size %d != %d", loss->struct_size, (int)sizeof(gs_learner_loss));
  const bool policy = net == GS_LEARNER_POLICY;
  if (loss->kind != GS_LOSS_DEFAULT && loss->kind != GS_LOSS_AWR && loss->kind != GS_LOSS_EXPECTILE)
    return fail(h, GS_E_INVALID, "gs_learner_set_loss: unknown kind %d", loss->kind);
  if (loss->kind == GS_LOSS_AWR && !policy) return fail(h, GS_E_INVALID, "gs_learner_set_loss: GS_LOSS_AWR is the policy's loss, not %s's", net_name(net));
  if (loss->kind == GS_LOSS_EXPECTILE && policy) return fail(h, GS_E_INVALID, "gs_learner_set_loss: GS_LOSS_EXPECTILE is a critic's loss, not the policy's");
  if (std::isnan(loss->temperature) || std::isnan(loss->weight_max) || std::isnan(loss->expectile))
    return fail(h, GS_E_INVALID, "gs_learner_loss: temperature, weight_max or expectile is NaN");
  if (loss->kind == GS_LOSS_AWR && (!(loss->temperature > 0.0) || !(loss->weight_max > 0.0)))
    return fail(h, GS_E_INVALID, "gs_learner_loss: GS_LOSS_AWR needs temperature > 0 and weight_max > 0 (+inf allowed)");
  if (loss->kind == GS_LOSS_EXPECTILE && !(loss->expectile > 0.0 && loss->expectile < 1.0))
    return fail(h, GS_E_INVALID, "gs_learner_loss: GS_LOSS_EXPECTILE needs 0 < expectile < 1");
  gs_handle::Learner& Ln = h->learner[net];
  if (!Ln.live) return fail(h, GS_E_STATE, "gs_learner_set_loss: no learner for %s", net_name(net));
  Ln.loss = *loss;        // (a queued step took its arguments by value: it keeps the loss it was queued with)
  return GS_OK;
}

// ---- the signal of the policy's and the reward critic's heads (include/gridstep.h "state-action critics"): host state, as the loss ----
int gs_learner_set_signal(gs_handle* h, int32_t net, int32_t signal) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (!net_ok(net)) return fail(h, GS_E_INVALID, "gs_learner_set_signal: unknown net %d", net);
  if (signal != GS_SIGNAL_BATCH && signal != GS_SIGNAL_Q) return fail(h, GS_E_INVALID, "gs_learner_set_signal: unknown signal %d", signal);
  if (signal == GS_SIGNAL_Q && net != GS_LEARNER_POLICY && net != GS_LEARNER_VALUE)
    return fail(h, GS_E_INVALID, "gs_learner_set_signal: GS_SIGNAL_Q is the policy's and the value network's, not %s's", net_name(net));
  gs_handle::Learner& Ln = h->learner[net];
  if (!Ln.live) return fail(h, GS_E_STATE, "gs_learner_set_signal: no learner for %s", net_name(net));
  Ln.signal = signal;     // (a queued step took its pointers by value: it keeps the signal it was queued with)
  return GS_OK;
}

int gs_learner_get_signal(gs_handle* h, int32_t net, int32_t* signal) {
  if (!h || !signal) return fail(h, GS_E_INVALID, "handle / signal is NULL");
  if (!net_ok(net)) return fail(h, GS_E_INVALID, "gs_learner_get_signal: unknown net %d", net);
  const gs_handle::Learner& Ln = h->learner[net];
  if (!Ln.live) return fail(h, GS_E_STATE, "gs_learner_get_signal: no learner for %s", net_name(net));
  *signal = Ln.signal;
  return GS_OK;
}

int gs_learner_get_loss(gs_handle* h, int32_t net, gs_learner_loss* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  if (!net_ok(net)) return fail(h, GS_E_INVALID, "gs_learner_get_loss: unknown net %d", net);
  const gs_handle::Learner& Ln = h->learner[net];
  if (!Ln.live) return fail(h, GS_E_STATE, "gs_learner_get_loss: no learner for %s", net_name(net));
  *out = Ln.loss;
  out->struct_size = (int32_t)sizeof(gs_learner_loss);
  return GS_OK;
}

}  // extern "C"
