// abi_batches.hip -- on-policy minibatch epochs (include/gridstep.h): gs_onpolicy_prepare over the last
// rollout (the combined advantage and its statistics through the dataset's reduction pair, the observation normalisation),
// gs_onpolicy_stats, and gs_onpolicy_batch (the kernels of kernels_batches.hip).  The handle's minibatch buffers (handle.h) are made
// here and released here (batches_release).
#include <cmath>
#include <cstring>

#include "handle.h"

using namespace gsi;

static_assert(GS_OPB_NORM_NONE == GS_ADVNORM_NONE && GS_OPB_NORM_ROLLOUT == GS_ADVNORM_ROLLOUT && GS_OPB_NORM_MINIBATCH == GS_ADVNORM_MINIBATCH,
              "the kernels' copies of the public constants");
static_assert(sizeof(gs_onpolicy_batch_config) == 64, "gs_onpolicy_batch_config: four int32, four doubles, two pointers");

namespace gsi __attribute__((visibility("hidden"))) {

void batches_release(gs_handle* h) {
  gs_handle::OnPolicyBatches& ob = h->opb;
  ob.comb.release(); ob.part.release(); ob.stats.release(); ob.norm.release(); ob.stage.release(); ob.adv_stats.release(); ob.idx.release();
  for (DevBuf<char>& b : ob.field) b.release();
  if (ob.ev) { (void)hipEventDestroy(ob.ev); ob.ev = nullptr; }
  if (ob.ev_norm) { (void)hipEventDestroy(ob.ev_norm); ob.ev_norm = nullptr; }
  ob.norm_pending = false;
  ob.prepared_on = 0; ob.N = 0; ob.have_norm = false; ob.chan = 0;
}

}  // namespace gsi

// the scalar fields in the order the gather's lanes take them (GS_OPB_SCALARS): their bit of gs_onpolicy_batch_config::fields
static const uint32_t kScalarBit[GS_OPB_SCALARS] = {
    GS_ONPOLICY_LOG_PROBS, GS_ONPOLICY_ADVANTAGES, GS_ONPOLICY_RETURNS, GS_ONPOLICY_VALUES,
    GS_ONPOLICY_COST_ADVANTAGES, GS_ONPOLICY_COST_ADVANTAGES, GS_ONPOLICY_COST_ADVANTAGES,
    GS_ONPOLICY_COST_RETURNS, GS_ONPOLICY_COST_RETURNS, GS_ONPOLICY_COST_RETURNS};

extern "C" {

int gs_onpolicy_prepare(gs_handle* h, const gs_onpolicy_batch_config* cfg) {
  if (!h || !cfg) return fail(h, GS_E_INVALID, "handle / config is NULL");
  if (cfg->struct_size != (int32_t)sizeof(gs_onpolicy_batch_config))
    return fail(h, GS_E_INVALID, "gs_onpolicy_batch_config struct_size %d != %d", cfg->struct_size, (int)sizeof(gs_onpolicy_batch_config));
  if (cfg->adv_norm != GS_ADVNORM_NONE && cfg->adv_norm != GS_ADVNORM_ROLLOUT && cfg->adv_norm != GS_ADVNORM_MINIBATCH)
    return fail(h, GS_E_INVALID, "gs_onpolicy_batch_config adv_norm = %d outside 0 .. 2", cfg->adv_norm);
  if (cfg->dtype != GS_COMPUTE_F64 && cfg->dtype != GS_COMPUTE_F32) return fail(h, GS_E_INVALID, "gs_onpolicy_batch_config: unknown dtype %d", cfg->dtype);
  if (cfg->fields & ~(uint32_t)GS_ONPOLICY_ALL_FIELDS) return fail(h, GS_E_INVALID, "gs_onpolicy_batch_config: unknown field bits 0x%x", cfg->fields);
  for (int c = 0; c < 3; ++c)
    if (!std::isfinite(cfg->lambda[c])) return fail(h, GS_E_INVALID, "gs_onpolicy_batch_config: lambda[%d] is not finite", c);
  if (!std::isfinite(cfg->adv_eps) || cfg->adv_eps < 0.0) return fail(h, GS_E_INVALID, "gs_onpolicy_batch_config: adv_eps must be finite and >= 0");
  if ((cfg->obs_shift == nullptr) != (cfg->obs_scale == nullptr))
    return fail(h, GS_E_INVALID, "gs_onpolicy_batch_config: obs_shift and obs_scale go together (both or neither)");
  const int D = h->obs_dim;
  if (cfg->obs_shift)
    for (int c = 0; c < D; ++c)
      if (!std::isfinite(cfg->obs_shift[c]) || !std::isfinite(cfg->obs_scale[c]))
        return fail(h, GS_E_INVALID, "gs_onpolicy_batch_config: obs_shift / obs_scale of column %d is not finite", c);
  gs_handle::Rollout& ro = h->ro;
  gs_handle::OnPolicyBatches& ob = h->opb;
  if (ro.T <= 0 || ro.calls == 0) return fail(h, GS_E_STATE, "gs_onpolicy_prepare: no rollout has been collected on this handle");
  const long long N = (long long)ro.T * h->B;
  if (N >= (1ll << 31)) return fail(h, GS_E_INVALID, "gs_onpolicy_prepare: %lld transitions (an epoch indexes fewer than 2^31)", N);
  if (!critic_current(h, h->critic[0])) return fail(h, GS_E_STATE, "gs_onpolicy_prepare: gs_rollout_evaluate has not run on the last rollout");
  const bool cost_fields = (cfg->fields & (GS_ONPOLICY_COST_ADVANTAGES | GS_ONPOLICY_COST_RETURNS)) != 0;
  int chan = 0;
  for (int c = 0; c < 3; ++c) {
    const bool current = critic_current(h, h->critic[1 + c]);
    if (cfg->lambda[c] != 0.0 && !current)
      return fail(h, GS_E_STATE, "gs_onpolicy_prepare: lambda[%d] != 0, but gs_rollout_evaluate_costs has not evaluated channel %d on the last rollout", c, c);
    if (cost_fields && current) chan |= 1 << c;
  }
  if (cost_fields && !chan)
    return fail(h, GS_E_STATE, "gs_onpolicy_prepare: a cost field is asked for, but gs_rollout_evaluate_costs has evaluated no channel on the last rollout");
  if ((cfg->fields & GS_ONPOLICY_LOG_PROBS) && !ro.logp_recorded)
    return fail(h, GS_E_STATE, "gs_onpolicy_prepare: GS_ONPOLICY_LOG_PROBS, but the last rollout recorded no log-probabilities (a stochastic GS_POLICY_MLP rollout does)");
  GS_ENTER(h);
  ob.prepared_on = 0;        // (until every launch is queued)
  int rc = GS_OK;
  const long long chunks = (N + GS_DS_ROWS_PER_CHUNK - 1) / GS_DS_ROWS_PER_CHUNK;
  const size_t Ds = (size_t)((D + 1) & ~1);
  if ((rc = ob.comb.grow(h, (size_t)ro.T_cap * h->B, "the combined advantage"))) return rc;
  if ((rc = ob.part.grow(h, (size_t)chunks * 2, "the combined advantage's partial statistics"))) return rc;
  if ((rc = ob.stats.grow(h, 2, "the combined advantage's statistics"))) return rc;
  if (cfg->obs_shift) {
    if ((rc = ob.norm.grow(h, 2 * Ds, "the minibatch's observation normalisation"))) return rc;
    if (ob.norm_pending) { HIPCHK(h, hipEventSynchronize(ob.ev_norm)); ob.norm_pending = false; }      // the staging copy of the call before
    if (!ob.ev_norm) HIPCHK(h, hipEventCreateWithFlags(&ob.ev_norm, hipEventDisableTiming));
    ob.h_norm.assign(2 * Ds, 0.0);
    memcpy(ob.h_norm.data(), cfg->obs_shift, D * sizeof(double));
    memcpy(ob.h_norm.data() + Ds, cfg->obs_scale, D * sizeof(double));
    HIPCHK(h, hipMemcpyAsync(ob.norm, ob.h_norm.data(), 2 * Ds * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(ob.ev_norm, h->stream));
    ob.norm_pending = true;
  }
  GsOpbCombineArgs C{};
  C.adv = h->critic[0].adv; C.comb = ob.comb; C.N = N;
  for (int c = 0; c < 3; ++c) { C.lambda[c] = cfg->lambda[c]; C.cadv[c] = cfg->lambda[c] != 0.0 ? h->critic[1 + c].adv.p : nullptr; }
  hipLaunchKernelGGL(gs_k_opb_combine, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, C);
  HIPCHK(h, hipGetLastError());
  // mean and standard deviation of comb, an [N][1] matrix, through the dataset's fixed tree (section 14)
  GsDsStatArgs S{};
  S.m[0] = GsDsMatrix{ob.comb, 1, 0, 1, 0};
  S.m[1] = GsDsMatrix{nullptr, 0, 1, 0, 0};
  S.m[2] = GsDsMatrix{nullptr, 0, 1, 0, 0};
  S.part = ob.part; S.N = N; S.chunks = chunks; S.Ct = 1;
  hipLaunchKernelGGL(gs_k_ds_chunk_stats, dim3((unsigned)((chunks + 3) / 4)), dim3(256), 0, h->stream, S);
  HIPCHK(h, hipGetLastError());
  for (long long stride = 1;; stride *= 16) {
    const long long nodes = (chunks + stride - 1) / stride, groups = (nodes + 15) / 16;
    const bool last = groups == 1;
    hipLaunchKernelGGL(gs_k_ds_merge, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, h->stream, ob.part.p, chunks, 1, stride, N,
                       S.m[0], S.m[1], S.m[2], last ? ob.stats.p : (double*)nullptr, last ? ob.stats + 1 : (double*)nullptr);
    HIPCHK(h, hipGetLastError());
    if (last) break;
  }
  ob.cfg = *cfg; ob.cfg.obs_shift = nullptr; ob.cfg.obs_scale = nullptr;
  ob.have_norm = cfg->obs_shift != nullptr; ob.chan = chan; ob.N = N;
  ob.prepared_on = ro.calls;
  return GS_OK;
}

int gs_onpolicy_stats(gs_handle* h, gs_onpolicy_stats_out* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::OnPolicyBatches& ob = h->opb;
  if (!ob.prepared_on || ob.prepared_on != h->ro.calls) return fail(h, GS_E_STATE, "gs_onpolicy_stats: gs_onpolicy_prepare has not run on the last rollout");
  GS_ENTER(h);
  double st[2];
  HIPCHK(h, hipMemcpyAsync(st, ob.stats, sizeof(st), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  out->n = ob.N; out->adv_mean = st[0]; out->adv_std = st[1];
  return GS_OK;
}

int gs_onpolicy_batch(gs_handle* h, uint64_t seed, uint32_t epoch, int64_t first, int32_t n, gs_onpolicy_batch_out* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  gs_handle::OnPolicyBatches& ob = h->opb;
  const gs_handle::Rollout& ro = h->ro;
  if (!ob.prepared_on || ob.prepared_on != ro.calls) return fail(h, GS_E_STATE, "gs_onpolicy_batch: gs_onpolicy_prepare has not run on the last rollout");
  const long long N = ob.N;
  if (n <= 0 || first < 0 || first > N - n)
    return fail(h, GS_E_INVALID, "gs_onpolicy_batch: positions %lld .. %lld + %d outside [0, %lld)", (long long)first, (long long)first, n, N);
  GS_ENTER(h);
  int rc = GS_OK;
  const gs_onpolicy_batch_config& cfg = ob.cfg;
  const uint32_t fields = cfg.fields;
  const int D = h->obs_dim, A = h->action_dim;
  const size_t esz = cfg.dtype == GS_COMPUTE_F32 ? sizeof(float) : sizeof(double);
  // where every wanted field goes: the caller's memory, or the handle's own buffer (grown before anything of this call is queued)
  void** slots[2 + GS_OPB_SCALARS] = {&out->observations, &out->actions, &out->log_probs, &out->advantages, &out->returns, &out->values,
                                      &out->cost_advantages[0], &out->cost_advantages[1], &out->cost_advantages[2],
                                      &out->cost_returns[0], &out->cost_returns[1], &out->cost_returns[2]};
  void* dst[2 + GS_OPB_SCALARS] = {};
  bool wanted[2 + GS_OPB_SCALARS] = {};
  wanted[0] = (fields & GS_ONPOLICY_OBSERVATIONS) != 0; wanted[1] = (fields & GS_ONPOLICY_ACTIONS) != 0;
  for (int k = 0; k < GS_OPB_SCALARS; ++k) {
    wanted[2 + k] = (fields & kScalarBit[k]) != 0;
    if (k >= 4) wanted[2 + k] = wanted[2 + k] && (ob.chan >> ((k - 4) % 3) & 1);
  }
  for (int k = 0; k < 2 + GS_OPB_SCALARS; ++k) {
    if (!wanted[k]) continue;
    dst[k] = *slots[k];
    if (dst[k]) continue;
    const size_t width = k == 0 ? (size_t)D : k == 1 ? (size_t)std::max(A, 1) : 1;
    if ((rc = ob.field[k].grow(h, (size_t)n * width * esz, "the minibatch"))) return rc;
    dst[k] = ob.field[k].p;
  }
  const bool want_adv = wanted[2 + GS_OPB_SC_ADV];
  int32_t* idx = (fields & GS_ONPOLICY_INDICES) ? out->indices : nullptr;
  if (!idx) { if ((rc = ob.idx.grow(h, (size_t)n, "the minibatch's indices"))) return rc; idx = ob.idx; }
  double* adv_stats = want_adv ? out->adv_stats : nullptr;
  if (want_adv) {
    if ((rc = ob.stage.grow(h, (size_t)n, "the minibatch's staged advantages"))) return rc;
    if (!adv_stats) { if ((rc = ob.adv_stats.grow(h, 2, "the minibatch's advantage statistics"))) return rc; adv_stats = ob.adv_stats; }
  }

  GsOpbIndexArgs I{};
  I.comb = want_adv ? ob.comb.p : nullptr; I.roll_stats = ob.stats; I.idx = idx; I.stage = ob.stage; I.adv_stats = adv_stats;
  I.seed_lo = (uint32_t)seed; I.seed_hi = (uint32_t)(seed >> 32); I.epoch = epoch;
  I.half_bits = 1;
  while ((1ll << (2 * I.half_bits)) < N) I.half_bits += 1;
  I.N = N; I.first = first; I.n = n; I.adv_norm = cfg.adv_norm;
  hipLaunchKernelGGL(gs_k_opb_index, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, I);
  HIPCHK(h, hipGetLastError());
  if (want_adv && cfg.adv_norm == GS_ADVNORM_MINIBATCH) {
    hipLaunchKernelGGL(gs_k_opb_mbstats, dim3(1), dim3(GS_OPB_STAT_THREADS), 0, h->stream, (const double*)ob.stage.p, (int)n, adv_stats);
    HIPCHK(h, hipGetLastError());
  }
  bool any = false;
  for (int k = 0; k < 2 + GS_OPB_SCALARS; ++k) any = any || wanted[k];
  if (any) {
    GsOpbGatherArgs G{};
    G.idx = idx; G.obs_seq = ro.obs_seq; G.act = ro.act;
    if (ob.have_norm) { G.shift = ob.norm; G.scale = ob.norm + ((D + 1) & ~1); }
    G.out_obs = dst[0]; G.out_act = A > 0 ? dst[1] : nullptr;
    const double* src[GS_OPB_SCALARS] = {ro.logp, ob.comb, h->critic[0].ret, h->critic[0].values,
                                         h->critic[1].adv, h->critic[2].adv, h->critic[3].adv, h->critic[1].ret, h->critic[2].ret, h->critic[3].ret};
    for (int k = 0; k < GS_OPB_SCALARS; ++k) { G.sc_dst[k] = dst[2 + k]; G.sc_src[k] = dst[2 + k] ? src[k] : nullptr; }
    G.stage = ob.stage; G.adv_stats = adv_stats; G.adv_eps = cfg.adv_eps;
    G.N = N; G.n = n; G.D = D; G.A = A; G.adv_norm = cfg.adv_norm;
    // column pairs (16-byte loads, 8-byte stores) where every row starts on such a boundary; single columns otherwise
    G.vec2 = (D % 2 == 0) && !((uintptr_t)dst[0] & 7);
    const int per_group = GS_OPB_WAVES * GS_OPB_SAMPLES;
    const dim3 grid((unsigned)((n + per_group - 1) / per_group)), block(64 * GS_OPB_WAVES);
    if (cfg.dtype == GS_COMPUTE_F32) hipLaunchKernelGGL(gs_k_opb_gather_f32, grid, block, 0, h->stream, G);
    else hipLaunchKernelGGL(gs_k_opb_gather_f64, grid, block, 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
  }
  if ((rc = publish(h, h->stream, ob.ev, consumer_stream))) return rc;
  for (int k = 0; k < 2 + GS_OPB_SCALARS; ++k) if (wanted[k]) *slots[k] = dst[k];
  if (fields & GS_ONPOLICY_INDICES) out->indices = idx;
  if (want_adv) out->adv_stats = adv_stats;
  return GS_OK;
}

}  // extern "C"
