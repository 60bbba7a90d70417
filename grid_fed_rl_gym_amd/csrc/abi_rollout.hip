// abi_rollout.hip -- closed-loop collection on the device (include/gridstep.h): the MLP policy (gs_policy_mlp_*) and gs_rollout
// with its views and downloads.  The policy's and the rollout's device buffers are made here and released here.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "handle.h"

using namespace gsi;

namespace gsi __attribute__((visibility("hidden"))) {

// the installed policy's image and the action block of gs_policy_mlp_eval (made by gs_policy_mlp_set_opts)
void policy_release(gs_handle* h) {
  h->pol.blob.release();
  h->pol.act.release();
  h->pol.set = false;
}

int upload_image_f32(gs_handle* h, DevBuf<char>& blob, const GsPolicyImageF32& im, const float** image, const double** norm) {
  // one allocation: the float image (a multiple of 16 floats), then shift and scale
  const size_t image_bytes = im.blob.size() * sizeof(float), norm_bytes = im.norm.size() * sizeof(double);
  int rc = blob.alloc(h, image_bytes + norm_bytes, "the network's float32 image");
  if (rc) return rc;
  HIPCHK(h, hipMemcpy(blob, im.blob.data(), image_bytes, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(blob + image_bytes, im.norm.data(), norm_bytes, hipMemcpyHostToDevice));
  *image = (const float*)blob.p; *norm = (const double*)(blob + image_bytes);
  return GS_OK;
}

// the rollout's buffers (made by rollout_ensure); keep_term_count: all but the 4-byte counter, which does not depend on T.
// The handle then holds no rollout: every gate on ro.T refuses until gs_rollout has collected one again.
void rollout_release(gs_handle* h, bool keep_term_count) {
  gs_handle::Rollout& ro = h->ro;
  ro.obs_seq.release(); ro.act.release(); ro.rew.release(); ro.done.release(); ro.term_idx.release(); ro.term_obs.release();
  if (!keep_term_count) ro.term_count.release();
  rollout_tracks_release(h, keep_term_count);
  ro.T_cap = 0; ro.T = 0; ro.n_term = -1;
}

void rollout_tracks_release(gs_handle* h, bool keep_carries) {
  onpolicy_release(h);           // (sized by T as well)
  costs_release(h);
  q_rollout_release(h);
  q_next_rollout_release(h);
  refresh_release(h);
  episodes_release(h, keep_carries);         // (the list is sized by the capacity; the carries outlive a longer rollout)
  batches_release(h);
  learner_scratch_release(h);
  window_release(h);
}

}  // namespace gsi

extern "C" {

// ---- the MLP policy (policy.h, kernels_policy.hip, kernels_policy_f32.hip) ------------------------------------------------------
int gs_policy_mlp_check(const gs_policy_mlp* p, int32_t obs_dim, int32_t action_dim) {
  const std::string why = gs_policy_check(p, obs_dim, action_dim);
  return why.empty() ? GS_OK : fail(nullptr, GS_E_INVALID, "%s", why.c_str());
}

int gs_policy_mlp_check_opts(const gs_policy_mlp* p, const gs_policy_mlp_opts* o, int32_t obs_dim, int32_t action_dim) {
  const std::string why = gs_policy_check_opts(p, o, obs_dim, action_dim);
  return why.empty() ? GS_OK : fail(nullptr, GS_E_INVALID, "%s", why.c_str());
}

int gs_policy_mlp_set(gs_handle* h, const gs_policy_mlp* p) { return gs_policy_mlp_set_opts(h, p, nullptr); }

int gs_policy_mlp_set_opts(gs_handle* h, const gs_policy_mlp* p, const gs_policy_mlp_opts* o) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (p) {         // (a refused policy leaves the installed one in place)
    const std::string why = gs_policy_check_opts(p, o, h->obs_dim, h->action_dim);
    if (!why.empty()) return fail(h, GS_E_INVALID, "%s", why.c_str());
  }
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  gs_handle::Policy& pol = h->pol;
  learner_drop(h, 0);              // (a learner trains the network it was created on)
  pol.blob.release();
  pol.set = false;
  h->qn.evaluated_on = 0;          // (the policy-action targets belong to the policy that was installed then)
  if (!p) return GS_OK;
  int rc = pol.act.grow(h, (size_t)h->B * h->action_dim, "the policy's actions");
  if (rc) return rc;
  if (gs_policy_is_f32(o)) {
    const GsPolicyImageF32 im = gs_policy_pack_f32(*p, *o);
    pol.lds32 = p->stochastic ? gs_pol32_lds_bytes(im.kb[0], h->action_dim) : gs_pol32_lds_bytes(im.kb[0]);
    HIPCHK(h, hipFuncSetAttribute((const void*)gs_k_policy_mlp_f32, hipFuncAttributeMaxDynamicSharedMemorySize, GS_POL32_LDS_MAX));
    const float* image = nullptr; const double* norm = nullptr;
    if ((rc = upload_image_f32(h, pol.blob, im, &image, &norm))) return rc;
    GsPolicyArgsF32& a = pol.args32;
    a = GsPolicyArgsF32{};
    a.shift = norm; a.scale = norm + 16 * im.kb[0];
    a.B = h->B; a.D = h->obs_dim; a.A = h->action_dim; a.n_layers = p->n_layers; a.activation = p->activation; a.head = p->head;
    a.stochastic = p->stochastic; a.first_instance = h->EC.first_instance; a.obs_stride = gs_pol32_obs_stride(im.kb[0]);
    for (int l = 0; l < p->n_layers; ++l) a.L[l] = GsPolicyLayerF32{image + im.w_off[l], image + im.b_off[l], im.kb[l], im.nt[l]};
    for (int l = 0; l <= p->n_layers; ++l) pol.dims[l] = p->dims[l];
    pol.h_norm = im.norm;
    pol.compute = GS_COMPUTE_F32;
    pol.set = true;
    return GS_OK;
  }
  const GsPolicyImage im = gs_policy_pack(*p);
  pol.lds64 = p->stochastic ? gs_pol_lds_bytes(h->action_dim) : GS_POL_LDS_BYTES;
  HIPCHK(h, hipFuncSetAttribute((const void*)gs_k_policy_mlp, hipFuncAttributeMaxDynamicSharedMemorySize, GS_POL_LDS_MAX));
  if ((rc = pol.blob.alloc(h, im.blob.size() * sizeof(double), "the policy's image"))) return rc;
  double* const image = (double*)pol.blob.p;
  HIPCHK(h, hipMemcpy(image, im.blob.data(), im.blob.size() * sizeof(double), hipMemcpyHostToDevice));
  GsPolicyArgs& a = pol.args;
  a = GsPolicyArgs{};
  a.B = h->B; a.D = h->obs_dim; a.A = h->action_dim; a.n_layers = p->n_layers; a.activation = p->activation; a.head = p->head;
  a.stochastic = p->stochastic; a.first_instance = h->EC.first_instance; a.logp_behind = gs_pol_logp_behind(h->action_dim);
  for (int l = 0; l < p->n_layers; ++l) a.L[l] = GsPolicyLayer{image + im.w_off[l], image + im.b_off[l], im.kb[l], im.nt[l]};
  pol.compute = GS_COMPUTE_F64;
  pol.set = true;
  return GS_OK;
}

}  // extern "C"

// one launch: actions[B][A] of the installed policy on obs[B][obs_dim] (device pointers), on the handle's main stream; logp: NULL or
// [B], the log-probabilities of the actions a stochastic policy samples
int gsi::launch_policy(gs_handle* h, const double* obs, double* act, uint64_t seed, int t, double* logp) {
  const dim3 grid((unsigned)((h->B + GS_POL_ROWS - 1) / GS_POL_ROWS)), block(64 * GS_POL_WAVES);
  if (h->pol.compute == GS_COMPUTE_F32) {
    GsPolicyArgsF32 a = h->pol.args32;
    a.obs = obs; a.act = act; a.seed = seed; a.t = t; a.logp = logp;
    hipLaunchKernelGGL(gs_k_policy_mlp_f32, grid, block, h->pol.lds32, h->stream, a);
  } else {
    GsPolicyArgs a = h->pol.args;
    a.obs = obs; a.act = act; a.seed = seed; a.t = t; a.logp = logp;
    hipLaunchKernelGGL(gs_k_policy_mlp, grid, block, h->pol.lds64, h->stream, a);
  }
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

extern "C" {

int gs_policy_mlp_eval(gs_handle* h, uint64_t policy_seed, int32_t t, double* actions_host) {
  if (!h || !actions_host) return fail(h, GS_E_INVALID, "handle / actions_host is NULL");
  if (!h->pol.set) return fail(h, GS_E_STATE, "gs_policy_mlp_eval before gs_policy_mlp_set");
  if (!h->was_reset) return fail(h, GS_E_STATE, "gs_policy_mlp_eval before gs_reset");
  GS_ENTER(h);
  int rc = launch_policy(h, h->d_obs2[h->obs_cur], h->pol.act, policy_seed, t);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(actions_host, h->pol.act, (size_t)h->B * h->action_dim * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

}  // extern "C"

// ---- device-resident rollout collection ---------------------------------------------------------------
// T fused env steps back to back, nothing on the host in between (algorithms/base.py:268-298, batched).
// Device layout (gs_rollout_device_view): obs_seq[T + 1][B][obs_dim] -- slot t is what step t started from, slot
// t + 1 is written by step t's kernel itself (its observation output IS the next slot: no copy) --, act[T][B][A],
// rew[T][B], done[T][B], and the side list of terminal observations (t, b, row) the in-place resets replaced.
// the constant columns of every slot: the step kernels write only the columns that change
int gsi::fill_const_columns(gs_handle* h) {
  gs_handle::Rollout& ro = h->ro;
  const long long rows = (long long)(ro.T_cap + 1) * h->B;
  const int w = h->obs_skip1 - h->obs_skip0;
  if (w > 0) {
    const long long total = rows * w;
    hipLaunchKernelGGL(gs_k_fill_const_columns, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, ro.obs_seq.p, rows,
                       h->obs_dim, h->obs_skip0, h->obs_skip1, h->map_obs, h->d_cst);
    HIPCHK(h, hipGetLastError());
  }
  ro.const_dirty = false;
  return GS_OK;
}

int gsi::rollout_ensure(gs_handle* h, int T, int min_term_cap) {
  gs_handle::Rollout& ro = h->ro;
  if (T <= ro.T_cap && min_term_cap <= ro.term_cap) return GS_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  T = std::max(T, ro.T_cap);       // (a load that only needs a longer list keeps the length the handle had)
  rollout_release(h, true);
  dataset_release(h, true);      // (its map and partial results are sized by T; installed statistics stay)
  const size_t B = h->B, D = h->obs_dim, A = std::max(h->action_dim, 1);
  // an instance finishes at most once per min(episode_length, 11) steps (truncation needs more than 10 violating steps
  // since its last reset, grid_env.py:604) plus once for an episode that was already under way; a loaded dataset (gs_rollout_load)
  // may end an episode at every transition and says how many it holds
  const int min_ep = std::max(1, std::min(h->cfg.episode_length, 11));
  const size_t cap = std::max(B * ((size_t)T / min_ep + 1), (size_t)std::max(min_term_cap, 0));
  int rc = ro.term_count.grow(h, 1, "the rollout's terminal counter");
  if (rc) return rc;
  // all or none; until gs_rollout sets ro.T again the handle holds no rollout (rollout_release)
  if ((rc = alloc_all(h, "the rollout's buffers", ro.obs_seq.want((size_t)(T + 1) * B * D), ro.act.want((size_t)T * B * A), ro.rew.want((size_t)T * B),
                      ro.done.want((size_t)T * B), ro.term_idx.want(cap * 2), ro.term_obs.want(cap * D)))) return rc;
  ro.T_cap = T; ro.term_cap = (int)std::min<size_t>(cap, 0x7fffffff);
  return fill_const_columns(h);      // once: a rollout leaves them alone
}

extern "C" {

int gs_rollout(gs_handle* h, int32_t T, int32_t policy, uint64_t policy_seed, const double* actions) {
  if (!h || T <= 0) return fail(h, GS_E_INVALID, "handle is NULL or T <= 0");
  if (policy != GS_POLICY_UPLOADED && policy != GS_POLICY_RANDOM && policy != GS_POLICY_MLP) return fail(h, GS_E_INVALID, "unknown policy %d", policy);
  if (policy == GS_POLICY_MLP && !h->pol.set) return fail(h, GS_E_STATE, "GS_POLICY_MLP before gs_policy_mlp_set");
  if (policy == GS_POLICY_UPLOADED && !actions && h->action_dim > 0) return fail(h, GS_E_INVALID, "GS_POLICY_UPLOADED needs actions[T][B][action_dim]");
  if (!h->was_reset) return fail(h, GS_E_STATE, "gs_rollout before gs_reset");
  GS_ENTER(h);
  int rc = rollout_ensure(h, T);
  if (rc) return rc;
  gs_handle::Rollout& ro = h->ro;
  if (ro.const_dirty && (rc = fill_const_columns(h))) return rc;      // (a loaded dataset's rows lay over them: gs_rollout_load)
  const size_t B = h->B, D = h->obs_dim, A = h->action_dim;
  // a stochastic policy's log-probabilities are recorded with its actions (on-policy rollouts, abi_onpolicy.hip)
  const bool stochastic = policy == GS_POLICY_MLP && (h->pol.compute == GS_COMPUTE_F32 ? h->pol.args32.stochastic : h->pol.args.stochastic);
  ro.logp_recorded = stochastic && ro.record_logp;
  if (ro.logp_recorded && (rc = ro.logp.grow(h, (size_t)ro.T_cap * B, "the rollout's log-probabilities"))) { ro.logp_recorded = false; return rc; }
  ro.T = T; ro.n_term = -1;
  HIPCHK(h, hipMemsetAsync(ro.term_count, 0, sizeof(int32_t), h->stream));
  if (A > 0) {
    if (policy == GS_POLICY_UPLOADED) {
      HIPCHK(h, hipMemcpyAsync(ro.act, actions, (size_t)T * B * A * sizeof(double), hipMemcpyHostToDevice, h->stream));
    } else if (policy == GS_POLICY_RANDOM) {
      const long long total = (long long)T * B * ((A + 3) / 4);
      hipLaunchKernelGGL(gs_k_rollout_actions, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, ro.act.p, (int)T, (int)B, (int)A,
                         policy_seed, h->EC.first_instance, 0u);
      HIPCHK(h, hipGetLastError());
    }
  }
  // slot 0 = the observation the environment stands at
  HIPCHK(h, hipMemcpyAsync(ro.obs_seq, h->d_obs2[h->obs_cur], B * D * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  // second-generation step kernels do the bookkeeping themselves (finished instances are reset at the start of the NEXT
  // step, rewards / flags written at the end of the step): one launch per step, and one small kernel after the last
  // step for the instances it finished; the other kernels are followed by that small kernel after every step
  // (The whole rollout as ONE launch -- each workgroup looping over the T steps by itself, no workgroup needs another --
  // was built in round 2 and is bit-identical, but slower: inlined into a loop the step's ~1 KB argument block stays live
  // across iterations (230 spilled registers); as an out-of-line call reading its arguments from memory the block lands in
  // scratch (59 M env-steps/s against 150 M for a launch per step).)
  // GS_POLICY_MLP: the policy of step t + 1 must see the FRESH observation of an instance that step t finished (the reference calls
  // env.reset() and then the policy, algorithms/base.py:289-290), so the bookkeeping cannot wait for the next step kernel: the small
  // kernel follows every step, as for the first-generation members, and the policy kernel reads the slot behind it
  const bool fused = h->second_gen() && policy != GS_POLICY_MLP;
  for (int t = 0; t < T; ++t) {
    double* nxt = ro.obs_seq + (size_t)(t + 1) * B * D;
    if (policy == GS_POLICY_MLP && (rc = launch_policy(h, ro.obs_seq + (size_t)t * B * D, ro.act + (size_t)t * B * A, policy_seed, t,
                                                       ro.logp_recorded ? ro.logp + (size_t)t * B : nullptr))) return rc;
    GsRolloutStep rs{ro.rew, ro.done, ro.obs_seq + (size_t)t * B * D, h->map_obs, h->d_cst, ro.term_count, ro.term_idx, ro.term_obs, ro.term_cap, h->obs_dim, t, 1};
    if ((rc = step_kernels(h, ro.act + (size_t)t * B * A, nxt, fused ? &rs : nullptr))) return rc;
    if (!fused || t == T - 1) {
      if ((rc = join_streams(h))) return rc;
      GsRolloutPostArgs pa{fused ? nullptr : ro.rew, fused ? nullptr : ro.done, nxt, h->map_obs, h->d_cst, ro.term_count, ro.term_idx, ro.term_obs, ro.term_cap, h->obs_dim, t, h->B};
      hipLaunchKernelGGL(gs_k_rollout_post, dim3(h->groups), dim3(256), 0, h->stream, h->T, h->R, h->EC, h->slab, pa);
      HIPCHK(h, hipGetLastError());
      // (the fresh rows it wrote carry the shared constants: every instance's own static load columns over them)
      if (h->pl && (rc = launch_load_columns(h, nxt))) return rc;
    }
  }
  if ((rc = join_streams(h))) return rc;
  // the environment now stands at slot T: that is its current observation for gs_download_step / gs_allgather_obs
  if (h->gather_pending[h->obs_cur]) { HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_gather[h->obs_cur], 0)); h->gather_pending[h->obs_cur] = false; }
  HIPCHK(h, hipMemcpyAsync(h->d_obs2[h->obs_cur], ro.obs_seq + (size_t)T * B * D, B * D * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  if (h->rows_stale) h->last_obs = h->d_obs2[h->obs_cur];      // (the slot may be reallocated by a longer rollout; this copy stays)
  ro.calls += 1;
  rollout_ended(h, 0, (uint32_t)T);      // (gs_rollout_continue may follow while the environment is not moved)
  return GS_OK;      // asynchronous: gs_synchronize / gs_rollout_download / gs_rollout_device_view wait for it
}

}  // extern "C"

int gsi::rollout_finish(gs_handle* h) {
  gs_handle::Rollout& ro = h->ro;
  if (ro.T <= 0) return fail(h, GS_E_STATE, "no rollout has been collected on this handle");
  GS_ENTER(h);
  if (ro.n_term < 0) {
    int32_t n = 0;
    HIPCHK(h, hipMemcpyAsync(&n, ro.term_count, sizeof n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n > ro.term_cap) return fail(h, GS_E_NOMEM, "internal: %d finished episodes exceed the terminal list (%d)", n, ro.term_cap);
    ro.n_term = n;
  }
  return GS_OK;
}

extern "C" {

int gs_rollout_device_view(gs_handle* h, gs_rollout_device* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  int rc = rollout_finish(h);
  if (rc) return rc;
  const gs_handle::Rollout& ro = h->ro;
  out->T = ro.T; out->B = h->B; out->obs_dim = h->obs_dim; out->action_dim = h->action_dim;
  out->obs_seq = ro.obs_seq; out->actions = ro.act; out->rewards = ro.rew; out->terminals = ro.done;
  out->n_terminal = ro.n_term; out->terminal_index = ro.term_idx; out->terminal_obs = ro.term_obs;
  return GS_OK;
}

int gs_rollout_download(gs_handle* h, const gs_rollout_view* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / view is NULL");
  int rc = rollout_finish(h);
  if (rc) return rc;
  const gs_handle::Rollout& ro = h->ro;
  const size_t T = ro.T, B = h->B, D = h->obs_dim, A = h->action_dim, blk = B * D;
  if (out->observations) HIPCHK(h, hipMemcpyAsync(out->observations, ro.obs_seq, T * blk * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->next_observations) HIPCHK(h, hipMemcpyAsync(out->next_observations, ro.obs_seq + blk, T * blk * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->final_observation) HIPCHK(h, hipMemcpyAsync(out->final_observation, ro.obs_seq + T * blk, blk * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->actions && A) HIPCHK(h, hipMemcpyAsync(out->actions, ro.act, T * B * A * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->rewards) HIPCHK(h, hipMemcpyAsync(out->rewards, ro.rew, T * B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->terminals) HIPCHK(h, hipMemcpyAsync(out->terminals, ro.done, T * B, hipMemcpyDeviceToHost, h->stream));
  std::vector<int32_t> idx((size_t)ro.n_term * 2);
  std::vector<double> rows(out->next_observations ? (size_t)ro.n_term * D : 0);
  if (ro.n_term && out->next_observations) {
    HIPCHK(h, hipMemcpyAsync(idx.data(), ro.term_idx, idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(rows.data(), ro.term_obs, rows.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // next_observations[t][b] of a finished transition is the terminal observation, not the fresh one in slot t + 1
  if (out->next_observations)
    for (int k = 0; k < ro.n_term; ++k)
      memcpy(out->next_observations + ((size_t)idx[2 * k] * B + idx[2 * k + 1]) * D, rows.data() + (size_t)k * D, D * sizeof(double));
  if (out->n_terminal) *out->n_terminal = ro.n_term;
  return GS_OK;
}

}  // extern "C"
