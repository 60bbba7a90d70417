// handle.h -- what the translation units of the C ABI's host side share (host only, internal): the handle and the checks object,
// error reporting, the stream join every entry point starts with, the handle's allocator, the owner of every other device buffer
// (DevBuf), the hand-over of a view to a consumer's stream (publish), launch timing, and the helpers that cross files.
// Which file owns what: DESIGN.md section 1, "File map of the ABI's host side".
//
// Whatever has external linkage here lives in namespace gsi, which is hidden: libgridstep.so exports the C ABI and nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gridstep.h"
#include "gs_internal.h"
#include "kernels.h"
#include "topology.h"
#include "plan.h"
#include "policy.h"
#include "train.h"
#include "q.h"
#include "pathwise.h"

// (also on the handle's parts that own a DevBuf and on gs_checks: their destructors are not part of the library's surface)
#define GS_HIDDEN __attribute__((visibility("hidden")))

constexpr int GS_LEARNER_COUNT = 2 + GS_COST_CHANNELS + 2;      // the policy, the reward critic, the cost critics, the twin Q networks
static_assert(GS_LEARNER_Q == 2 + GS_COST_CHANNELS, "the Q learners follow the cost critics'");

struct GsLoopComm;      // abi_comm.hip
struct gs_handle;

namespace gsi GS_HIDDEN {

typedef void* gs_ncclComm_t;
struct TimedLaunch { int kid; hipEvent_t a, b; };

// the message as the library's last error (gs_last_error; gridstep_abi.hip holds it) and, with a handle, as the handle's
int fail(gs_handle* h, int code, const char* fmt, ...);

// A hipMalloc of its own (what does NOT go through dev_alloc): the pointer WITH its capacity in elements, 0 exactly when the pointer
// is NULL.  Reads like the pointer.  Freed by release() or at scope exit; a handle's members are released by their owners
// (*_release, called by gs_destroy with the device current and the streams idle), so their destructors find nothing left.
template <typename X>
struct DevBuf {
  X* p = nullptr; size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  operator X*() const { return p; }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  // `count` elements (at least one) in place of what it held; GS_E_NOMEM naming `what` leaves it empty and HIP's last error clear
  int alloc(gs_handle* h, size_t count, const char* what) {
    release();
    count = std::max<size_t>(count, 1);
    if (hipMalloc((void**)&p, count * sizeof(X)) != hipSuccess) {
      p = nullptr; (void)hipGetLastError();
      return fail(h, GS_E_NOMEM, "%s: %zu bytes do not fit on the device", what, count * sizeof(X));
    }
    cap = count;
    return GS_OK;
  }
  int grow(gs_handle* h, size_t count, const char* what);      // nothing if it holds `count`; else waits for the handle's stream, then alloc
  struct Want { DevBuf& b; size_t count; };
  Want want(size_t count) { return Want{*this, count}; }
};
// several buffers or none: alloc_all(h, what, a.want(n), b.want(m), ...)
template <typename... W>
int alloc_all(gs_handle* h, const char* what, W... w) {
  int rc = GS_OK;
  ((rc = rc ? rc : w.b.alloc(h, w.count, what)), ...);
  if (rc) (w.b.release(), ...);
  return rc;
}

}  // namespace gsi
using gsi::DevBuf;

// A handle is its plan (plan.h: members, rows, launch shapes, host tables) and the device state built from it.
struct gs_handle : GsPlan {
  int device = 0;
  hipStream_t stream = nullptr;
  gs_config cfg{};
  HostTopology topo;
  GsTables T{};
  struct gs_checks* fused = nullptr;      // checks evaluated inside the step kernel's epilogue (gs_checks_set_fused)
  // A step of the second-generation kernels goes out as TWO launches, each half of the workgroups, on two streams
  // (GsPlan::split_ok): consecutive steps of one half need nothing from the other half, so the second stream's kernels slide
  // into the launch gaps and the uneven tails of the first's (two handles of 4096 instances on two streams: 205 M env-steps/s
  // against 186 M for one of 8192).  `forked`: stream2 holds step launches the main stream has not waited for yet; every entry
  // point other than the step itself joins first (GS_ENTER).
  bool forked = false;
  hipStream_t stream2 = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_peer = nullptr, ev_peer2 = nullptr;
  // The second-generation step kernels do not write the (|V|, angle) / (flow, |P| / rating) row pairs: those are the first
  // 2 n + 2 m columns of the observation block the step writes anyway.  `rows_stale`: the rows lag behind `last_obs`, the block
  // of the last step; every entry point that reads or partly rewrites them restores them first (ensure_rows).
  bool rows_stale = false; const double* last_obs = nullptr;
  unsigned long long* d_stamps = nullptr;
  bool was_reset = false;
  std::vector<void*> allocs;
  char* arena = nullptr; size_t arena_left = 0;      // dev_alloc: the current chunk of small tables
  double* slab = nullptr;
  double* d_in = nullptr; size_t in_doubles = 0;
  double* d_out = nullptr; size_t out_doubles = 0;
  // [B][obs_dim] x 2, owned by the environment path: both written whole at reset, the changing columns of the other one by
  // every step -- so that the all-gather of step k (on its own stream) can run while step k + 1 computes
  double* d_obs2[2] = {nullptr, nullptr}; int obs_cur = 0;
  hipStream_t comm_stream = nullptr; hipEvent_t ev_step = nullptr, ev_gather[2] = {nullptr, nullptr}; bool gather_pending[2] = {false, false};
  // host observation arrays whose constant columns are in place (gs_host_obs_bind): gs_step / gs_download_step copy only the
  // changing columns into these -- two strided copies instead of one whole block, 36 % fewer bytes over PCIe on the 123-bus feeder
  std::vector<const double*> bound_obs;
  float* d_obs32 = nullptr;                // float32 copy of the observation block (gs_step_f32 / gs_download_step_f32), on first use
  hipEvent_t ev_scalars = nullptr;
  DevBuf<double> d_actions;                // gs_upload_actions: [batches][B][max(action_dim, 1)]
  // gs_rollout: [T + 1][B][obs_dim] observation sequence, [T][B][A] actions, [T][B] rewards / done flags, and the side
  // list of terminal observations (the rows the in-place resets replaced)
  struct GS_HIDDEN Rollout {
    int T_cap = 0, T = 0, term_cap = 0; uint64_t calls = 0;
    DevBuf<double> obs_seq, act, rew, term_obs; DevBuf<uint8_t> done; DevBuf<int32_t> term_count, term_idx;
    int32_t n_term = 0;
    // logp [T][B]: the log-probabilities of the last rollout's actions (recorded: by the last rollout); abi_onpolicy.hip
    bool record_logp = true, logp_recorded = false;
    DevBuf<double> logp; hipEvent_t ev_eval = nullptr;
    // a load (abi_load.hip) overwrote whole rows of obs_seq: the next gs_rollout puts the constant columns back before it steps
    bool const_dirty = false;
    // gs_rollout_continue (abi_window.hip).  ended_on = `calls` of the last rollout that was COLLECTED here
    // (gs_rollout / gs_rollout_continue; a load advances `calls` alone), moves_at_end = env_moves when it ended: the environment
    // stands at its last slot exactly while both still match.  kept: its steps that came from the rollout before; t0_next: the draw
    // index its last step used, plus one
    uint64_t ended_on = 0, moves_at_end = 0; int kept = 0; uint32_t t0_next = 0;
  } ro;
  // gs_rollout_continue's second terminal list (term_idx [term_cap][2], term_obs [term_cap][obs_dim]: the compaction writes it and the
  // two lists change places), pos [term_cap] where each old entry went, n_old [1] the old count; made on the first shift in place,
  // released with the rollout's buffers
  struct GS_HIDDEN Window { DevBuf<int32_t> term_idx, pos, n_old; DevBuf<double> term_obs; } win;
  // gs_rollout_load (abi_load.hip): two page-locked staging buffers and their device chunks (`bytes` each, grown
  // to the largest asked for), the stream the chunks are copied on, per buffer the events "copied" and "consumed", and the verdict
  // (offending transitions, the first one's index).  Kept between loads, released with the handle.
  struct GS_HIDDEN Loader {
    char* pin[2] = {nullptr, nullptr}; DevBuf<char> dev[2]; size_t bytes = 0;
    hipStream_t copy = nullptr; hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_used[2] = {nullptr, nullptr}; bool busy[2] = {false, false};
    DevBuf<int32_t> verdict;
  } ld;
  // gs_dataset_*: the dataset over the last rollout (abi_dataset.hip).  built_on = ro.calls of the rollout the map (and, unless
  // the statistics were installed or kept, the statistics) was built on, 0 = none; stats = mean[Ct] then std[Ct] at stride Cs
  // (Ct = obs_dim + action_dim + 1, Cs = Ct rounded up to even) on the device; part = the chunks' partial results; idx / h_idx =
  // the sample indices on the device / their page-locked staging copy; batch[k] = the handle's own buffer for output k
  struct GS_HIDDEN Dataset {
    uint64_t built_on = 0; long long N = 0; bool have_stats = false;
    DevBuf<double> stats, part; DevBuf<int32_t> map;
    DevBuf<int32_t> idx; int32_t* h_idx = nullptr; hipEvent_t ev_idx = nullptr; bool idx_pending = false;      // (h_idx: idx.cap entries)
    DevBuf<char> batch[5]; hipEvent_t ev_batch = nullptr;
  } ds;
  // gs_policy_mlp_set: the policy's packed weights and biases (one allocation), the actions of gs_policy_mlp_eval [B][A], and the
  // argument block of gs_k_policy_mlp with everything but obs / act / t / seed filled in.  Not environment state.
  // compute: GS_COMPUTE_*; with GS_COMPUTE_F32 `blob` holds the float32 image and the normalisation vectors, and args32 is the
  // argument block of gs_k_policy_mlp_f32 (kernels_policy_f32.hip)
  // dims / h_norm (float32 path): the layers' widths and the host copy of shift then scale ([16 kb_0] each), for the learner
  struct GS_HIDDEN Policy { bool set = false; DevBuf<char> blob; DevBuf<double> act; GsPolicyArgs args{}; int compute = GS_COMPUTE_F64; GsPolicyArgsF32 args32{}; int lds32 = 0, lds64 = GS_POL_LDS_BYTES;
                            int32_t dims[GS_POLICY_MAX_LAYERS + 1] = {}; std::vector<double> h_norm; } pol;
  // a value network: its float32 image and normalisation vectors (one allocation), the values of gs_value_mlp_eval [B] (the reward
  // critic's only), and the argument block of gs_k_value_mlp_f32 with everything but obs / out / rows filled in
  // (dims / h_norm: as the policy's)
  struct GS_HIDDEN Value { bool set = false; DevBuf<char> blob; DevBuf<double> out; GsValueArgs args{}; int lds = 0;
                           int32_t dims[GS_POLICY_MAX_LAYERS + 1] = {}; std::vector<double> h_norm; };
  // A critic over rollouts (abi_onpolicy.hip): its network and what critic_evaluate made of the last rollout -- values [T_cap + 1][B],
  // term_values [term_cap], adv / ret [T_cap][B], made on first use (all four or none), sized by the rollout's capacity and released
  // with it; evaluated_on = ro.calls of the rollout they belong to, 0 = none.  critic[0]: the reward critic (gs_value_mlp_set,
  // gs_rollout_evaluate); critic[1 + c]: the critic of constraint channel c (gs_cost_value_mlp_set, gs_rollout_evaluate_costs)
  struct GS_HIDDEN Critic { Value net; DevBuf<double> values, term_values, adv, ret; uint64_t evaluated_on = 0; } critic[1 + GS_COST_CHANNELS];
  // gs_rollout_costs (abi_costs.hip): margins / costs [3][T][B], counts [3][T][B], n_viol [3] of the last rollout, channel c at
  // c * T * B; computed_on = ro.calls of the rollout they belong to, 0 = none.  Sized by the rollout's capacity and released with it.
  struct GS_HIDDEN Costs {
    DevBuf<double> margins, costs; DevBuf<int32_t> counts; DevBuf<unsigned long long> n_viol;
    uint64_t computed_on = 0; hipEvent_t ev = nullptr;
  } cc;
  // gs_rollout_episodes (abi_episodes.hip): the per-instance carries of the open episodes ([B]; cost / viol [3][B]; partial: B bytes
  // in whole words), the episode list of the last accounted rollout (cap entries, the rollout's term_cap; cost / viol channel c at
  // c * cap), seg [B] (counts, then offsets), n_ep [1] and the statistics.  live: a track exists (gs_episodes_clear ends it);
  // accounted_on = ro.calls of the rollout the list belongs to, 0 = none; moves_at = env_moves when that rollout was accounted.
  // The carries are made on first use (all or none) and live until the track is cleared; the list goes with the rollout's buffers.
  struct GS_HIDDEN EpisodeTrack {
    DevBuf<double> c_ret, c_cost; DevBuf<int32_t> c_len, c_ord, c_viol, c_anyv, seg, n_ep; DevBuf<uint32_t> c_partial;
    DevBuf<double> e_ret, e_cost; DevBuf<int32_t> e_idx, e_len, e_ord, e_flags, e_viol, e_anyv; DevBuf<GsEpisodeStats> stats;
    size_t cap = 0; bool live = false; int with_costs = 0;
    uint64_t accounted_on = 0, moves_at = 0; hipEvent_t ev = nullptr;
  } ep;
  // gs_onpolicy_* (abi_batches.hip): comb [T_cap][B] the combined advantage of the last prepared rollout, part the chunks' partial
  // results, stats (mean, std) of comb, norm = shift then scale at stride Ds (obs_dim rounded up to even) with h_norm its host
  // staging copy (ev_norm: read); idx / stage / adv_stats / field[k] = the handle's own buffers of a minibatch.  prepared_on = ro.calls of the rollout
  // prepare ran on, 0 = none; cfg = what it was given (the host pointers dropped), chan = bit c: cost channel c is gathered.  Made
  // on first use, released with the rollout's buffers.
  struct GS_HIDDEN OnPolicyBatches {
    uint64_t prepared_on = 0; long long N = 0; gs_onpolicy_batch_config cfg{}; bool have_norm = false; int chan = 0;
    DevBuf<double> comb, part, stats, norm, stage, adv_stats; std::vector<double> h_norm;
    DevBuf<int32_t> idx; DevBuf<char> field[2 + GS_OPB_SCALARS]; hipEvent_t ev = nullptr, ev_norm = nullptr; bool norm_pending = false;
  } opb;
  // gs_learner_* (abi_learner.hip).  learner[0]: the policy's, learner[1 + k]: critic[k]'s.  live: created and
  // the network not installed again since.  net: the kernels' description (forward image = the installed network's, T = wt);
  // params / grad / m / v [P] in torch order; steps: Adam's t.  Per-sample arrays of the last step (n_last samples; 0: none) and
  // stats / blocksum: scratch, grown to the largest n seen and released with the rollout's buffers, like tr (acts / deltas
  // [n][row_stride], partial [segments][P]), which every learner of the handle shares.  gen: advanced by every gs_learner_create (a
  // federation remembers it: abi_fed.hip).
  struct GS_HIDDEN Learner {
    bool live = false; gs_learner_config cfg{}; uint64_t steps = 0, gen = 0; GsTrainNet net{}; int A = 0;
    gs_learner_loss loss{};      // gs_learner_set_loss; GS_LOSS_DEFAULT from gs_learner_create and after learner_drop
    DevBuf<float> params, grad, m, v, wt;
    DevBuf<double> lp_new, ratio, term0, term1, stats, blocksum; DevBuf<int32_t> clipped; int n_last = 0;
    hipEvent_t ev = nullptr;
    int signal = GS_SIGNAL_BATCH;      // gs_learner_set_signal; reset like `loss`
    // parameter anchors (abi_anchor.hip), all made on first use by the gs_learner_anchor_* / gs_learner_fisher_*
    // entries and gone with the learner (learner_drop): prox [P] the PROX centre (have_prox), importance / centre [P] the EWC slot
    // (tasks commits merged), pending [P] the open or last task's Fisher sum over `samples` samples (open: between begin and commit),
    // sums [3][red blocks] what gs_k_train_anchor leaves for gs_learner_anchor_stats.  mu / lambda: the coefficients the next step
    // reads; stepped: a step ran with one of them non-zero, under step_mu / step_lambda.
    struct GS_HIDDEN Anchor {
      DevBuf<float> prox, importance, centre; DevBuf<double> pending, sums;
      bool have_prox = false, open = false, stepped = false;
      double mu = 0.0, lambda = 0.0, step_mu = 0.0, step_lambda = 0.0;
      int64_t tasks = 0, samples = 0;
      void drop_prox() { prox.release(); have_prox = false; mu = 0.0; }
      void drop_ewc() { importance.release(); centre.release(); pending.release(); open = false; tasks = 0; samples = 0; lambda = 0.0; }
      void release() { drop_prox(); drop_ewc(); sums.release(); stepped = false; step_mu = step_lambda = 0.0; }
    } an;
  } learner[GS_LEARNER_COUNT];
  // (qsa [n][obs_dim + A], qy [n]: the Q learner's input rows and targets, and the Q-based signals; abi_learner.hip)
  struct GS_HIDDEN TrainScratch { DevBuf<float> acts, deltas, partial, qsa, qy; } tr;
  // gs_q_* (abi_q.hip).  qnet[which]: a twin -- the network (blob = the ONLINE image and the normalisation; args
  // unused but for L, n_layers and activation), its target image (image_floats floats, laid out as the online one: TL points into
  // it) and the argument block of gs_k_q_mlp_f32 on the online image.  learner[GS_LEARNER_Q + which] trains it.
  struct GS_HIDDEN QNet { Value net; DevBuf<float> target; size_t image_floats = 0; GsPolicyLayerF32 TL[GS_POLICY_MAX_LAYERS] = {}; GsQArgs qargs{}; } qnet[2];
  // what gs_rollout_evaluate_q made of the last rollout: q [src][which][T_cap][B], q_min [src][T_cap][B], q_adv, td [T_cap][B]; made
  // on first use (all or none), released with the rollout's buffers; evaluated_on = ro.calls of the rollout they belong to, 0 = none
  struct GS_HIDDEN QTrack { DevBuf<double> q, q_min, q_adv, td; uint64_t evaluated_on = 0; hipEvent_t ev = nullptr; } qt;
  // gs_rollout_evaluate_q_next (abi_q_next.hip): pre [T_cap][B][2 A], act / eps [T_cap][B][A], lp / q_min / td [T_cap][B],
  // q [which][T_cap][B] and the same over the terminal list (term_cap entries; t_q [which][term_cap]); made on first use (all or none),
  // released with the rollout's buffers; evaluated_on as QTrack's; with_terms: the last evaluation wrote the terminal arrays.
  // target_source: gs_q_set_target_source, host state that outlives rollouts and networks
  struct GS_HIDDEN QNext {
    DevBuf<float> pre, t_pre; DevBuf<double> act, eps, lp, q, q_min, td, t_act, t_eps, t_lp, t_q, t_q_min, t_value;
    uint64_t evaluated_on = 0; bool with_terms = false; hipEvent_t ev = nullptr; int target_source = GS_Q_TARGET_VALUE;
    int mask = 0;      // the bootstrap_mask of the last evaluation (gs_learner_refresh's GS_REFRESH_TD_POLICY asks for the same)
  } qn;
  // gs_learner_refresh (abi_refresh.hip).  map [T_cap][B]: transition -> terminal entry of the rollout map_on (=
  // ro.calls, 0 = none), made on the first refresh of a rollout.  The rest is scratch for n batch rows, grown to the largest n seen:
  // tb [n][2] the rows' (t, b), ie / t_tb [n][2] the compacted terminal rows' (i, e) and their entries' (t, b), pos [n], count [1]; own / next / tobs
  // [n][D] and act [n][A] the gathered rows; pre / t_pre [n][2 A], nact / neps / t_nact / t_neps [n][A], nlp / t_nlp [n] what the policy
  // leaves; q / t_q [2][n] the twins'; v / t_v [n] the value network's.  All of it is released with the rollout's buffers.
  struct GS_HIDDEN Refresh {
    uint64_t map_on = 0; size_t n_cap = 0; hipEvent_t ev = nullptr;
    DevBuf<int32_t> map, tb, ie, t_tb, pos, count;
    DevBuf<double> own, next, tobs, act, nact, neps, nlp, t_nact, t_neps, t_nlp, q, t_q, v, t_v; DevBuf<float> pre, t_pre;
  } rfr;
  // gs_learner_step_pathwise (abi_learner.hip): the twins' passes of an actor step have scratch of their own (acts /
  // deltas [n][the wider twin's row_stride], qsa [n][obs_dim + A]: the policy's saved activations in tr survive them), and the step's
  // per-sample arrays (n_last samples; 0: none): actions / noise [n][A], logp / qmin / bc / terms [n], q [2][n], which [n], dqda
  // [2][n][A]; installed: bit w = twin w took part.  Grown to the largest n seen and released with the rollout's buffers, like tr.
  struct GS_HIDDEN Pathwise {
    DevBuf<float> acts, deltas, qsa, dqda; DevBuf<double> actions, noise, logp, q, qmin, bc, terms; DevBuf<int32_t> which; int n_last = 0, installed = 0;
  } pw;
  // gs_learner_step_conservative (abi_learner.hip): the last conservative critic step's arrays (n_last minibatch
  // rows; 0: none), of twin `net`: random [n][A], the policy block's actions / noise [n][A] and logp [n], y [n] (the targets: tr.qy is
  // the next plain step's), q / weights [3 n], terms [n], scalars [4] m, S, lse, qbar.  pre_off: where the policy's saved
  // activations begin in tr.acts, behind the twin's 3 n rows, so that the view's pre-head values outlive the twin's passes.  Made on
  // first use, grown to the largest n seen and released with the rollout's buffers, like tr.
  struct GS_HIDDEN Conservative {
    DevBuf<double> random, actions, noise, logp, q, weights, terms, scalars; DevBuf<float> y; int n_last = 0, net = 0; size_t pre_off = 0;
  } cq;
  // gs_fed_* (abi_fed.hip): the federations this handle is a client of; gs_destroy detaches them (fed_detach)
  std::vector<gs_fed*> feds;
  // entries that move the environment outside gs_rollout (gs_reset, gs_set_state, gs_step*, gs_upload_injections, gs_solve*) count
  // themselves here: gs_rollout_episodes(GS_EPISODES_CONTINUE) refuses to carry an episode across one
  uint64_t env_moves = 0;
  double* d_cst = nullptr;
  int32_t *map_obs = nullptr, *map_vm = nullptr, *map_va = nullptr, *map_flow = nullptr, *map_load = nullptr,
          *map_p = nullptr, *map_q = nullptr, *map_act = nullptr, *map_state = nullptr;
  int32_t *rows_f = nullptr, *rows_i = nullptr, *rows_u = nullptr;
  double* sc_f = nullptr; int32_t* sc_i = nullptr; uint8_t* sc_u = nullptr;
  uint64_t* d_seeds = nullptr; uint8_t* d_mask = nullptr;
  // gs_fallback_linear: line reactances, dict-order bus lists and staging, created on first use
  std::vector<double> line_x;
  bool fb_ready = false; GsFallbackArgs FB{};
  // per-instance line impedances (GsPlan::pz): what the handle holds ([B][m], host copy and device copy, the fallback reads the
  // device one), the nominal values they are checked against, the arguments of gs_k_line_params (LP.pz: the step kernels' entries)
  std::vector<double> inst_r, inst_x, nominal_r, nominal_x;
  GsLineParamArgs LP{}; uint8_t* d_pzmask = nullptr;
  // per-instance load powers (GsPlan::pl): what the handle holds ([B][n_loads], host copy and device copy) and the arguments of
  // gs_k_load_params (LL.pl: the step kernels' entries)
  std::vector<double> inst_load;
  GsLoadParamArgs LL{}; uint8_t* d_plmask = nullptr;
  double *fb_load = nullptr, *fb_gen = nullptr, *fb_tl = nullptr, *fb_tg = nullptr; uint8_t* fb_mask = nullptr; int32_t* fb_applied = nullptr;
  // host copies of the per-instance scalars: ONE page-locked block the device addresses -- gs_k_scalars stores into it itself (three
  // copies through the runtime's staging buffer cost 80 us of a 0.9 ms env.step()); hd_*: the same block as the device sees it
  void* h_pin = nullptr;
  double* h_f = nullptr; int32_t* h_i = nullptr; uint8_t* h_u = nullptr; uint32_t* h_v4 = nullptr;
  double* hd_f = nullptr; int32_t* hd_i = nullptr; uint8_t* hd_u = nullptr; uint32_t* hd_v4 = nullptr;
  // timing
  bool timing = false;
  bool timing_span = false, span_open = false; hipEvent_t span_a = nullptr, span_b = nullptr; int span_kid = 0; int64_t span_launches[8] = {0};
  std::vector<gsi::TimedLaunch> timed; size_t timed_used = 0;
  // comm
  gsi::gs_ncclComm_t comm = nullptr; int rank = 0, world = 1; double* d_obs_full = nullptr;
  double *d_gather_send = nullptr, *d_gather_recv = nullptr;     // compact observation blocks (changing columns only): [B][nd], [world * B][nd]
  struct GsLoopComm* loop = nullptr;                              // the in-process transport (gs_comm_init_loopback) instead of RCCL
  hipEvent_t ev_full = nullptr;                                   // gs_allgather_obs_view: the gathered block is complete
  mutable std::string err;
};

// ---- post-step checks -------------------------------------------------------------------------------
struct GS_HIDDEN gs_checks {
  gs_handle* h = nullptr;
  GsChecksCfg C{};
  DevBuf<double> prev, out_f, freq; DevBuf<int32_t> state, out_i; DevBuf<uint8_t> bus_mask, line_mask;      // (go with `delete`: gs_checks_destroy)
  bool use_freq = false, want_masks = true;
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; size_t ev_used = 0;
};

namespace gsi GS_HIDDEN {

// A peer's stream as it crosses the C ABI: NULL = none; hipStreamLegacy (1) = the legacy default stream, i.e. handle 0
static inline hipStream_t peer_stream(void* s) { return s == (void*)hipStreamLegacy ? (hipStream_t)nullptr : (hipStream_t)s; }

#define HIPCHK(h, expr)                                                                           \
  do { hipError_t e_ = (expr);                                                                    \
       if (e_ != hipSuccess) return fail((h), GS_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

// Work of the second step stream joins the main stream (see gs_handle::forked)
static inline int join_streams(gs_handle* h) {
  if (!h->forked) return GS_OK;
  HIPCHK(h, hipEventRecord(h->ev_join, h->stream2));
  HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
  h->forked = false;
  return GS_OK;
}
#define GS_ENTER(h)                                                                               \
  do { HIPCHK((h), hipSetDevice((h)->device));                                                    \
       if ((h)->forked) { int rc_ = join_streams(h); if (rc_) return rc_; } } while (0)

constexpr size_t GS_ARENA_SMALL = 64 * 1024, GS_ARENA_CHUNK = 2 * 1024 * 1024;
template <typename X>
int dev_alloc(gs_handle* h, X** p, size_t count) {
  void* q = nullptr;
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(X);
  // Tables (a few hundred bytes to a few KB each, forty of them) share 2 MB chunks: as allocations of their own each sat on a
  // page of its own, and a workgroup's first touch of every one of them was an address-translation miss at kernel start.
  if (bytes <= GS_ARENA_SMALL && !GS_EXPERIMENT_ENV("GS_NO_TABLE_ARENA")) {
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (h->arena_left < need) {
      hipError_t e = hipMalloc(&q, GS_ARENA_CHUNK);
      if (e != hipSuccess) return fail(h, GS_E_NOMEM, "hipMalloc(%zu) failed: %s", (size_t)GS_ARENA_CHUNK, hipGetErrorString(e));
      h->allocs.push_back(q);
      h->arena = (char*)q; h->arena_left = GS_ARENA_CHUNK;
    }
    *p = (X*)h->arena;
    h->arena += need; h->arena_left -= need;
    return GS_OK;
  }
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) return fail(h, GS_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  h->allocs.push_back(q);
  *p = (X*)q;
  return GS_OK;
}

template <typename X>
int dev_upload(gs_handle* h, const X** p, const std::vector<X>& v) {
  X* q = nullptr;
  int rc = dev_alloc(h, &q, v.size());
  if (rc) return rc;
  if (!v.empty()) HIPCHK(h, hipMemcpy(q, v.data(), v.size() * sizeof(X), hipMemcpyHostToDevice));
  *p = q;
  return GS_OK;
}

inline int upload_map(gs_handle* h, int32_t** p, const std::vector<int32_t>& v) {
  const int32_t* q = nullptr;
  int rc = dev_upload(h, &q, v);
  *p = const_cast<int32_t*>(q);
  return rc;
}

// What did NOT go through dev_alloc (whose allocations live as long as the handle and go with it) is a hipMalloc of its own: a
// DevBuf, or (the communicator's buffers, abi_comm.hip) a plain pointer freed with this, which leaves it NULL
template <typename X>
void dev_free(X*& p) {
  if (p) { (void)hipFree(p); p = nullptr; }
}

template <typename X>
int DevBuf<X>::grow(gs_handle* h, size_t count, const char* what) {
  if (p && count <= cap) return GS_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));      // (what is queued may still read the old allocation)
  return alloc(h, count, what);
}

// Hands what `producer` has queued so far to a consumer: with a consumer's stream that stream waits, on the device, for an event
// recorded now (`ev`: created on first use, destroyed by its owner); without one the host waits
static inline int publish(gs_handle* h, hipStream_t producer, hipEvent_t& ev, void* consumer_stream) {
  if (!consumer_stream) { HIPCHK(h, hipStreamSynchronize(producer)); return GS_OK; }
  if (!ev) HIPCHK(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIPCHK(h, hipEventRecord(ev, producer));
  HIPCHK(h, hipStreamWaitEvent(peer_stream(consumer_stream), ev, 0));
  return GS_OK;
}

// ---- timing wrapper -------------------------------------------------------------------------
struct LaunchTimer {
  gs_handle* h; TimedLaunch* t = nullptr;
  LaunchTimer(gs_handle* hh, int kid) : h(hh) {
    if (h->timing_span) {          // one event pair around the whole timed region: no marker packets between the launches
      if (!h->span_open) {
        if (!h->span_a && (hipEventCreate(&h->span_a) != hipSuccess || hipEventCreate(&h->span_b) != hipSuccess)) return;
        (void)hipEventRecord(h->span_a, h->stream);
        h->span_open = true; h->span_kid = kid;
        for (int k = 0; k < GS_K_COUNT; ++k) h->span_launches[k] = 0;
      }
      if (kid >= 0 && kid < GS_K_COUNT) h->span_launches[kid] += 1;
      return;
    }
    if (!h->timing) return;
    if (h->timed_used == h->timed.size()) {
      TimedLaunch n; n.kid = kid;
      if (hipEventCreate(&n.a) != hipSuccess || hipEventCreate(&n.b) != hipSuccess) return;
      h->timed.push_back(n);
    }
    t = &h->timed[h->timed_used++];
    t->kid = kid;
    (void)hipEventRecord(t->a, h->stream);
  }
  ~LaunchTimer() { if (t) (void)hipEventRecord(t->b, h->stream); }
};

// ---- helpers of gridstep_abi.hip that the other files call (described where they are defined) ----
int launch_load_columns(gs_handle* h, double* dst);
int ensure_rows(gs_handle* h);
int pack_to_host(gs_handle* h, const int32_t* map, int C, double* host);
int unpack_from_host(gs_handle* h, const int32_t* map, int C, const double* host);
int step_kernels(gs_handle* h, const double* d_actions, double* obs_out = nullptr, const GsRolloutStep* rs = nullptr);

// ---- owners of what gs_destroy does not free itself (abi_rollout.hip) ----
void policy_release(gs_handle* h);
// the float32 image of an MLP as one allocation (image, then shift and scale) in `blob`; *image / *norm: where the two parts lie
int upload_image_f32(gs_handle* h, DevBuf<char>& blob, const GsPolicyImageF32& im, const float** image, const double** norm);
void rollout_release(gs_handle* h, bool keep_term_count = false);
// what is sized by the rollout's capacity but is not the rollout: every track over it, and the scratch that goes with it
void rollout_tracks_release(gs_handle* h, bool keep_carries = false);
// the constant columns of every slot of ro.obs_seq (queued); the installed policy on obs[B][obs_dim] -> act[B][A] with draw index t
int fill_const_columns(gs_handle* h);
int launch_policy(gs_handle* h, const double* obs, double* act, uint64_t seed, int t, double* logp = nullptr);
// a collected rollout has ended (its `calls` counted): the environment stands at its last slot until it is moved
static inline void rollout_ended(gs_handle* h, int kept, uint32_t t0_next) {
  h->ro.ended_on = h->ro.calls; h->ro.moves_at_end = h->env_moves; h->ro.kept = kept; h->ro.t0_next = t0_next;
}
// ---- owner of the window's second terminal list (abi_window.hip) ----
void window_release(gs_handle* h);
// buffers for a rollout of T steps whose terminal list holds at least min_term_cap entries (gs_rollout's own bound if that is more);
// a handle that has them keeps them, otherwise everything sized by T_cap or term_cap goes (rollout_release) and is made again
int rollout_ensure(gs_handle* h, int T, int min_term_cap = 0);
// ---- owner of the loader's staging (abi_load.hip) ----
void load_release(gs_handle* h);
int rollout_finish(gs_handle* h);      // waits for the last rollout's number of finished episodes (ro.n_term); GS_E_STATE without one

// ---- owner of the value networks and of the critics' arrays over the rollout (abi_onpolicy.hip) ----
void value_release(gs_handle* h);
void onpolicy_release(gs_handle* h);
// installs `p` (checked by the caller; NULL removes) as `val`; want_out: with the [B] block of gs_value_mlp_eval
int value_install(gs_handle* h, gs_handle::Value& val, const gs_policy_mlp* p, const gs_policy_mlp_opts* o, bool want_out);
// what gs_gae_config and gs_cost_gae_config (per channel) must satisfy; signal: "reward" / "cost", for the message
int gae_check(gs_handle* h, int bootstrap_mask, double gamma, double lambda, double shift, double scale, const char* signal);
// values, terminal values, advantages and returns of `c` over the last rollout, from signal[T][B] (device); queued, not stamped
int critic_evaluate(gs_handle* h, gs_handle::Critic& c, const double* signal, int bootstrap_mask, double gamma, double lambda, double shift, double scale);
// critic_evaluate has run for `c` on the rollout the handle holds
static inline bool critic_current(const gs_handle* h, const gs_handle::Critic& c) { return c.evaluated_on && c.evaluated_on == h->ro.calls; }
// queues the copies of c's arrays over the last rollout to these host pointers (NULL: not wanted)
int critic_download(gs_handle* h, const gs_handle::Critic& c, double* values, double* term_values, double* adv, double* ret);

// ---- what the scalar-output networks share on the host (scalar_net.hip): gs_k_value_mlp_f32 (value_install) and gs_k_q_mlp_f32 (gs_q_mlp_set),
// and the one launch of every kernel that runs a network over rows ----
// a packed network and where its parts lie on the device
struct ScalarNet { GsPolicyImageF32 im; const float* image = nullptr; const double* norm = nullptr; };
// packs `p` with `o` (both checked by the caller), sizes the LDS of `kernel` and uploads the image into val.blob; also val.lds,
// val.dims and val.h_norm.  val.args and val.set are the caller's.
int scalar_net_install(gs_handle* h, gs_handle::Value& val, const void* kernel, const gs_policy_mlp& p, const gs_policy_mlp_opts& o, ScalarNet& net);
// the fields GsValueArgs and GsQArgs have in common
template <typename Args>
static inline void scalar_net_args(Args& a, const gs_policy_mlp& p, const ScalarNet& net) {
  const GsPolicyImageF32& im = net.im;
  a.shift = net.norm; a.scale = net.norm + 16 * im.kb[0];
  a.n_layers = p.n_layers; a.activation = p.activation;
  a.panel_kb = gs_val_panel_kb(im.kb[0]); a.obs_stride = gs_val_obs_stride(im.kb[0]);
  for (int l = 0; l < p.n_layers; ++l) a.L[l] = GsPolicyLayerF32{net.image + im.w_off[l], net.image + im.b_off[l], im.kb[l], im.nt[l]};
}
// the workgroups of a launch of GS_VAL_ROWS rows each over `rows` > 0 rows; refuses a count the kernels' 32-bit row index cannot
// hold (`kernel`: "value" / "Q", for the message)
int scalar_net_grid(gs_handle* h, long long rows, const char* kernel, unsigned* blocks);
// The launches below are queued on the handle's main stream over `rows` rows (device pointers); rows_dev: NULL, or the device word
// holding how many of them are there.
// the value network `val` on obs; rows <= 0: nothing; scatter_*: GsValueArgs
int launch_value_rows(gs_handle* h, const gs_handle::Value& val, const double* obs, double* out, long long rows, const int32_t* rows_dev = nullptr,
                      const int32_t* scatter_idx = nullptr, double* scatter_out = nullptr, int scatter_T = 0);
// twin `Q` under the layer table `L` (its online image Q.qargs.L or its target image Q.TL) on (obs, act)
int launch_q_rows(gs_handle* h, const gs_handle::QNet& Q, const GsPolicyLayerF32* L, const double* obs, const double* act, long long rows, const int32_t* rows_dev,
                  double* out);
// the installed policy (policy_rows_ready) on obs with noise indices idx[row] = (t, b), NULL: the row; `noise`: the caller's config
struct PolicyNoise { int32_t stochastic; uint32_t draw; uint64_t seed; };
int launch_policy_rows(gs_handle* h, const PolicyNoise& noise, const double* obs, long long rows, const int32_t* rows_dev, const int32_t* idx, uint32_t tag,
                       float* pre, double* act, double* eps, double* lp);
// the most dynamic LDS for gs_k_policy_rows_f32 and gs_k_q_mlp_rows_f32, which no install sizes: before an entry's first launch of them
int rows_kernels_lds_cap(gs_handle* h);
// gs_k_policy_rows_f32 can run: a float32 tanh-Gaussian policy is installed
static inline bool policy_rows_ready(const gs_handle* h) { return h->pol.set && h->pol.compute == GS_COMPUTE_F32 && h->pol.args32.head == GS_HEAD_GAUSSIAN_TANH; }

// ---- owner of the rollout's constraint arrays (abi_costs.hip) ----
void costs_release(gs_handle* h);

// ---- owner of the episode track (abi_episodes.hip); keep_carries: only the list, which is sized by the rollout's capacity, goes ----
void episodes_release(gs_handle* h, bool keep_carries = false);

// ---- owner of the on-policy minibatch buffers (abi_batches.hip) ----
void batches_release(gs_handle* h);

// ---- owner of the learners (abi_learner.hip).  learner_drop: learner `k` (0 the policy's, 1 + c critic c's, GS_LEARNER_Q + w twin w's) ends, its parameters go
// (every *_set* entry calls it for its network); learner_scratch_release: what is sized by n; learner_release: everything ----
void learner_drop(gs_handle* h, int k);
void learner_scratch_release(gs_handle* h);
void learner_release(gs_handle* h);
// the table of the learners' networks: learner `net` by name, for a message, and the installed network it trains -- its layers,
// widths, activation, host normalisation (shift then scale, [16 kb_0] each) and image; false: not installed (the policy: not with
// GS_COMPUTE_F32)
const char* net_name(int net);
struct Installed { const GsPolicyLayerF32* L; const int32_t* dims; int n_layers, activation; const std::vector<double>* norm; const DevBuf<char>* blob; };
bool installed(const gs_handle* h, int net, Installed& I);

// the argument block of gs_k_train_grad / gs_k_train_grad_sq over h->tr's passes on the input rows `obs` [n][D]; returns the launch's
// workgroups along x (its y: gs_tr_segments(n))
int train_grad_args(gs_handle* h, const GsTrainNet& N, const float* obs, int n, int D, GsTrainGradArgs& G);
// gs_learner_step from its checks through the backward-data pass, shared with gs_learner_fisher_accumulate: the gather (where the net
// has one), the forward pass, the head of the learner's loss and the backward-data pass on `batch`, h->tr holding the passes.  `who`
// names the entry in the messages; `extra` (NULL: none) is a check of the caller's, run behind the step's own and before any launch.
// ps: the input rows [n][Din] the weight gradient reads, and the loss (GS_LOSS_*) the head ran
struct LearnerPass { const float* rows; int Din, loss; };
int learner_backprop(gs_handle* h, const char* who, int32_t net, const gs_onpolicy_batch_out* batch, int32_t n, int (*extra)(gs_handle*, int32_t),
                     LearnerPass& ps);

// ---- the terms on the parameters (abi_anchor.hip): gs_k_train_anchor on Ln's reduced gradient under Ln.an's
// coefficients, queued on the handle's stream behind gs_k_train_reduce (queue_grad_reduce of abi_learner.hip) ----
int anchor_queue(gs_handle* h, gs_handle::Learner& Ln);

// ---- owner of the Q networks, their targets and their arrays over the rollout (abi_q.hip) ----
void q_release(gs_handle* h);              // everything
void q_rollout_release(gs_handle* h);      // what is sized by the rollout's capacity
static inline bool q_current(const gs_handle* h) { return h->qt.evaluated_on && h->qt.evaluated_on == h->ro.calls; }

// ---- owner of the policy-action targets over the rollout (abi_q_next.hip) ----
void q_next_rollout_release(gs_handle* h);
static inline bool q_next_current(const gs_handle* h) { return h->qn.evaluated_on && h->qn.evaluated_on == h->ro.calls; }

// ---- owner of the per-minibatch refresh's map and scratch (abi_refresh.hip) ----
void refresh_release(gs_handle* h);

// ---- the federations of a handle that is being destroyed lose it (abi_fed.hip) ----
void fed_detach(gs_handle* h);

// ---- owner of the dataset's buffers (abi_dataset.hip); keep_stats: only what depends on the rollout's length goes ----
void dataset_release(gs_handle* h, bool keep_stats = false);
// map[0 .. N) = -1, then entry k of the last rollout's terminal list (t, b) -> map[t B + b] = k; queued on the handle's stream
int terminal_map_fill(gs_handle* h, int32_t* map, long long N);

}  // namespace gsi
