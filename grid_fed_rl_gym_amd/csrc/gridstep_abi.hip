// gridstep_abi.hip -- host side of the C ABI declared in include/gridstep.h.
//
// Owns: the compiled topology tables, one slab of per-instance rows in HBM
// (slab[group][row][64 lanes]), staging buffers for the batch-major <-> batch-innermost layout
// change, one HIP stream, optional HIP-event timing of every launch, and (lazily, via dlopen)
// an RCCL communicator for the observation all-gather.  No CPU arithmetic on the data path:
// every entry point either moves bytes or launches kernels.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gridstep.h"
#include "gs_internal.h"
#include "kernels.h"
#include "topology.h"
#include "mesh_schedule.h"
#include "plan.h"
#include "policy.h"

namespace {

thread_local std::string g_last_error;

// ---- RCCL entry points resolved at run time -------------------------------------------------
typedef struct { char internal[128]; } gs_ncclUniqueId;
typedef void* gs_ncclComm_t;
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(gs_ncclUniqueId*) = nullptr;
  int (*CommInitRank)(gs_ncclComm_t*, int, gs_ncclUniqueId, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, gs_ncclComm_t, hipStream_t) = nullptr;
  int (*CommDestroy)(gs_ncclComm_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*CommCount)(gs_ncclComm_t, int*) = nullptr;
  int (*CommUserRank)(gs_ncclComm_t, int*) = nullptr;
  int (*CommCuDevice)(gs_ncclComm_t, int*) = nullptr;
  int (*GetVersion)(int*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;

bool load_rccl(std::string& why) {
  if (g_rccl.lib) return true;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* lib = nullptr;
  for (const char* nm : names) { lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
  if (!lib) { why = std::string("cannot dlopen librccl: ") + dlerror(); return false; }
  RcclApi a; a.lib = lib;
  a.GetUniqueId = (int (*)(gs_ncclUniqueId*))dlsym(lib, "ncclGetUniqueId");
  a.CommInitRank = (int (*)(gs_ncclComm_t*, int, gs_ncclUniqueId, int))dlsym(lib, "ncclCommInitRank");
  a.AllGather = (int (*)(const void*, void*, size_t, int, gs_ncclComm_t, hipStream_t))dlsym(lib, "ncclAllGather");
  a.CommDestroy = (int (*)(gs_ncclComm_t))dlsym(lib, "ncclCommDestroy");
  a.GroupStart = (int (*)())dlsym(lib, "ncclGroupStart");
  a.GroupEnd = (int (*)())dlsym(lib, "ncclGroupEnd");
  a.CommCount = (int (*)(gs_ncclComm_t, int*))dlsym(lib, "ncclCommCount");
  a.CommUserRank = (int (*)(gs_ncclComm_t, int*))dlsym(lib, "ncclCommUserRank");
  a.CommCuDevice = (int (*)(gs_ncclComm_t, int*))dlsym(lib, "ncclCommCuDevice");
  a.GetVersion = (int (*)(int*))dlsym(lib, "ncclGetVersion");
  a.GetErrorString = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
  if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.CommDestroy) { why = "librccl lacks a required symbol"; return false; }
  g_rccl = a;
  return true;
}

struct TimedLaunch { int kid; hipEvent_t a, b; };
constexpr size_t GS_CHECKS_MAX_EVENTS = 4096;

}  // namespace

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
  double* d_actions = nullptr; int n_action_batches = 0;
  // gs_rollout: [T + 1][B][obs_dim] observation sequence, [T][B][A] actions, [T][B] rewards / done flags, and the side
  // list of terminal observations (the rows the in-place resets replaced)
  struct Rollout {
    int T_cap = 0, T = 0, term_cap = 0; uint64_t calls = 0;
    double* obs_seq = nullptr; double* act = nullptr; double* rew = nullptr; uint8_t* done = nullptr;
    int32_t* term_count = nullptr; int32_t* term_idx = nullptr; double* term_obs = nullptr;
    int32_t n_term = 0;
  } ro;
  // gs_policy_mlp_set: the policy's packed weights and biases (one allocation), the actions of gs_policy_mlp_eval [B][A], and the
  // argument block of gs_k_policy_mlp with everything but obs / act / t / seed filled in.  Not environment state.
  // compute: GS_COMPUTE_*; with GS_COMPUTE_F32 `blob` holds the float32 image and the normalisation vectors, and args32 is the
  // argument block of gs_k_policy_mlp_f32 (kernels_policy_f32.hip)
  struct Policy { bool set = false; double* blob = nullptr; double* act = nullptr; GsPolicyArgs args{}; int compute = GS_COMPUTE_F64; GsPolicyArgsF32 args32{}; int lds32 = 0; } pol;
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
  std::vector<TimedLaunch> timed; size_t timed_used = 0;
  // comm
  gs_ncclComm_t comm = nullptr; int rank = 0, world = 1; double* d_obs_full = nullptr;
  double *d_gather_send = nullptr, *d_gather_recv = nullptr;     // compact observation blocks (changing columns only): [B][nd], [world * B][nd]
  struct GsLoopComm* loop = nullptr;                              // the in-process transport (gs_comm_init_loopback) instead of RCCL
  hipEvent_t ev_full = nullptr;                                   // gs_allgather_obs_view: the gathered block is complete
  mutable std::string err;
};

namespace {

int fail(gs_handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_last_error = buf;
  if (h) h->err = buf;
  return code;
}

// A peer's stream as it crosses the C ABI: NULL = none; hipStreamLegacy (1) = the legacy default stream, i.e. handle 0
static inline hipStream_t peer_stream(void* s) { return s == (void*)hipStreamLegacy ? (hipStream_t)nullptr : (hipStream_t)s; }

#define HIPCHK(h, expr)                                                                           \
  do { hipError_t e_ = (expr);                                                                    \
       if (e_ != hipSuccess) return fail((h), GS_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

// Work of the second step stream joins the main stream (see gs_handle::forked)
static int join_streams(gs_handle* h) {
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

int upload_map(gs_handle* h, int32_t** p, const std::vector<int32_t>& v) {
  const int32_t* q = nullptr;
  int rc = dev_upload(h, &q, v);
  *p = const_cast<int32_t*>(q);
  return rc;
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

// ---- layout movers --------------------------------------------------------------------------
int launch_pack(gs_handle* h, const int32_t* map, int C, double* dst) {
  if (C <= 0) return GS_OK;
  LaunchTimer lt(h, GS_K_PACK);
  dim3 grid(h->groups, (C + 63) / 64);
  hipLaunchKernelGGL(gs_k_pack, grid, dim3(256), 0, h->stream, map, h->d_cst, C, h->R.total, h->slab, dst, h->B);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

// each instance's own static load columns of a per-instance-loads handle (GsPlan::pl) into the observation block dst [B][obs_dim]
int launch_load_columns(gs_handle* h, double* dst) {
  const size_t threads = (size_t)h->B * 2 * h->n_loads;
  hipLaunchKernelGGL(gs_k_load_columns, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->LL.pl, dst, h->B, h->obs_dim,
                     2 * h->n + 2 * h->m + 1, h->n_loads);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}
// A whole observation block [B][obs_dim] from the rows: every column, the constants included -- on a per-instance-loads handle
// the static load columns of each instance are its own, written over the shared constants
int launch_pack_obs(gs_handle* h, double* dst) {
  const int rc = launch_pack(h, h->map_obs, h->obs_dim, dst);
  return rc || !h->pl ? rc : launch_load_columns(h, dst);
}

int launch_unpack(gs_handle* h, const int32_t* map, int C, const double* src, int stride = 0) {
  if (C <= 0) return GS_OK;
  LaunchTimer lt(h, GS_K_UNPACK);
  dim3 grid(h->groups, (C + 63) / 64);
  hipLaunchKernelGGL(gs_k_unpack, grid, dim3(256), 0, h->stream, map, C, h->R.total, h->slab, src, h->B, stride ? stride : C);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

// The result rows a lean step left behind (gs_handle::lean), copied back from the observation block it wrote: exact (the
// block's first 2 n + 2 m columns ARE those rows' values).  Called, after GS_ENTER, by whatever reads or partly rewrites them.
int ensure_rows(gs_handle* h) {
  if (!h->rows_stale) return GS_OK;
  h->rows_stale = false;
  return launch_unpack(h, h->map_obs, 2 * h->n + 2 * h->m, h->last_obs, h->obs_dim);
}

int pack_to_host(gs_handle* h, const int32_t* map, int C, double* host) {
  if (!host || C <= 0) return GS_OK;
  int rc = launch_pack(h, map, C, h->d_out);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(host, h->d_out, (size_t)h->B * C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

int unpack_from_host(gs_handle* h, const int32_t* map, int C, const double* host) {
  if (C <= 0) return GS_OK;
  HIPCHK(h, hipMemcpyAsync(h->d_in, host, (size_t)h->B * C * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return launch_unpack(h, map, C, h->d_in);
}

int fetch_scalars(gs_handle* h, bool sync = true) {
  hipLaunchKernelGGL(gs_k_scalars, dim3(h->groups), dim3(64), 0, h->stream, h->rows_f, (int)SF_COUNT, h->rows_i,
                     (int)SI_COUNT, h->rows_u, (int)SU_COUNT, h->R.total, h->slab, h->hd_f, h->hd_i, h->hd_u, h->Bp, h->hd_v4, (int)SU_VF0);
  HIPCHK(h, hipGetLastError());
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

void launch_dense(gs_handle* h, int grid, const GsDenseArgs& args, double* slab, int nb) {
#if defined(GS_BUILD_EXPERIMENTS)
  if (!h->dense_blockrow) { hipLaunchKernelGGL(gs_k_nr_dense_mfma, dim3(grid), dim3(256), h->dense_lds, h->stream, args, slab, nb); return; }
#endif
  hipLaunchKernelGGL(gs_k_nr_dense_mfma2, dim3(grid), dim3(256), h->dense_lds, h->stream, args, slab, nb);
}

// the linear solve of nr_dense_mfma / nr_sparse_lds: a launch of its own between the two halves of the step / solve
void launch_linear(gs_handle* h) {
#if defined(GS_BUILD_EXPERIMENTS)
  if (h->solve == SolveMember::nr_sparse_lds) {
    hipLaunchKernelGGL(gs_k_nr_sparse_lds, dim3(h->sparse_grid), dim3(64 * h->SA.waves), h->sparse_lds, h->stream, h->SA, h->slab, h->B);
    return;
  }
#endif
  launch_dense(h, h->dense_grid, h->DA, h->slab, h->B);
}

int launch_solve(gs_handle* h) {
  LaunchTimer lt(h, GS_K_SOLVE);
  GsSolveFn k = gs_solve_kernels[(int)h->solve].solve;
  if (!k) {         // nr_dense_mfma / nr_sparse_lds: the linear solve, then line flows, losses and angles
    launch_linear(h);
    k = gs_k_posts_nr_dmfma;
  }
  hipLaunchKernelGGL(k, dim3(h->groups), dim3(64 * h->W), h->dyn_lds, h->stream, h->T, h->R, h->SC, h->slab, h->B);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

GsFusedChecks fused_checks_args(gs_handle* h);      // defined with gs_checks below

// obs_out: where the step writes the changing columns of its observation block ([B][obs_dim], constants already in
// place); NULL = the other one of the handle's two observation buffers
int step_kernels(gs_handle* h, const double* d_actions, double* obs_out = nullptr, const GsRolloutStep* rs = nullptr) {
  // one fused launch: actions -> pre-solve dynamics -> load flow -> post-solve dynamics / reward / flags
  { LaunchTimer lt(h, GS_K_SOLVE);
    dim3 grid(h->groups), block(64 * h->W);
    if (!obs_out) {
      const int next = h->obs_cur ^ 1;
      if (h->gather_pending[next]) {
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_gather[next], 0));
        if (h->split_ok) HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_gather[next], 0));     // (the second half writes the same buffer)
        h->gather_pending[next] = false;
      }
      h->obs_cur = next;
      obs_out = h->d_obs2[next];
    }
    GsPackArgs pa{h->map_obs, h->d_cst, obs_out, h->obs_dim, (int)std::max<size_t>(1, std::min<size_t>(3, (h->dyn_lds - 49152) / (64 * 65 * sizeof(double)))), 0, 0,
                  h->obs_skip0, h->obs_skip1};
    pa.pair_ok = !(h->obs_dim & 1) && !((h->obs_skip1 - h->obs_skip0) & 1) && pa.tiles_per_pass >= 2 && !GS_EXPERIMENT_ENV("GS_PACK_BY_COLUMN");
    pa.early_pass0 = 2 * h->n + 2 * h->m >= 64 * pa.tiles_per_pass;   // the frequency column (grid_env.py:766) lies beyond the first pass
    pa.lean = h->lean ? 1 : 0;
    if (h->lean) { h->rows_stale = true; h->last_obs = obs_out; }
    const GsFusedChecks fc = fused_checks_args(h);
    const GsRolloutStep rsv = rs ? *rs : GsRolloutStep{};
    if (h->second_gen()) {        // 64 / IW workgroups per 64-instance slab group, each with its own IW instances
      const int per_group = 64 / h->f2().iw, n_wg = h->groups * per_group;
      const dim3 b2(64 * h->f2().nw);
      // (two half-grid launches on two streams, see gs_handle::forked; the halves are whole 64-instance slab groups)
      // (per-launch event pairs, gs_timing_enable(1), bracket ONE launch on the main stream: the step stays whole then)
      const bool split = h->split_ok && !h->timing;
      const int n_first = split ? (h->groups / 2) * per_group : n_wg;
      if (split && !h->forked) {
        HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
        HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
        h->forked = true;
      }
      GsF2Tables f2a = h->F2, f2b = h->F2;
      f2a.wg_offset = 0; f2b.wg_offset = n_first;
      // the handle's form of its member; pz, pl: the per-instance line impedances / load powers, behind the argument block (null
      // where the handle has none: its form does not read them)
      const GsStepFns<GsF2StepFn>& form = gs_step_kernels[(int)h->step].form[h->pz][h->pl];
      const GsF2StepFn k = fc.enabled ? form.stepc : form.step;
      if (!k) return fail(h, GS_E_STATE, "%s: no such step kernel", h->f2().name);
      const double *pz = h->LP.pz, *pl = h->LL.pl;
      hipLaunchKernelGGL(k, dim3(n_first), b2, h->F2.lds_bytes, h->stream, h->T, f2a, h->R, h->SC, h->EC, h->slab, h->B, d_actions, h->total_load, pa, fc, rsv, pz, pl);
      if (n_first < n_wg)
        hipLaunchKernelGGL(k, dim3(n_wg - n_first), b2, h->F2.lds_bytes, h->stream2, h->T, f2b, h->R, h->SC, h->EC, h->slab, h->B, d_actions, h->total_load, pa, fc, rsv, pz, pl);
      HIPCHK(h, hipGetLastError());
      return GS_OK;
    }
    const GsStepFns<GsStepFn> k = gs_solve_kernels[(int)h->solve].step;
#define GS_STEP(k) hipLaunchKernelGGL(k, grid, block, h->dyn_lds, h->stream, h->T, h->R, h->SC, h->EC, h->slab, h->B, d_actions, h->total_load, pa, fc)
    if (k.step) GS_STEP(fc.enabled ? k.stepc : k.step);
    else {        // nr_dense_mfma / nr_sparse_lds: prologue | the linear solve, one workgroup / wavefront per instance | epilogue + observation pack
      GS_STEP(gs_k_pre_nr_dmfma);
      launch_linear(h);
      GS_STEP(fc.enabled ? gs_k_postc_nr_dmfma : gs_k_post_nr_dmfma);
    }
#undef GS_STEP
    HIPCHK(h, hipGetLastError()); }
  return GS_OK;     // the observation block was written by the step kernel itself
}

void copy_info(gs_handle* h, double* reward, uint8_t* term, uint8_t* trunc, const gs_info_view* info) {
  const int B = h->B, Bp = h->Bp;
  const double* f = h->h_f; const int32_t* i32 = h->h_i; const uint8_t* u = h->h_u;
  if (reward) memcpy(reward, f + (size_t)SF_REWARD * Bp, B * sizeof(double));
  if (term) memcpy(term, u + (size_t)SU_TERM * Bp, B);
  if (trunc) memcpy(trunc, u + (size_t)SU_TRUNC * Bp, B);
  if (!info) return;
  if (info->power_flow_converged) memcpy(info->power_flow_converged, u + (size_t)SU_CONV * Bp, B);
  if (info->max_voltage) memcpy(info->max_voltage, f + (size_t)SF_VMAX * Bp, B * sizeof(double));
  if (info->min_voltage) memcpy(info->min_voltage, f + (size_t)SF_VMIN * Bp, B * sizeof(double));
  if (info->total_losses) memcpy(info->total_losses, f + (size_t)SF_LOSSES * Bp, B * sizeof(double));
  if (info->violations) memcpy(info->violations, h->h_v4, (size_t)B * 4);      // (the four flags of an instance, interleaved by the kernel)
  if (info->constraint_violations) memcpy(info->constraint_violations, i32 + (size_t)SI_VIOL * Bp, B * sizeof(int32_t));
  if (info->current_step) memcpy(info->current_step, i32 + (size_t)SI_STEP * Bp, B * sizeof(int32_t));
  if (info->episode_reward) memcpy(info->episode_reward, f + (size_t)SF_EPREW * Bp, B * sizeof(double));
  if (info->iterations) memcpy(info->iterations, i32 + (size_t)SI_ITERS * Bp, B * sizeof(int32_t));
  if (info->status) memcpy(info->status, i32 + (size_t)SI_STATUS * Bp, B * sizeof(int32_t));
}


// argument checks of gs_create and gs_plan_describe
int check_args(const gs_topology* topo, const gs_config* cfg, int32_t batch) {
  if (!topo || !cfg) return fail(nullptr, GS_E_INVALID, "topology / config is NULL");
  if (topo->struct_size != (int32_t)sizeof(gs_topology) || cfg->struct_size != (int32_t)sizeof(gs_config))
    return fail(nullptr, GS_E_INVALID, "struct_size mismatch (ABI %d): topology %d vs %zu, config %d vs %zu",
                GS_ABI_VERSION, topo->struct_size, sizeof(gs_topology), cfg->struct_size, sizeof(gs_config));
  if (batch <= 0) return fail(nullptr, GS_E_INVALID, "batch must be > 0");
  if (cfg->max_iterations < 1) return fail(nullptr, GS_E_INVALID, "max_iterations must be >= 1");
  if (!(cfg->power_base > 0.0)) return fail(nullptr, GS_E_INVALID, "power_base must be > 0");
  if (!(cfg->timestep > 0.0)) return fail(nullptr, GS_E_INVALID, "timestep must be > 0");
  if ((topo->line_r_inst == nullptr) != (topo->line_x_inst == nullptr))
    return fail(nullptr, GS_E_INVALID, "line_r_inst and line_x_inst go together (both NULL or both [batch][m])");
  if (topo->line_r_inst && topo->m > 0 && topo->r && topo->x) {
    const std::string why = gs_check_line_impedances(*topo, batch, topo->line_r_inst, topo->line_x_inst, nullptr);
    if (!why.empty()) return fail(nullptr, GS_E_INVALID, "%s", why.c_str());
  }
  if (topo->load_base_inst) {
    const std::string why = gs_check_load_powers(topo->n_loads, batch, topo->load_base_inst, nullptr);
    if (!why.empty()) return fail(nullptr, GS_E_INVALID, "%s", why.c_str());
  }
  return GS_OK;
}

// gs_k_load_params for the instances of mask (device, NULL = all)
int launch_load_params(gs_handle* h, const uint8_t* d_mask) {
  GsLoadParamArgs A = h->LL;
  A.mask = d_mask;
  const size_t threads = (size_t)h->groups * GS_LANES * (GS_PL_NP(A.n_loads) + 1);
  hipLaunchKernelGGL(gs_k_load_params, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, A);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

// gs_k_line_params for the instances of mask (device, NULL = all)
int launch_line_params(gs_handle* h, const uint8_t* d_mask) {
  GsLineParamArgs A = h->LP;
  A.mask = d_mask;
  const size_t threads = (size_t)h->groups * GS_LANES * (A.n_slots + A.m);
  hipLaunchKernelGGL(gs_k_line_params, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, A);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

// the topology compiled and the handle planned (host only), or the rejection as the library's error
int plan_handle(const gs_topology& topo, const gs_config& cfg, int32_t batch, int cus, HostTopology& ht, GsPlan& p) {
  std::string why = gs_compile_topology(topo, cfg.zero_z_mode, cfg.linear_solver == GS_LINSOLVE_SPARSE_LU,
                                        cfg.solver_kind == GS_SOLVER_NR && cfg.jacobian_mode == GS_JACOBIAN_AS_CODED &&
                                            (cfg.linear_solver == GS_LINSOLVE_AUTO || cfg.linear_solver == GS_LINSOLVE_DENSE_PIVOT),
                                        ht);
  if (!why.empty()) return fail(nullptr, GS_E_INVALID, "topology: %s", why.c_str());
  why = gs_plan(topo, cfg, ht, batch, cus, p);
  if (!why.empty()) return fail(nullptr, p.err_code, "%s", why.c_str());
  return GS_OK;
}

// The flat-start captures.  Iteration 0 of every solve starts from the flat start, where the Jacobian is the same for every
// instance: what it computes from it is computed once here, by the solver kernels themselves (bit-identical: the same blocks,
// the same operations), and kept as a table that iteration 0 then reads.
int flat_start_captures(gs_handle* h) {
  const HostTopology& ht = h->topo;
  const GsRows& R = h->R;
  int rc = 0;
  // dense block LU: the block factors, by one workgroup of the solver kernel in mode 1 (gs_create allocated DA.flat)
  if (h->DA.flat) {
    GsDenseArgs once = h->DA;
    once.jinv_t = nullptr; once.mode = 1; once.max_it = 1;
    launch_dense(h, 1, once, nullptr, 1);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
      return fail(nullptr, GS_E_HIP, "dense_mfma: factorisation of the flat-start Jacobian failed");
  }
#if defined(GS_BUILD_EXPERIMENTS)
  // sparse block LU in LDS: the factors, by one workgroup of the solver kernel in mode 1 (GS_LU_NO_FLAT=1: off)
  if (h->solve == SolveMember::nr_sparse_lds && !getenv("GS_LU_NO_FLAT")) {
    double* flat = nullptr;
    if ((rc = dev_alloc(h, &flat, (size_t)4 * (ht.lu_n_slots + ht.n) + 4))) return rc;
    GsSparseArgs once = h->SA;
    once.flat_out = flat; once.mode = 1; once.max_it = 1;
    hipLaunchKernelGGL(gs_k_nr_sparse_lds, dim3(1), dim3(64 * h->SA.waves), h->sparse_lds, h->stream, once, h->slab, 1);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
      return fail(nullptr, GS_E_HIP, "sparse_lds: factorisation of the flat-start Jacobian failed");
    h->SA.flat = flat;
  }
#endif
  // Sparse block LU (GsTables::lu_flat): one ordinary solve of group 0, capped at one iteration, leaves the factors in the rows
  // of lane 0; they are kept as a table of wave-uniform scalars and iteration 0 then only carries its right-hand side through
  // (kernels_solve.hip, linsolve_lu_flat).  GS_LU_NO_FLAT=1: off.
  if (h->solve == SolveMember::nr_sparse_lu && ht.lu_n_piv > 0 && !getenv("GS_LU_NO_FLAT")) {
    double* tab = nullptr;
    const int nblk = ht.lu_n_slots + ht.n;
    if ((rc = dev_alloc(h, &tab, (size_t)4 * nblk + 4))) return rc;
    hipLaunchKernelGGL(gs_k_fill_rows, dim3(1), dim3(64), 0, h->stream, R.P.base, 2, ht.n, R.total, h->slab, -0.01);
    hipLaunchKernelGGL(gs_k_fill_rows, dim3(1), dim3(64), 0, h->stream, R.Q.base, 2, ht.n, R.total, h->slab, 0.0);
    GsSolveCfg once = h->SC; once.max_iterations = 1; once.stamps = nullptr;
    hipLaunchKernelGGL(gs_solve_kernels[(int)h->solve].solve, dim3(1), dim3(64 * h->W), h->dyn_lds, h->stream, h->T, h->R, once, h->slab, 1);
    if (ht.lu_n_slots > 0)
      hipLaunchKernelGGL(gs_k_gather_lane, dim3((4 * ht.lu_n_slots + 255) / 256), dim3(256), 0, h->stream, R.LU, 4 * ht.lu_n_slots, 0, h->slab, tab);
    hipLaunchKernelGGL(gs_k_gather_lane, dim3((4 * ht.n + 255) / 256), dim3(256), 0, h->stream, R.LUD, 4 * ht.n, 0, h->slab, tab + (size_t)4 * ht.lu_n_slots);
    double status = 0.0;
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
        hipMemcpy(&status, h->slab + GS_ELEM(R.STATUS, 0), sizeof status, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(nullptr, GS_E_HIP, "sparse LU: factorisation of the flat-start Jacobian failed");
    const double flag = status == (double)GS_STATUS_SINGULAR ? 1.0 : 0.0;
    if (hipMemcpy(tab + (size_t)4 * nblk, &flag, sizeof flag, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(h->slab, 0, (size_t)R.total * GS_LANES * sizeof(double)) != hipSuccess)      // group 0 as gs_create leaves every group
      return fail(nullptr, GS_E_HIP, "sparse LU: flat-start table");
    h->T.lu_flat = tab;
  }
  // Newton-Raphson on the second-generation frame: the constants of the flat-start elimination (GsF2Tables::nrflat), written by
  // ONE workgroup of the step kernel itself on the zeroed state of group 0, then group 0 is cleared again.  GS_NR_NO_FLAT=1: off.
  // (GsPlan::nr_flat: a Newton-Raphson member, GS_NR_NO_FLAT unset, no per-instance impedances -- the table is the flat start's of
  // the shared Ybus)
  if (h->nr_flat) {
    double* tab = nullptr;
    const size_t npos = h->f2().positions();
    if ((rc = dev_alloc(h, &tab, npos * 16))) return rc;
    if (hipMemset(tab, 0, npos * 16 * sizeof(double)) != hipSuccess ||
        hipMemset(h->d_in, 0, h->in_doubles * sizeof(double)) != hipSuccess ||     // (d_in: zero actions for the capture step)
        hipDeviceSynchronize() != hipSuccess) return fail(nullptr, GS_E_HIP, "hipMemset failed");      // (and the memsets done before the capture reads)
    GsF2Tables cap = h->F2; cap.nrflat = tab; cap.nrflat_mode = 1; cap.wg_offset = 0;
    GsPackArgs pa{}; GsFusedChecks fc{}; GsRolloutStep rsv{};
    GsSolveCfg sc = h->SC; sc.stamps = nullptr;
    hipLaunchKernelGGL(gs_step_kernels[(int)h->step].form[0][0].step, dim3(1), dim3(64 * h->f2().nw), h->F2.lds_bytes, h->stream, h->T, cap, h->R, sc,
                       h->EC, h->slab, std::min(h->B, h->f2().iw), h->d_in, h->total_load, pa, fc, rsv, nullptr, nullptr);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
        hipMemset(h->slab, 0, (size_t)R.total * GS_LANES * sizeof(double)) != hipSuccess)
      return fail(nullptr, GS_E_HIP, "Newton-Raphson: flat-start table");
    h->F2.nrflat = tab; h->F2.nrflat_mode = 2;
  }
  return GS_OK;
}

}  // namespace

// =============================================================================================
extern "C" {

int gs_version(void) { return GS_ABI_VERSION; }

int gs_build_experiments(void) {
#if defined(GS_BUILD_EXPERIMENTS)
  return 1;
#else
  return 0;
#endif
}

int gs_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

const char* gs_last_error(const gs_handle* h) { return h ? h->err.c_str() : g_last_error.c_str(); }

int gs_create(const gs_topology* topo, const gs_config* cfg, int32_t batch, int32_t device,
              int64_t first_instance, gs_handle** out) {
  if (!out) return fail(nullptr, GS_E_INVALID, "out is NULL");
  *out = nullptr;
  int rc = check_args(topo, cfg, batch);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, GS_E_NO_DEVICE, "no HIP device visible: libgridstep has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(nullptr, GS_E_NO_DEVICE, "device %d out of range (0..%d)", device, ndev - 1);
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);

  gs_handle* h = new gs_handle();
  h->device = device;
  h->cfg = *cfg;
  if ((rc = plan_handle(*topo, *cfg, batch, cus, h->topo, *h))) { delete h; return rc; }
  const HostTopology& ht = h->topo;
  h->EC.first_instance = first_instance;
  h->line_x.assign(topo->x, topo->x + topo->m);
  h->nominal_r.assign(topo->r, topo->r + topo->m); h->nominal_x.assign(topo->x, topo->x + topo->m);
  auto bail = [&](int rc) { gs_destroy(h); return rc; };
  if (hipSetDevice(device) != hipSuccess) return bail(fail(nullptr, GS_E_HIP, "hipSetDevice failed"));
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(nullptr, GS_E_HIP, "hipStreamCreate failed"));

  {
    // the attribute is per function, i.e. shared by every handle of the process: always raise it to the most any handle may ask
    // for -- the first generation: 160 KB per workgroup minus the 24 KB static block; the second has no static LDS
    auto raise = [](auto f, int bytes) { return !f || hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess; };
    const int max_dyn = 160 * 1024 - 24576;
    bool ok = raise(gs_k_pre_nr_dmfma, max_dyn) && raise(gs_k_post_nr_dmfma, max_dyn) && raise(gs_k_postc_nr_dmfma, max_dyn) && raise(gs_k_posts_nr_dmfma, max_dyn);
    for (const GsSolveKernels& k : gs_solve_kernels) ok = ok && raise(k.solve, max_dyn) && raise(k.step.step, max_dyn) && raise(k.step.stepc, max_dyn);
    if (!ok) return bail(fail(nullptr, GS_E_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize=%d) failed", max_dyn));
    for (const GsStepKernels& k : gs_step_kernels)
      for (const auto& forms : k.form)
        for (const GsStepFns<GsF2StepFn>& f : forms) ok = ok && raise(f.step, 160 * 1024) && raise(f.stepc, 160 * 1024);
#if defined(GS_BUILD_EXPERIMENTS)
    ok = ok && raise(gs_k_nr_sparse_lds, 160 * 1024);
#endif
    if (!ok) return bail(fail(nullptr, GS_E_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize=%d) failed", 160 * 1024));
    hipError_t e = hipFuncSetAttribute((const void*)gs_k_nr_dense_mfma2, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
#if defined(GS_BUILD_EXPERIMENTS)
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)gs_k_nr_dense_mfma, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
#endif
    if (e != hipSuccess) return bail(fail(nullptr, GS_E_HIP, "hipFuncSetAttribute(gs_k_nr_dense_mfma): %s", hipGetErrorString(e)));
  }

  // ---- uploads (the table arena packs them in this order) ----
  if (!h->mesh_w.empty() && (rc = dev_upload(h, &h->F2.mesh_w, h->mesh_w))) return bail(rc);
  GsTables& T = h->T;
  T.n = h->n; T.m = h->m; T.nnz = ht.nnz; T.n_levels = ht.n_levels;
  T.n_loads = h->n_loads; T.n_gens = h->n_gens; T.n_bats = h->n_bats;
  T.lu_n_piv = ht.lu_n_piv; T.lu_n_slots = ht.lu_n_slots; T.lu_n_orig = ht.lu_n_orig; T.lu_n_levels = ht.lu_n_levels;
  T.dn_N = ht.dn_N;
#define UP(field, vec) if ((rc = dev_upload(h, &T.field, ht.vec))) return bail(rc)
  UP(ell_col, ell_col); UP(ell_G, ell_G); UP(ell_B, ell_B); UP(rem_ptr, rem_ptr); UP(rem_col, rem_col);
  UP(rem_G, rem_G); UP(rem_B, rem_B);
  UP(row_ptr, row_ptr); UP(col, col); UP(G, G); UP(Bv, B); UP(Gd, Gd); UP(Bd, Bd);
  UP(th_free, th_free); UP(vm_free, vm_free); UP(v_set, v_set); UP(fixed_v, fixed_v);
  UP(lvl_ptr, lvl_ptr); UP(lvl_bus, lvl_bus); UP(parent, parent); UP(parent_pos, parent_pos);
  UP(child_ptr, child_ptr); UP(child_idx, child_idx); UP(lvl_pos, lvl_pos);
  if ((rc = dev_upload(h, &T.winj, h->winj)) || (rc = dev_upload(h, &T.wi_ptr, h->wi_ptr))) return bail(rc);
  if ((rc = dev_upload(h, &T.wbus, h->wbus)) || (rc = dev_upload(h, &T.wb_ptr, h->wb_ptr))) return bail(rc);
  if ((rc = dev_upload(h, &T.witems, h->witems)) || (rc = dev_upload(h, &T.wl_ptr, h->wl_ptr)) || (rc = dev_upload(h, &T.ovf_slot, h->ovf_slot))) return bail(rc);
  T.max_level_width = ht.max_level_width;
  UP(fbs_parent, fbs_parent); UP(fbs_parent_pos, fbs_parent_pos);
  UP(lfrom, lfrom); UP(lto, lto); UP(lyr, lyr); UP(lyi, lyi); UP(lrating, lrating); UP(lrating_inv, lrating_inv);
  UP(lu_piv_bus, lu_piv_bus); UP(lu_nb_ptr, lu_nb_ptr); UP(lu_nb_bus, lu_nb_bus); UP(lu_nb_kj, lu_nb_kj);
  UP(lu_nb_jk, lu_nb_jk); UP(lu_pair_ptr, lu_pair_ptr); UP(lu_pair_ik, lu_pair_ik); UP(lu_pair_kj, lu_pair_kj);
  UP(lu_pair_ij, lu_pair_ij); UP(lu_orig_slot, lu_orig_slot); UP(lu_orig_i, lu_orig_i); UP(lu_orig_j, lu_orig_j);
  UP(lu_orig_pos, lu_orig_pos);
  if ((rc = dev_upload(h, &T.lu_a_ptr, h->lu_a_ptr)) || (rc = dev_upload(h, &T.lu_a, h->lu_a)) || (rc = dev_upload(h, &T.lu_b_ptr, h->lu_b_ptr)) ||
      (rc = dev_upload(h, &T.lu_b, h->lu_b)) || (rc = dev_upload(h, &T.lu_c_ptr, h->lu_c_ptr)) || (rc = dev_upload(h, &T.lu_c, h->lu_c)) ||
      (rc = dev_upload(h, &T.lu_r_ptr, h->lu_r_ptr)) || (rc = dev_upload(h, &T.lu_r, h->lu_r))) return bail(rc);
  UP(dn_th_idx, dn_th_idx); UP(dn_vm_idx, dn_vm_idx);
  UP(bl_ptr, bl_ptr); UP(bl_idx, bl_idx); UP(bg_ptr, bg_ptr); UP(bg_idx, bg_idx); UP(bb_ptr, bb_ptr); UP(bb_idx, bb_idx);
  UP(load_base, load_base); UP(load_q, load_q); UP(gen_kind, gen_kind); UP(gen_cap, gen_cap); UP(gen_p0, gen_p0);
  UP(gen_p1, gen_p1); UP(gen_p2, gen_p2); UP(bat_cap, bat_cap); UP(bat_rating, bat_rating); UP(bat_eff, bat_eff);
#undef UP
  if (h->solve == SolveMember::nr_dense_mfma) {
    GsDenseArgs& D = h->DA;
    if ((rc = dev_upload(h, &D.act_bus, h->act_bus)) || (rc = dev_upload(h, &D.act_of, h->act_of)) || (rc = dev_upload(h, &D.ent_ptr, h->ent_ptr)) ||
        (rc = dev_upload(h, &D.ent, h->ent)) || (rc = dev_upload(h, &D.bent_ptr, h->bent_ptr)) || (rc = dev_upload(h, &D.bent, h->bent))) return bail(rc);
    D.row_ptr = T.row_ptr; D.col = T.col; D.G = T.G; D.Bv = T.Bv; D.Gd = T.Gd; D.Bd = T.Bd;
    D.th_free = T.th_free; D.vm_free = T.vm_free; D.fixed_v = T.fixed_v; D.v_set = T.v_set;
    const size_t blocks = (size_t)D.NB * D.NB * 64 * 64;
    if ((rc = dev_alloc(h, &D.scratch, (size_t)h->dense_grid * blocks)) || (h->dense_flat && (rc = dev_alloc(h, &D.flat, blocks + 8))) ||
        (!h->jinv_t.empty() && (rc = dev_upload(h, &D.jinv_t, h->jinv_t)))) return bail(rc);
  }
  if (h->step == StepMember::nr_mesh2 &&
      ((rc = dev_upload(h, &h->F2.mesh_items, h->mesh_items)) || (rc = dev_upload(h, &h->F2.mesh_rowinfo, h->mesh_rowinfo)))) return bail(rc);
  if (h->second_gen() &&
      ((rc = dev_upload(h, &h->F2.recs, h->f2recs)) || (rc = dev_upload(h, &h->F2.anc, h->f2anc)) || (rc = dev_upload(h, &h->F2.zbus, h->f2z)) ||
       (h->fs_slot.size() > 1 && ((rc = dev_upload(h, &h->F2.fixed_slot, h->fs_slot)) || (rc = dev_upload(h, &h->F2.fixed_val, h->fs_val)))))) return bail(rc);
  if (h->pz) {
    GsLineParamArgs& A = h->LP;
    const size_t Bm = (size_t)h->B * h->m;
    h->inst_r.assign(topo->line_r_inst, topo->line_r_inst + Bm); h->inst_x.assign(topo->line_x_inst, topo->line_x_inst + Bm);
    A.B = h->B; A.groups = h->groups; A.n_slots = ht.n + 3; A.m = ht.m; A.newton = h->f2().newton() ? 1 : 0;
    A.lyr_nom = T.lyr; A.lyi_nom = T.lyi;
    double *dr = nullptr, *dx = nullptr, *dpz = nullptr;
    const size_t n_pz = (size_t)h->groups * GS_PZ_NQ(A.n_slots, A.m) * GS_LANES * 2;
    if ((rc = dev_upload(h, &A.zero_z, h->pz_zero)) || (rc = dev_upload(h, &A.ops_ptr, h->pz_ops_ptr)) || (rc = dev_upload(h, &A.ops, h->pz_ops)) ||
        (rc = dev_upload(h, &A.has, h->pz_has)) || (rc = dev_alloc(h, &dr, Bm)) || (rc = dev_alloc(h, &dx, Bm)) ||
        (rc = dev_alloc(h, &h->d_pzmask, (size_t)h->B)) || (rc = dev_alloc(h, &dpz, n_pz))) return bail(rc);
    A.r = dr; A.x = dx; A.pz = dpz;
    // (the handle's stream is non-blocking: it is not ordered behind the null stream's copies and memsets, which may still be
    // running when they return -- gs_k_line_params then read r / x half copied, or the memset zeroed entries it had written)
    if (hipMemcpy(dr, h->inst_r.data(), Bm * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dx, h->inst_x.data(), Bm * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(dpz, 0, n_pz * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      return bail(fail(nullptr, GS_E_HIP, "per-instance line impedances: upload failed"));
    if ((rc = launch_line_params(h, nullptr))) return bail(fail(nullptr, rc, "%s", h->err.c_str()));
  }
  if (h->pl) {
    GsLoadParamArgs& A = h->LL;
    const size_t Bl = (size_t)h->B * h->n_loads;
    h->inst_load.assign(topo->load_base_inst, topo->load_base_inst + Bl);
    A.B = h->B; A.groups = h->groups; A.n_loads = h->n_loads;
    double *db = nullptr, *dpl = nullptr;
    const size_t n_pl = (size_t)h->groups * GS_PL_NQ(A.n_loads) * GS_LANES * 2;
    if ((rc = dev_upload(h, &A.tan_phi, h->pl_tan)) || (rc = dev_alloc(h, &db, Bl)) || (rc = dev_alloc(h, &h->d_plmask, (size_t)h->B)) ||
        (rc = dev_alloc(h, &dpl, n_pl))) return bail(rc);
    A.base = db; A.pl = dpl;
    // (as for the line impedances above: the null stream's copy and memset are complete before the handle's stream derives from them)
    if (hipMemcpy(db, h->inst_load.data(), Bl * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(dpl, 0, n_pl * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      return bail(fail(nullptr, GS_E_HIP, "per-instance load powers: upload failed"));
    if ((rc = launch_load_params(h, nullptr))) return bail(fail(nullptr, rc, "%s", h->err.c_str()));
  }
  { const double* q = nullptr; if ((rc = dev_upload(h, &q, h->cst))) return bail(rc); h->d_cst = const_cast<double*>(q); }
  if ((rc = upload_map(h, &h->map_obs, h->mo)) || (rc = upload_map(h, &h->map_vm, h->mvm)) || (rc = upload_map(h, &h->map_va, h->mva)) ||
      (rc = upload_map(h, &h->map_flow, h->mfl)) || (rc = upload_map(h, &h->map_load, h->mld)) || (rc = upload_map(h, &h->map_p, h->mp)) ||
      (rc = upload_map(h, &h->map_q, h->mq)) || (rc = upload_map(h, &h->map_act, h->mact)) || (rc = upload_map(h, &h->map_state, h->mst)) ||
      (rc = upload_map(h, &h->rows_f, h->rf)) || (rc = upload_map(h, &h->rows_i, h->ri)) || (rc = upload_map(h, &h->rows_u, h->ru)))
    return bail(rc);

  // ---- big buffers ----
  const size_t slab_doubles = (size_t)h->groups * h->R.total * GS_LANES;
  if ((rc = dev_alloc(h, &h->slab, slab_doubles))) return bail(rc);
  if (hipMemset(h->slab, 0, slab_doubles * sizeof(double)) != hipSuccess) return bail(fail(nullptr, GS_E_HIP, "hipMemset(slab) failed"));
  const size_t widest = std::max<size_t>({(size_t)h->obs_dim, (size_t)h->state_dim, (size_t)h->n, (size_t)h->m, (size_t)h->action_dim, 1});
  h->in_doubles = (size_t)h->B * widest; h->out_doubles = (size_t)h->B * widest;
  if ((rc = dev_alloc(h, &h->d_in, h->in_doubles)) || (rc = dev_alloc(h, &h->d_out, h->out_doubles)) ||
      (rc = dev_alloc(h, &h->d_obs2[0], (size_t)h->Bp * h->obs_dim)) || (rc = dev_alloc(h, &h->d_obs2[1], (size_t)h->Bp * h->obs_dim))) return bail(rc);
  if ((rc = dev_alloc(h, &h->sc_f, (size_t)SF_COUNT * h->Bp)) || (rc = dev_alloc(h, &h->sc_i, (size_t)SI_COUNT * h->Bp)) ||
      (rc = dev_alloc(h, &h->sc_u, (size_t)SU_COUNT * h->Bp)) || (rc = dev_alloc(h, &h->d_seeds, (size_t)h->B)) ||
      (rc = dev_alloc(h, &h->d_mask, (size_t)h->B)))
    return bail(rc);
  {
    const size_t nf = (size_t)SF_COUNT * h->Bp * sizeof(double), ni = (size_t)SI_COUNT * h->Bp * sizeof(int32_t), nv = (size_t)h->Bp * sizeof(uint32_t),
                 nu = (size_t)SU_COUNT * h->Bp;
    void* dp = nullptr;
    if (hipHostMalloc(&h->h_pin, nf + ni + nv + nu, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&dp, h->h_pin, 0) != hipSuccess) {
      (void)hipGetLastError();
      return bail(fail(nullptr, GS_E_NOMEM, "hipHostMalloc(%zu bytes, mapped) for the per-instance scalars failed", nf + ni + nv + nu));
    }
    memset(h->h_pin, 0, nf + ni + nv + nu);
    char* hp = (char*)h->h_pin; char* dv = (char*)dp;
    h->h_f = (double*)hp; h->h_i = (int32_t*)(hp + nf); h->h_v4 = (uint32_t*)(hp + nf + ni); h->h_u = (uint8_t*)(hp + nf + ni + nv);
    h->hd_f = (double*)dv; h->hd_i = (int32_t*)(dv + nf); h->hd_v4 = (uint32_t*)(dv + nf + ni); h->hd_u = (uint8_t*)(dv + nf + ni + nv);
  }
#if defined(GS_BUILD_EXPERIMENTS)
  if (h->solve == SolveMember::nr_sparse_lds) {
    GsSparseArgs& Sp = h->SA;
    if ((rc = dev_upload(h, &Sp.ipack, h->ipack)) || (rc = dev_upload(h, &Sp.dpack, h->dpack))) return bail(rc);
    Sp.orig_slot = T.lu_orig_slot; Sp.orig_i = T.lu_orig_i; Sp.orig_j = T.lu_orig_j; Sp.orig_pos = T.lu_orig_pos;
  }
#endif
  // (the captures run on the handle's stream: the tables, the zeroed slab and the rest of the null stream's work go first)
  if (hipDeviceSynchronize() != hipSuccess) return bail(fail(nullptr, GS_E_HIP, "hipDeviceSynchronize failed"));
  if ((rc = flat_start_captures(h))) return bail(rc);
  if (h->split_ok &&
      (hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking) != hipSuccess ||
       hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
       hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess))
    return bail(fail(nullptr, GS_E_HIP, "second step stream: hipStreamCreate / hipEventCreate failed"));
  if (hipDeviceSynchronize() != hipSuccess) return bail(fail(nullptr, GS_E_HIP, "hipDeviceSynchronize failed"));
  *out = h;
  return GS_OK;
}

void gs_destroy(gs_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream2) (void)hipStreamSynchronize(h->stream2);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
  if (h->loop || h->comm) (void)gs_comm_destroy(h);
  if (h->stream2) { (void)hipStreamDestroy(h->stream2); (void)hipEventDestroy(h->ev_fork); (void)hipEventDestroy(h->ev_join); }
  if (h->ev_peer) (void)hipEventDestroy(h->ev_peer);
  if (h->ev_peer2) (void)hipEventDestroy(h->ev_peer2);
  if (h->ev_step) (void)hipEventDestroy(h->ev_step);
  if (h->ev_full) (void)hipEventDestroy(h->ev_full);
  if (h->ev_scalars) (void)hipEventDestroy(h->ev_scalars);
  for (int k = 0; k < 2; ++k) if (h->ev_gather[k]) (void)hipEventDestroy(h->ev_gather[k]);
  if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
  for (auto& t : h->timed) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
  if (h->span_a) { (void)hipEventDestroy(h->span_a); (void)hipEventDestroy(h->span_b); }
  for (void* p : h->allocs) (void)hipFree(p);
  if (h->d_actions) (void)hipFree(h->d_actions);
  if (h->pol.blob) (void)hipFree(h->pol.blob);
  if (h->pol.act) (void)hipFree(h->pol.act);
  for (void* p : {(void*)h->ro.obs_seq, (void*)h->ro.act, (void*)h->ro.rew, (void*)h->ro.done, (void*)h->ro.term_count,
                  (void*)h->ro.term_idx, (void*)h->ro.term_obs})
    if (p) (void)hipFree(p);
  if (h->h_pin) (void)hipHostFree(h->h_pin);
  if (h->d_obs_full) (void)hipFree(h->d_obs_full);
  if (h->d_gather_send) (void)hipFree(h->d_gather_send);
  if (h->d_gather_recv) (void)hipFree(h->d_gather_recv);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int gs_dims(const gs_handle* h, int32_t* n, int32_t* m, int32_t* obs_dim, int32_t* action_dim,
            int32_t* state_dim, int32_t* batch) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (n) *n = h->n; if (m) *m = h->m; if (obs_dim) *obs_dim = h->obs_dim; if (action_dim) *action_dim = h->action_dim;
  if (state_dim) *state_dim = h->state_dim; if (batch) *batch = h->B;
  return GS_OK;
}

int gs_describe(const gs_handle* h, char* buf, int32_t buflen) {
  if (!h || !buf || buflen <= 0) return fail(nullptr, GS_E_INVALID, "bad arguments");
  gs_plan_format(*h, h->topo, buf, buflen);
  return GS_OK;
}

int gs_plan_describe(const gs_topology* topo, const gs_config* cfg, int32_t batch, int32_t cus, char* buf, int32_t buflen) {
  if (!buf || buflen <= 0 || cus < 1) return fail(nullptr, GS_E_INVALID, "bad arguments");
  int rc = check_args(topo, cfg, batch);
  if (rc) return rc;
  HostTopology ht;
  GsPlan p;
  if ((rc = plan_handle(*topo, *cfg, batch, cus, ht, p))) return rc;
  gs_plan_format(p, ht, buf, buflen);
  return GS_OK;
}

int gs_synchronize(gs_handle* h) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->comm_stream) HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  return GS_OK;
}

// ---- per-instance line impedances ------------------------------------------------------------
int gs_set_line_impedances(gs_handle* h, const double* r, const double* x, const uint8_t* mask) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (!h->pz) return fail(h, GS_E_STATE, "gs_set_line_impedances: the handle was created without per-instance line impedances "
                                         "(gs_topology::line_r_inst / line_x_inst)");
  if (!r || !x) return fail(h, GS_E_INVALID, "gs_set_line_impedances: r and x are [B][m] and go together");
  gs_topology nominal{};
  nominal.m = h->m; nominal.r = h->nominal_r.data(); nominal.x = h->nominal_x.data();
  const std::string why = gs_check_line_impedances(nominal, h->B, r, x, mask);
  if (!why.empty()) return fail(h, GS_E_INVALID, "%s", why.c_str());
  GS_ENTER(h);
  const size_t m = (size_t)h->m;
  for (int b = 0; b < h->B; ++b) {
    if (mask && !mask[b]) continue;
    std::copy(r + b * m, r + (b + 1) * m, h->inst_r.begin() + b * m);
    std::copy(x + b * m, x + (b + 1) * m, h->inst_x.begin() + b * m);
  }
  // (a step still in flight may read the entries: the stream orders the copies and the derivation behind it)
  HIPCHK(h, hipMemcpyAsync(const_cast<double*>(h->LP.r), h->inst_r.data(), h->inst_r.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(const_cast<double*>(h->LP.x), h->inst_x.data(), h->inst_x.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (mask) HIPCHK(h, hipMemcpyAsync(h->d_pzmask, mask, (size_t)h->B, hipMemcpyHostToDevice, h->stream));
  int rc = launch_line_params(h, mask ? h->d_pzmask : nullptr);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));      // (the caller's mask and the host copies are pageable)
  return GS_OK;
}

int gs_get_line_impedances(const gs_handle* h, double* r, double* x) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (!h->pz) return fail(const_cast<gs_handle*>(h), GS_E_STATE, "gs_get_line_impedances: the handle has no per-instance line impedances");
  if (r) std::copy(h->inst_r.begin(), h->inst_r.end(), r);
  if (x) std::copy(h->inst_x.begin(), h->inst_x.end(), x);
  return GS_OK;
}

// ---- per-instance load powers -----------------------------------------------------------------
int gs_set_load_powers(gs_handle* h, const double* base, const uint8_t* mask) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (!h->pl) return fail(h, GS_E_STATE, "gs_set_load_powers: the handle was created without per-instance load powers "
                                         "(gs_topology::load_base_inst)");
  if (!base) return fail(h, GS_E_INVALID, "gs_set_load_powers: base is [B][n_loads]");
  const std::string why = gs_check_load_powers(h->n_loads, h->B, base, mask);
  if (!why.empty()) return fail(h, GS_E_INVALID, "%s", why.c_str());
  GS_ENTER(h);
  const size_t nl = (size_t)h->n_loads;
  for (int b = 0; b < h->B; ++b) {
    if (mask && !mask[b]) continue;
    std::copy(base + b * nl, base + (b + 1) * nl, h->inst_load.begin() + b * nl);
  }
  // (a step still in flight may read the entries: the stream orders the copy and the derivation behind it)
  HIPCHK(h, hipMemcpyAsync(const_cast<double*>(h->LL.base), h->inst_load.data(), h->inst_load.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (mask) HIPCHK(h, hipMemcpyAsync(h->d_plmask, mask, (size_t)h->B, hipMemcpyHostToDevice, h->stream));
  int rc = launch_load_params(h, mask ? h->d_plmask : nullptr);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));      // (the caller's mask and the host copy are pageable)
  return GS_OK;
}

int gs_get_load_powers(const gs_handle* h, double* base) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (!h->pl) return fail(const_cast<gs_handle*>(h), GS_E_STATE, "gs_get_load_powers: the handle has no per-instance load powers");
  if (base) std::copy(h->inst_load.begin(), h->inst_load.end(), base);
  return GS_OK;
}

// ---- solver -------------------------------------------------------------------------------
static const char* const kPzNoSolve = "gs_solve / gs_solve_device: this handle has per-instance line impedances, which the solver API does not "
                                      "support (the step, rollout and fallback entry points do)";
int gs_upload_injections(gs_handle* h, const double* P_spec, const double* Q_spec) {
  if (!h || !P_spec) return fail(h, GS_E_INVALID, "handle / P_spec is NULL");
  if (h->pz) return fail(h, GS_E_STATE, "%s", kPzNoSolve);
  GS_ENTER(h);
  int rc = unpack_from_host(h, h->map_p, h->n, P_spec);
  if (rc) return rc;
  if (Q_spec) {
    HIPCHK(h, hipStreamSynchronize(h->stream));      // d_in is reused
    rc = unpack_from_host(h, h->map_q, h->n, Q_spec);
    if (rc) return rc;
  } else {
    hipLaunchKernelGGL(gs_k_fill_rows, dim3(h->groups), dim3(64), 0, h->stream, h->R.Q.base, 2, h->n, h->R.total, h->slab, 0.0);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

int gs_solve_device(gs_handle* h) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (h->pz) return fail(h, GS_E_STATE, "%s", kPzNoSolve);
  GS_ENTER(h);
  h->rows_stale = false;            // the solve writes every result row
  return launch_solve(h);
}

int gs_download_solution(gs_handle* h, const gs_solution_view* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / view is NULL");
  GS_ENTER(h);
  int rc;
  if ((rc = ensure_rows(h))) return rc;
  if ((rc = pack_to_host(h, h->map_vm, h->n, out->bus_voltages))) return rc;
  if ((rc = pack_to_host(h, h->map_va, h->n, out->bus_angles))) return rc;
  if ((rc = pack_to_host(h, h->map_flow, h->m, out->line_flows))) return rc;
  if ((rc = pack_to_host(h, h->map_load, h->m, out->line_loadings))) return rc;
  if ((rc = fetch_scalars(h))) return rc;
  const int B = h->B, Bp = h->Bp;
  if (out->losses) memcpy(out->losses, h->h_f + (size_t)SF_LOSSES * Bp, B * sizeof(double));
  if (out->max_mismatch) memcpy(out->max_mismatch, h->h_f + (size_t)SF_MAXMIS * Bp, B * sizeof(double));
  if (out->iterations) memcpy(out->iterations, h->h_i + (size_t)SI_ITERS * Bp, B * sizeof(int32_t));
  if (out->status) memcpy(out->status, h->h_i + (size_t)SI_STATUS * Bp, B * sizeof(int32_t));
  if (out->converged) memcpy(out->converged, h->h_u + (size_t)SU_CONV * Bp, B);
  return GS_OK;
}

int gs_solve(gs_handle* h, const double* P_spec, const double* Q_spec, const gs_solution_view* out) {
  int rc = gs_upload_injections(h, P_spec, Q_spec);
  if (rc) return rc;
  if ((rc = gs_solve_device(h))) return rc;
  return out ? gs_download_solution(h, out) : gs_synchronize(h);
}

// ---- environment ----------------------------------------------------------------------------
int gs_reset(gs_handle* h, const uint64_t* seeds, const uint8_t* mask, double* obs_out) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  GS_ENTER(h);
  { int rc0 = ensure_rows(h); if (rc0) return rc0; }      // a masked reset leaves the other instances' rows as they are: they must be current
  if (seeds) HIPCHK(h, hipMemcpyAsync(h->d_seeds, seeds, (size_t)h->B * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
  if (mask) HIPCHK(h, hipMemcpyAsync(h->d_mask, mask, (size_t)h->B, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(gs_k_env_reset, dim3(h->groups), dim3(64), 0, h->stream, h->T, h->R, h->EC, h->slab, h->B,
                     seeds ? h->d_seeds : (const uint64_t*)nullptr, mask ? h->d_mask : (const uint8_t*)nullptr);
  HIPCHK(h, hipGetLastError());
  h->was_reset = true;
  if (h->comm_stream) HIPCHK(h, hipStreamSynchronize(h->comm_stream));       // no gather may still be reading an observation buffer
  h->gather_pending[0] = h->gather_pending[1] = false; h->obs_cur = 0;
  int rc = launch_pack_obs(h, h->d_obs2[0]);   // every column, the constants included
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(h->d_obs2[1], h->d_obs2[0], (size_t)h->B * h->obs_dim * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  if (obs_out) HIPCHK(h, hipMemcpyAsync(obs_out, h->d_obs2[0], (size_t)h->B * h->obs_dim * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

int gs_host_alloc(void** out, size_t bytes) {
  if (!out || bytes == 0) return fail(nullptr, GS_E_INVALID, "gs_host_alloc: out is NULL or bytes == 0");
  *out = nullptr;
  if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return fail(nullptr, GS_E_NOMEM, "hipHostMalloc(%zu bytes) failed", bytes);
  }
  return GS_OK;
}

int gs_host_free(void* p) {
  if (!p) return GS_OK;
  if (hipHostFree(p) != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, GS_E_INVALID, "gs_host_free: not a gs_host_alloc pointer"); }
  return GS_OK;
}

// obs32: the observation block rounded to float32 (the dtype the reference DECLARES for its observation space, grid_env.py:346; its
// values are Python floats) -- converted on the device, 22 MB instead of 45 over the link at [8192][684]
static int download_step_impl(gs_handle* h, double* obs, float* obs32, double* reward, uint8_t* terminated, uint8_t* truncated,
                              const gs_info_view* info) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  GS_ENTER(h);
  if (obs32) {
    if (!h->d_obs32) { int rc0 = dev_alloc(h, &h->d_obs32, (size_t)h->Bp * h->obs_dim); if (rc0) return rc0; }
    if (!h->ev_scalars) HIPCHK(h, hipEventCreateWithFlags(&h->ev_scalars, hipEventDisableTiming));
    int rc = fetch_scalars(h, false);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(h->ev_scalars, h->stream));
    const long long n = (long long)h->B * h->obs_dim;
    hipLaunchKernelGGL(gs_k_obs_to_f32, dim3((unsigned)((n + 2 * 256 - 1) / (2 * 256))), dim3(256), 0, h->stream, h->d_obs2[h->obs_cur], h->d_obs32, n);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(obs32, h->d_obs32, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev_scalars));
    copy_info(h, reward, terminated, truncated, info);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return GS_OK;
  }
  if (!obs) {
    int rc = fetch_scalars(h);
    if (rc) return rc;
    copy_info(h, reward, terminated, truncated, info);
    return GS_OK;
  }
  // the scalars first (half a megabyte the kernel stores into the handle's page-locked block itself), then the observation block
  // behind them: the caller's reward / flag / info arrays are filled while the block is still crossing the link
  if (!h->ev_scalars) HIPCHK(h, hipEventCreateWithFlags(&h->ev_scalars, hipEventDisableTiming));
  int rc = fetch_scalars(h, false);
  if (rc) return rc;
  HIPCHK(h, hipEventRecord(h->ev_scalars, h->stream));
  const double* src = h->d_obs2[h->obs_cur];
  const size_t D = (size_t)h->obs_dim, pitch = D * sizeof(double), s0 = (size_t)h->obs_skip0, s1 = (size_t)h->obs_skip1, B = (size_t)h->B;
  const bool bound = s1 > s0 && std::find(h->bound_obs.begin(), h->bound_obs.end(), obs) != h->bound_obs.end();
  if (bound) {
    // The constants are in place (gs_host_obs_bind).  What changes is, in memory order, ONE run per row boundary: the columns of row r
    // behind the constant block and those of row r + 1 in front of it -- a single pitched copy of B - 1 runs of obs_dim - (skip1 -
    // skip0) doubles, plus the head of row 0 and the tail of row B - 1.  Measured at B = 8192 on the 123-bus feeder, per env.step():
    // this 0.78 ms; a kernel storing the same columns into the mapped array 0.82 ms (its stores cross the link 64 bytes at a time);
    // two pitched copies, one either side of the constants, 1.00 ms; the whole block 1.10 ms.
    if (s0 > 0) HIPCHK(h, hipMemcpyAsync(obs, src, s0 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (B > 1)
      HIPCHK(h, hipMemcpy2DAsync(obs + s1, pitch, src + s1, pitch, (D - (s1 - s0)) * sizeof(double), B - 1, hipMemcpyDeviceToHost, h->stream));
    if (D > s1)
      HIPCHK(h, hipMemcpyAsync(obs + (B - 1) * D + s1, src + (B - 1) * D + s1, (D - s1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  } else {
    HIPCHK(h, hipMemcpyAsync(obs, src, B * pitch, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipEventSynchronize(h->ev_scalars));
  copy_info(h, reward, terminated, truncated, info);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GS_OK;
}

int gs_download_step(gs_handle* h, double* obs, double* reward, uint8_t* terminated, uint8_t* truncated, const gs_info_view* info) {
  return download_step_impl(h, obs, nullptr, reward, terminated, truncated, info);
}

int gs_download_step_f32(gs_handle* h, float* obs, double* reward, uint8_t* terminated, uint8_t* truncated, const gs_info_view* info) {
  if (!obs) return fail(h, GS_E_INVALID, "gs_download_step_f32: obs is NULL");
  return download_step_impl(h, nullptr, obs, reward, terminated, truncated, info);
}

// A host observation array [B][obs_dim] the caller will hand to gs_step / gs_download_step again and again: its constant columns
// (the static load powers, grid_env.py:769-770 -- they never change) are written here, once, and later downloads into the same
// address move the changing columns only.  The caller must leave those columns alone (or bind again).
int gs_host_obs_bind(gs_handle* h, double* obs) {
  if (!h || !obs) return fail(h, GS_E_INVALID, "handle / obs is NULL");
  if (!h->was_reset) return fail(h, GS_E_STATE, "gs_host_obs_bind before gs_reset");
  GS_ENTER(h);
  if (h->obs_skip1 > h->obs_skip0) {
    const size_t pitch = (size_t)h->obs_dim * sizeof(double);
    HIPCHK(h, hipMemcpy2DAsync(obs + h->obs_skip0, pitch, h->d_obs2[h->obs_cur] + h->obs_skip0, pitch, (size_t)(h->obs_skip1 - h->obs_skip0) * sizeof(double),
                               (size_t)h->B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  if (std::find(h->bound_obs.begin(), h->bound_obs.end(), obs) == h->bound_obs.end()) h->bound_obs.push_back(obs);
  return GS_OK;
}

int gs_host_obs_unbind(gs_handle* h, double* obs) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  auto it = std::find(h->bound_obs.begin(), h->bound_obs.end(), (const double*)obs);
  if (it != h->bound_obs.end()) h->bound_obs.erase(it);
  return GS_OK;
}

int gs_step(gs_handle* h, const double* actions, double* obs, double* reward, uint8_t* terminated,
            uint8_t* truncated, const gs_info_view* info) {
  if (!h || (!actions && h->action_dim > 0)) return fail(h, GS_E_INVALID, "handle / actions is NULL");
  if (!h->was_reset) return fail(h, GS_E_STATE, "gs_step before gs_reset");
  GS_ENTER(h);
  if (h->action_dim > 0)
    HIPCHK(h, hipMemcpyAsync(h->d_in, actions, (size_t)h->B * h->action_dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
  int rc = step_kernels(h, h->d_in);
  if (rc) return rc;
  return gs_download_step(h, obs, reward, terminated, truncated, info);
}

int gs_step_f32(gs_handle* h, const double* actions, float* obs, double* reward, uint8_t* terminated, uint8_t* truncated,
                const gs_info_view* info) {
  if (!h || (!actions && h->action_dim > 0) || !obs) return fail(h, GS_E_INVALID, "handle / actions / obs is NULL");
  if (!h->was_reset) return fail(h, GS_E_STATE, "gs_step_f32 before gs_reset");
  GS_ENTER(h);
  if (h->action_dim > 0)
    HIPCHK(h, hipMemcpyAsync(h->d_in, actions, (size_t)h->B * h->action_dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
  int rc = step_kernels(h, h->d_in);
  if (rc) return rc;
  return download_step_impl(h, nullptr, obs, reward, terminated, truncated, info);
}

int gs_step_device_ptr(gs_handle* h, const double* d_actions, void* producer_stream) {
  if (!h || (!d_actions && h->action_dim > 0)) return fail(h, GS_E_INVALID, "handle / d_actions is NULL");
  if (!h->was_reset) return fail(h, GS_E_STATE, "gs_step_device_ptr before gs_reset");
  HIPCHK(h, hipSetDevice(h->device));
  if (producer_stream) {             // the step waits, on the device, for what the producer has queued so far
    if (!h->ev_peer) HIPCHK(h, hipEventCreateWithFlags(&h->ev_peer, hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(h->ev_peer, peer_stream(producer_stream)));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_peer, 0));
    if (h->forked) HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_peer, 0));
  }
  return step_kernels(h, d_actions);
}

int gs_step_device_view(gs_handle* h, gs_step_device_out* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  if (!h->was_reset) return fail(h, GS_E_STATE, "gs_step_device_view before gs_reset");
  GS_ENTER(h);
  hipLaunchKernelGGL(gs_k_scalars, dim3(h->groups), dim3(64), 0, h->stream, h->rows_f, (int)SF_COUNT, h->rows_i,
                     (int)SI_COUNT, h->rows_u, (int)SU_COUNT, h->R.total, h->slab, h->sc_f, h->sc_i, h->sc_u, h->Bp, (uint32_t*)nullptr, 0);
  HIPCHK(h, hipGetLastError());
  if (consumer_stream) {
    if (!h->ev_peer2) HIPCHK(h, hipEventCreateWithFlags(&h->ev_peer2, hipEventDisableTiming));
    HIPCHK(h, hipEventRecord(h->ev_peer2, h->stream));
    HIPCHK(h, hipStreamWaitEvent(peer_stream(consumer_stream), h->ev_peer2, 0));
  } else {
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  out->observations = h->d_obs2[h->obs_cur];
  out->reward = h->sc_f + (size_t)SF_REWARD * h->Bp;
  out->terminated = h->sc_u + (size_t)SU_TERM * h->Bp;
  out->truncated = h->sc_u + (size_t)SU_TRUNC * h->Bp;
  out->B = h->B; out->obs_dim = h->obs_dim;
  return GS_OK;
}

int gs_upload_actions(gs_handle* h, const double* actions, int32_t n_batches) {
  if (!h || !actions || n_batches <= 0) return fail(h, GS_E_INVALID, "bad arguments");
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->d_actions) { (void)hipFree(h->d_actions); h->d_actions = nullptr; }
  const size_t bytes = (size_t)n_batches * h->B * std::max(h->action_dim, 1) * sizeof(double);
  HIPCHK(h, hipMalloc((void**)&h->d_actions, bytes));
  HIPCHK(h, hipMemcpy(h->d_actions, actions, (size_t)n_batches * h->B * h->action_dim * sizeof(double), hipMemcpyHostToDevice));
  h->n_action_batches = n_batches;
  return GS_OK;
}

int gs_step_device(gs_handle* h, int32_t k) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (!h->was_reset) return fail(h, GS_E_STATE, "gs_step_device before gs_reset");
  if (k < 0 || k >= h->n_action_batches) return fail(h, GS_E_INVALID, "action batch %d not uploaded (have %d)", k, h->n_action_batches);
  HIPCHK(h, hipSetDevice(h->device));
  return step_kernels(h, h->d_actions + (size_t)k * h->B * h->action_dim);
}


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
  if (pol.blob) { (void)hipFree(pol.blob); pol.blob = nullptr; }
  pol.set = false;
  if (!p) return GS_OK;
  if (!pol.act) HIPCHK(h, hipMalloc((void**)&pol.act, (size_t)h->B * h->action_dim * sizeof(double)));
  if (gs_policy_is_f32(o)) {
    const GsPolicyImageF32 im = gs_policy_pack_f32(*p, *o);
    pol.lds32 = gs_pol32_lds_bytes(im.kb[0]);
    HIPCHK(h, hipFuncSetAttribute((const void*)gs_k_policy_mlp_f32, hipFuncAttributeMaxDynamicSharedMemorySize, pol.lds32));
    // one allocation: the float image (a multiple of 16 floats), then shift and scale
    const size_t image_bytes = im.blob.size() * sizeof(float), norm_bytes = im.norm.size() * sizeof(double);
    HIPCHK(h, hipMalloc((void**)&pol.blob, image_bytes + norm_bytes));
    const float* image = (const float*)pol.blob;
    const double* norm = (const double*)((const char*)pol.blob + image_bytes);
    HIPCHK(h, hipMemcpy((void*)image, im.blob.data(), image_bytes, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy((void*)norm, im.norm.data(), norm_bytes, hipMemcpyHostToDevice));
    GsPolicyArgsF32& a = pol.args32;
    a = GsPolicyArgsF32{};
    a.shift = norm; a.scale = norm + 16 * im.kb[0];
    a.B = h->B; a.D = h->obs_dim; a.A = h->action_dim; a.n_layers = p->n_layers; a.activation = p->activation; a.head = p->head;
    a.stochastic = p->stochastic; a.first_instance = h->EC.first_instance; a.obs_stride = gs_pol32_obs_stride(im.kb[0]);
    for (int l = 0; l < p->n_layers; ++l) a.L[l] = GsPolicyLayerF32{image + im.w_off[l], image + im.b_off[l], im.kb[l], im.nt[l]};
    pol.compute = GS_COMPUTE_F32;
    pol.set = true;
    return GS_OK;
  }
  const GsPolicyImage im = gs_policy_pack(*p);
  HIPCHK(h, hipFuncSetAttribute((const void*)gs_k_policy_mlp, hipFuncAttributeMaxDynamicSharedMemorySize, GS_POL_LDS_BYTES));
  HIPCHK(h, hipMalloc((void**)&pol.blob, im.blob.size() * sizeof(double)));
  HIPCHK(h, hipMemcpy(pol.blob, im.blob.data(), im.blob.size() * sizeof(double), hipMemcpyHostToDevice));
  GsPolicyArgs& a = pol.args;
  a = GsPolicyArgs{};
  a.B = h->B; a.D = h->obs_dim; a.A = h->action_dim; a.n_layers = p->n_layers; a.activation = p->activation; a.head = p->head;
  a.stochastic = p->stochastic; a.first_instance = h->EC.first_instance;
  for (int l = 0; l < p->n_layers; ++l) a.L[l] = GsPolicyLayer{pol.blob + im.w_off[l], pol.blob + im.b_off[l], im.kb[l], im.nt[l]};
  pol.compute = GS_COMPUTE_F64;
  pol.set = true;
  return GS_OK;
}

// one launch: actions[B][A] of the installed policy on obs[B][obs_dim] (device pointers), on the handle's main stream
static int launch_policy(gs_handle* h, const double* obs, double* act, uint64_t seed, int t) {
  const dim3 grid((unsigned)((h->B + GS_POL_ROWS - 1) / GS_POL_ROWS)), block(64 * GS_POL_WAVES);
  if (h->pol.compute == GS_COMPUTE_F32) {
    GsPolicyArgsF32 a = h->pol.args32;
    a.obs = obs; a.act = act; a.seed = seed; a.t = t;
    hipLaunchKernelGGL(gs_k_policy_mlp_f32, grid, block, h->pol.lds32, h->stream, a);
  } else {
    GsPolicyArgs a = h->pol.args;
    a.obs = obs; a.act = act; a.seed = seed; a.t = t;
    hipLaunchKernelGGL(gs_k_policy_mlp, grid, block, GS_POL_LDS_BYTES, h->stream, a);
  }
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

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


// ---- device-resident rollout collection ---------------------------------------------------------------
// T fused env steps back to back, nothing on the host in between (algorithms/base.py:268-298, batched).
// Device layout (gs_rollout_device_view): obs_seq[T + 1][B][obs_dim] -- slot t is what step t started from, slot
// t + 1 is written by step t's kernel itself (its observation output IS the next slot: no copy) --, act[T][B][A],
// rew[T][B], done[T][B], and the side list of terminal observations (t, b, row) the in-place resets replaced.
static int rollout_ensure(gs_handle* h, int T) {
  gs_handle::Rollout& ro = h->ro;
  if (T <= ro.T_cap) return GS_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (void* p : {(void*)ro.obs_seq, (void*)ro.act, (void*)ro.rew, (void*)ro.done, (void*)ro.term_idx, (void*)ro.term_obs})
    if (p) (void)hipFree(p);
  ro.obs_seq = nullptr; ro.act = nullptr; ro.rew = nullptr; ro.done = nullptr; ro.term_idx = nullptr; ro.term_obs = nullptr; ro.T_cap = 0;
  const size_t B = h->B, D = h->obs_dim, A = std::max(h->action_dim, 1);
  // an instance finishes at most once per min(episode_length, 11) steps (truncation needs more than 10 violating steps
  // since its last reset, grid_env.py:604) plus once for an episode that was already under way
  const int min_ep = std::max(1, std::min(h->cfg.episode_length, 11));
  const size_t cap = B * ((size_t)T / min_ep + 1);
  if (!ro.term_count) HIPCHK(h, hipMalloc((void**)&ro.term_count, sizeof(int32_t)));
  if (hipMalloc((void**)&ro.obs_seq, (size_t)(T + 1) * B * D * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&ro.act, (size_t)T * B * A * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&ro.rew, (size_t)T * B * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&ro.done, (size_t)T * B) != hipSuccess ||
      hipMalloc((void**)&ro.term_idx, cap * 2 * sizeof(int32_t)) != hipSuccess ||
      hipMalloc((void**)&ro.term_obs, cap * D * sizeof(double)) != hipSuccess)
    return fail(h, GS_E_NOMEM, "rollout buffers for T = %d (%.1f MB per step) do not fit", T, (double)B * D * 8e-6);
  ro.T_cap = T; ro.term_cap = (int)std::min<size_t>(cap, 0x7fffffff);
  // the constant columns of every slot, once: the step kernels write only the columns that change
  const long long rows = (long long)(T + 1) * B;
  const int w = h->obs_skip1 - h->obs_skip0;
  if (w > 0) {
    const long long total = rows * w;
    hipLaunchKernelGGL(gs_k_fill_const_columns, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, ro.obs_seq, rows,
                       h->obs_dim, h->obs_skip0, h->obs_skip1, h->map_obs, h->d_cst);
    HIPCHK(h, hipGetLastError());
  }
  return GS_OK;
}

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
  const size_t B = h->B, D = h->obs_dim, A = h->action_dim;
  ro.T = T; ro.n_term = -1;
  HIPCHK(h, hipMemsetAsync(ro.term_count, 0, sizeof(int32_t), h->stream));
  if (A > 0) {
    if (policy == GS_POLICY_UPLOADED) {
      HIPCHK(h, hipMemcpyAsync(ro.act, actions, (size_t)T * B * A * sizeof(double), hipMemcpyHostToDevice, h->stream));
    } else if (policy == GS_POLICY_RANDOM) {
      const long long total = (long long)T * B * ((A + 3) / 4);
      hipLaunchKernelGGL(gs_k_rollout_actions, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, ro.act, (int)T, (int)B, (int)A,
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
    if (policy == GS_POLICY_MLP && (rc = launch_policy(h, ro.obs_seq + (size_t)t * B * D, ro.act + (size_t)t * B * A, policy_seed, t))) return rc;
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
  return GS_OK;      // asynchronous: gs_synchronize / gs_rollout_download / gs_rollout_device_view wait for it
}

static int rollout_finish(gs_handle* h) {
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

// ---- checkpoint ---------------------------------------------------------------------------------
int gs_get_state(gs_handle* h, double* state) {
  if (!h || !state) return fail(h, GS_E_INVALID, "handle / state is NULL");
  GS_ENTER(h);
  int rc = ensure_rows(h);
  if (rc) return rc;
  return pack_to_host(h, h->map_state, h->state_dim, state);
}

int gs_set_state(gs_handle* h, const double* state) {
  if (!h || !state) return fail(h, GS_E_INVALID, "handle / state is NULL");
  GS_ENTER(h);
  h->rows_stale = false;            // the checkpoint carries every result row
  int rc = unpack_from_host(h, h->map_state, h->state_dim, state);
  if (rc) return rc;
  // rows that follow from the checkpoint: the rectangular voltages (what a warm-started sweep solver resumes from) and
  // the uncurtailed renewable powers of the observation
  hipLaunchKernelGGL(gs_k_polar_to_rect, dim3(h->groups), dim3(64), 0, h->stream, h->T, h->R, h->slab, h->B);
  HIPCHK(h, hipGetLastError());
  // both observation buffers whole, as gs_reset leaves them: the step kernel never writes the constant columns, so a
  // handle that is restored without ever having been reset (resume in a new process) must get them here
  if (h->comm_stream) HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  h->gather_pending[0] = h->gather_pending[1] = false;
  if ((rc = launch_pack_obs(h, h->d_obs2[h->obs_cur]))) return rc;
  HIPCHK(h, hipMemcpyAsync(h->d_obs2[h->obs_cur ^ 1], h->d_obs2[h->obs_cur], (size_t)h->B * h->obs_dim * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->was_reset = true;
  return GS_OK;
}

// ---- multi-GPU ------------------------------------------------------------------------------------
int gs_comm_unique_id(uint8_t id_out[128]) {
  std::string why;
  if (!load_rccl(why)) return fail(nullptr, GS_E_COMM, "%s", why.c_str());
  gs_ncclUniqueId id;
  int rc = g_rccl.GetUniqueId(&id);
  if (rc != 0) return fail(nullptr, GS_E_COMM, "ncclGetUniqueId: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
  memcpy(id_out, id.internal, 128);
  return GS_OK;
}

// What both transports need on a member: the gathered block [world * B][obs_dim] with its constant columns in place,
// the compact send / receive blocks, the exchange stream and its events.
static int comm_buffers(gs_handle* h, int rank, int world_size) {
  h->rank = rank; h->world = world_size;
  HIPCHK(h, hipMalloc((void**)&h->d_obs_full, (size_t)world_size * h->B * h->obs_dim * sizeof(double)));
  const int nd = h->obs_dim - (h->obs_skip1 - h->obs_skip0);
  HIPCHK(h, hipMalloc((void**)&h->d_gather_send, (size_t)h->B * nd * sizeof(double)));
  HIPCHK(h, hipMalloc((void**)&h->d_gather_recv, (size_t)world_size * h->B * nd * sizeof(double)));
  if (!h->comm_stream) {
    HIPCHK(h, hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_step, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_full, hipEventDisableTiming));
    for (int k = 0; k < 2; ++k) HIPCHK(h, hipEventCreateWithFlags(&h->ev_gather[k], hipEventDisableTiming));
  }
  // the constant columns of the gathered block do not depend on the rank (static load powers of the shared feeder):
  // written here once, never sent
  if (h->obs_skip1 > h->obs_skip0) {
    const long long rows = (long long)world_size * h->B, total = rows * (h->obs_skip1 - h->obs_skip0);
    hipLaunchKernelGGL(gs_k_fill_const_columns, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->comm_stream, h->d_obs_full, rows,
                       h->obs_dim, h->obs_skip0, h->obs_skip1, h->map_obs, h->d_cst);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  }
  return GS_OK;
}

int gs_comm_init(gs_handle* h, const uint8_t id[128], int32_t rank, int32_t world_size) {
  if (!h || !id || world_size < 1 || rank < 0 || rank >= world_size) return fail(h, GS_E_INVALID, "bad arguments");
  if (h->comm || h->loop) return fail(h, GS_E_STATE, "the handle already belongs to a communicator");
  std::string why;
  if (!load_rccl(why)) return fail(h, GS_E_COMM, "%s", why.c_str());
  GS_ENTER(h);
  gs_ncclUniqueId uid; memcpy(uid.internal, id, 128);
  int rc = g_rccl.CommInitRank(&h->comm, world_size, uid, rank);
  if (rc != 0) return fail(h, GS_E_COMM, "ncclCommInitRank: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
  return comm_buffers(h, rank, world_size);
}

// ---- the in-process transport ----------------------------------------------------------------------
// `world` handles of ONE process form the communicator; rank r's compact block reaches rank q by a device-to-device
// copy on q's exchange stream where RCCL would move it over xGMI.  Everything either side of that copy -- compaction,
// slot offsets, expansion into [world * B][obs_dim], constant columns, the double-buffered observation buffers and
// their events -- is the code the RCCL transport runs.  The collective completes when the last member has called
// (the semantics of a grouped RCCL call): that call queues every member's copies.
struct GsLoopComm {
  int world = 0, n_live = 0, n_arrived = 0;
  std::vector<gs_handle*> member;
  std::vector<hipEvent_t> ev_sent;      // rank r's send block is complete (recorded on r's exchange stream)
  std::vector<hipEvent_t> ev_taken;     // rank r has copied every send block of the round (before anyone refills one)
  std::vector<uint8_t> arrived, taken_valid;
  std::vector<double*> host_out;
};

static int loop_complete_body(GsLoopComm* lc) {
  const gs_handle* h0 = lc->member[0];
  const int D = h0->obs_dim, nd = D - (h0->obs_skip1 - h0->obs_skip0);
  const size_t count = (size_t)h0->B * nd;
  for (int r = 0; r < lc->world; ++r) {
    gs_handle* q = lc->member[r];
    HIPCHK(q, hipSetDevice(q->device));
    for (int p = 0; p < lc->world; ++p) {
      if (p != r) HIPCHK(q, hipStreamWaitEvent(q->comm_stream, lc->ev_sent[p], 0));
      HIPCHK(q, hipMemcpyAsync(q->d_gather_recv + (size_t)p * count, lc->member[p]->d_gather_send, count * sizeof(double),
                               hipMemcpyDeviceToDevice, q->comm_stream));
    }
    HIPCHK(q, hipEventRecord(lc->ev_taken[r], q->comm_stream));
    lc->taken_valid[r] = 1;
    const size_t total = count * lc->world;
    hipLaunchKernelGGL(gs_k_obs_compact, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, q->comm_stream, q->d_gather_recv, q->d_obs_full,
                       (long long)lc->world * q->B, D, q->obs_skip0, q->obs_skip1, 1);
    HIPCHK(q, hipGetLastError());
    if (lc->host_out[r])
      HIPCHK(q, hipMemcpyAsync(lc->host_out[r], q->d_obs_full, (size_t)q->B * D * lc->world * sizeof(double), hipMemcpyDeviceToHost, q->comm_stream));
  }
  for (int r = 0; r < lc->world; ++r)
    if (lc->host_out[r]) HIPCHK(lc->member[r], hipStreamSynchronize(lc->member[r]->comm_stream));
  return GS_OK;
}

// The round ends here whether or not it succeeded: a failed round leaves no member "arrived" and keeps no pointer into
// the callers' memory, so that the next call reports its own error (or works) instead of "called twice" / "gather half-way".
static int loop_complete(GsLoopComm* lc) {
  const int rc = loop_complete_body(lc);
  if (rc)       // copies of the failed round may still be queued towards the callers' host arrays: drain before letting go of them
    for (int r = 0; r < lc->world; ++r)
      if (lc->host_out[r] && lc->member[r] && lc->member[r]->comm_stream) { (void)hipSetDevice(lc->member[r]->device); (void)hipStreamSynchronize(lc->member[r]->comm_stream); }
  for (int r = 0; r < lc->world; ++r) { lc->host_out[r] = nullptr; lc->arrived[r] = 0; }
  lc->n_arrived = 0;
  return rc;
}

int gs_comm_init_loopback(gs_handle* const* shards, int32_t nshards) {
  if (!shards || nshards < 1) return fail(nullptr, GS_E_INVALID, "bad arguments");
  for (int r = 0; r < nshards; ++r) {
    gs_handle* h = shards[r];
    if (!h) return fail(nullptr, GS_E_INVALID, "shard %d is NULL", r);
    if (h->comm || h->loop) return fail(h, GS_E_STATE, "shard %d already belongs to a communicator", r);
    if (h->B != shards[0]->B || h->obs_dim != shards[0]->obs_dim || h->obs_skip0 != shards[0]->obs_skip0 || h->obs_skip1 != shards[0]->obs_skip1)
      return fail(h, GS_E_INVALID, "shard %d: batch / observation layout differs from shard 0 (the all-gather needs equal shards)", r);
    for (int q = 0; q < r; ++q) if (shards[q] == h) return fail(h, GS_E_INVALID, "shard %d is shard %d again", r, q);
  }
  GsLoopComm* lc = new GsLoopComm();
  lc->world = lc->n_live = nshards;
  lc->member.assign(shards, shards + nshards);
  lc->ev_sent.assign(nshards, nullptr); lc->ev_taken.assign(nshards, nullptr);
  lc->arrived.assign(nshards, 0); lc->taken_valid.assign(nshards, 0); lc->host_out.assign(nshards, nullptr);
  for (int r = 0; r < nshards; ++r) {
    gs_handle* h = shards[r];
    int rc = GS_OK;
    do {
      hipError_t e = hipSetDevice(h->device);
      if (e == hipSuccess && h->forked) { rc = join_streams(h); if (rc) break; }
      if (e == hipSuccess) e = hipEventCreateWithFlags(&lc->ev_sent[r], hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&lc->ev_taken[r], hipEventDisableTiming);
      if (e != hipSuccess) { rc = fail(h, GS_E_HIP, "loopback communicator set-up failed: %s", hipGetErrorString(e)); break; }
      rc = comm_buffers(h, r, nshards);
    } while (0);
    if (rc) {       // undo: members attached so far go back to "no communicator"
      for (int q = 0; q <= r; ++q) { shards[q]->loop = nullptr; (void)gs_comm_destroy(shards[q]); }
      for (int q = 0; q < nshards; ++q) { if (lc->ev_sent[q]) (void)hipEventDestroy(lc->ev_sent[q]); if (lc->ev_taken[q]) (void)hipEventDestroy(lc->ev_taken[q]); }
      delete lc;
      return rc;
    }
    h->loop = lc;
  }
  return GS_OK;
}

// The exchange of one member in three parts, so that a process driving several members through RCCL can put ONLY the
// collectives between ncclGroupStart and ncclGroupEnd: inside a group ncclAllGather merely records the call, the work is
// enqueued on the exchange stream at ncclGroupEnd -- anything launched on that stream in between (the expansion, a
// download) would run BEFORE the collective and see the previous round's block.
//   gather_prepare     behind the step that produced the current observation buffer: compact its changing columns
//   gather_collective  ncclAllGather of the compact blocks (RCCL transport only)
//   gather_finish      expand into [world * B][obs_dim]; optional download
static int gather_prepare(gs_handle* h) {
  GsLoopComm* lc = h->loop;
  const int D = h->obs_dim, nd = D - (h->obs_skip1 - h->obs_skip0);
  const size_t count = (size_t)h->B * nd;
  // On its own stream, behind the step that produced the current observation buffer.  Only the columns that change
  // travel: the block is compacted first (which is also all the gather needs of the observation buffer -- the step
  // after the next one, which reuses that buffer, waits for ev_gather = the end of the compaction, not of the gather),
  // the compact blocks are gathered over xGMI, and expanded into the [world * B][obs_dim] block.
  const int cur = h->obs_cur;
  HIPCHK(h, hipEventRecord(h->ev_step, h->stream));
  HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->ev_step, 0));
  if (lc)       // loopback only: the peers copy OUT of this send block on their own streams (RCCL reads it on this one)
    for (int r = 0; r < lc->world; ++r)
      if (r != h->rank && lc->taken_valid[r]) HIPCHK(h, hipStreamWaitEvent(h->comm_stream, lc->ev_taken[r], 0));
  hipLaunchKernelGGL(gs_k_obs_compact, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->comm_stream, h->d_obs2[cur], h->d_gather_send,
                     (long long)h->B, D, h->obs_skip0, h->obs_skip1, 0);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev_gather[cur], h->comm_stream));
  h->gather_pending[cur] = true;
  return GS_OK;
}

static int gather_collective(gs_handle* h) {
  const size_t count = (size_t)h->B * (h->obs_dim - (h->obs_skip1 - h->obs_skip0));
  const int rc = g_rccl.AllGather(h->d_gather_send, h->d_gather_recv, count, /*ncclFloat64*/ 8, h->comm, h->comm_stream);
  if (rc != 0) return fail(h, GS_E_COMM, "ncclAllGather: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
  return GS_OK;
}

static int gather_finish(gs_handle* h, double* obs_full_host) {
  const int D = h->obs_dim;
  const size_t total = (size_t)h->B * (D - (h->obs_skip1 - h->obs_skip0)) * h->world;
  hipLaunchKernelGGL(gs_k_obs_compact, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->comm_stream, h->d_gather_recv, h->d_obs_full,
                     (long long)h->world * h->B, D, h->obs_skip0, h->obs_skip1, 1);
  HIPCHK(h, hipGetLastError());
  if (obs_full_host) {
    HIPCHK(h, hipMemcpyAsync(obs_full_host, h->d_obs_full, (size_t)h->B * D * h->world * sizeof(double), hipMemcpyDeviceToHost, h->comm_stream));
    HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  }
  return GS_OK;
}

int gs_allgather_obs(gs_handle* h, double* obs_full_host) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (!h->comm && !h->loop) return fail(h, GS_E_STATE, "gs_allgather_obs before gs_comm_init / gs_comm_init_loopback");
  GsLoopComm* lc = h->loop;
  if (lc && lc->n_live != lc->world) return fail(h, GS_E_STATE, "a member of the loopback communicator has left");
  if (lc && lc->arrived[h->rank]) return fail(h, GS_E_STATE, "rank %d called gs_allgather_obs twice before every member had called once", h->rank);
  GS_ENTER(h);
  int rc = gather_prepare(h);
  if (rc) return rc;
  if (lc) {
    HIPCHK(h, hipEventRecord(lc->ev_sent[h->rank], h->comm_stream));
    lc->arrived[h->rank] = 1; lc->host_out[h->rank] = obs_full_host;
    if (++lc->n_arrived == lc->world) return loop_complete(lc);
    return GS_OK;
  }
  if ((rc = gather_collective(h))) return rc;
  return gather_finish(h, obs_full_host);
}

int gs_allgather_obs_shards(gs_handle* const* shards, int32_t nshards, double* obs_full_host) {
  if (!shards || nshards < 1 || !shards[0]) return fail(nullptr, GS_E_INVALID, "bad arguments");
  GsLoopComm* lc = shards[0]->loop;
  for (int r = 0; r < nshards; ++r) {
    if (!shards[r]) return fail(nullptr, GS_E_INVALID, "shard %d is NULL", r);
    if (shards[r]->loop != lc || (!lc && !shards[r]->comm)) return fail(shards[r], GS_E_STATE, "shard %d is not in the communicator of shard 0", r);
  }
  if (lc && (nshards != lc->world || lc->n_arrived != 0)) return fail(shards[0], GS_E_STATE, "the call must name every member of the loopback communicator once, with no gather half-way");
  if (!lc) {      // one process driving several GPUs through RCCL: the members' collectives form one group (see gather_prepare)
    if (!g_rccl.GroupStart || !g_rccl.GroupEnd) return fail(shards[0], GS_E_COMM, "librccl lacks ncclGroupStart / ncclGroupEnd");
    int rc = GS_OK;
    for (int r = 0; r < nshards; ++r) {
      gs_handle* h = shards[r];
      GS_ENTER(h);
      if ((rc = gather_prepare(h))) return rc;
    }
    g_rccl.GroupStart();
    for (int r = 0; r < nshards && !rc; ++r) {
      if (hipSetDevice(shards[r]->device) != hipSuccess) rc = fail(shards[r], GS_E_HIP, "hipSetDevice failed");
      else rc = gather_collective(shards[r]);
    }
    const int rg = g_rccl.GroupEnd();          // (always closed, also after a failed call inside the group)
    if (rc) return rc;
    if (rg != 0) return fail(shards[0], GS_E_COMM, "ncclGroupEnd: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rg) : "error");
    for (int r = 0; r < nshards; ++r) {
      HIPCHK(shards[r], hipSetDevice(shards[r]->device));
      if ((rc = gather_finish(shards[r], r == 0 ? obs_full_host : nullptr))) return rc;
    }
    return GS_OK;
  }
  for (int r = 0; r < nshards; ++r) {
    int rc = gs_allgather_obs(shards[r], r == 0 ? obs_full_host : nullptr);
    if (rc) return rc;
  }
  return GS_OK;
}

int gs_allgather_obs_view(gs_handle* h, gs_gathered_obs* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  if (!h->d_obs_full) return fail(h, GS_E_STATE, "no communicator on this handle");
  if (h->loop && h->loop->arrived[h->rank]) return fail(h, GS_E_STATE, "the gather of this round is not complete: not every member has called gs_allgather_obs");
  HIPCHK(h, hipSetDevice(h->device));
  if (consumer_stream) {
    HIPCHK(h, hipEventRecord(h->ev_full, h->comm_stream));
    HIPCHK(h, hipStreamWaitEvent(peer_stream(consumer_stream), h->ev_full, 0));
  } else {
    HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  }
  out->observations = h->d_obs_full; out->rows = (int64_t)h->world * h->B; out->obs_dim = h->obs_dim;
  out->rank = h->rank; out->world = h->world; out->reserved = 0;
  return GS_OK;
}

int gs_allgather_obs_download(gs_handle* h, double* obs_full_host) {
  if (!h || !obs_full_host) return fail(h, GS_E_INVALID, "handle / obs_full_host is NULL");
  gs_gathered_obs v;
  int rc = gs_allgather_obs_view(h, &v, nullptr);
  if (rc) return rc;
  HIPCHK(h, hipMemcpy(obs_full_host, v.observations, (size_t)v.rows * v.obs_dim * sizeof(double), hipMemcpyDeviceToHost));
  return GS_OK;
}

// What the communicator itself says about this member -- asked of RCCL (ncclCommCount / ncclCommUserRank /
// ncclCommCuDevice / ncclGetVersion), not echoed from the arguments of gs_comm_init --, and the device's UUID, so that a
// multi-rank run can show in its own output that N ranks on N different devices took part.
int gs_comm_info(gs_handle* h, gs_comm_info_t* out) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  if (!h->comm && !h->loop) return fail(h, GS_E_STATE, "no communicator on this handle");
  memset(out, 0, sizeof *out);
  out->transport = h->comm ? 1 : 2;
  out->device = h->device;
  hipUUID uu;
  if (hipDeviceGetUuid(&uu, h->device) == hipSuccess) memcpy(out->device_uuid, uu.bytes, 16);
  if (h->loop) { out->nranks = h->loop->world; out->rank = h->rank; out->comm_device = h->device; return GS_OK; }
  int v = 0;
  out->nranks = -1; out->rank = -1; out->comm_device = -1;
  if (g_rccl.CommCount && g_rccl.CommCount(h->comm, &v) == 0) out->nranks = v;
  if (g_rccl.CommUserRank && g_rccl.CommUserRank(h->comm, &v) == 0) out->rank = v;
  if (g_rccl.CommCuDevice && g_rccl.CommCuDevice(h->comm, &v) == 0) out->comm_device = v;
  if (g_rccl.GetVersion && g_rccl.GetVersion(&v) == 0) out->rccl_version = v;
  return GS_OK;
}

int gs_comm_destroy(gs_handle* h) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  (void)hipSetDevice(h->device);
  if (h->loop) {      // nobody may still be copying out of this member's send block
    GsLoopComm* lc = h->loop;
    for (gs_handle* q : lc->member)
      if (q && q->comm_stream) { (void)hipSetDevice(q->device); (void)hipStreamSynchronize(q->comm_stream); }
    (void)hipSetDevice(h->device);
    lc->member[h->rank] = nullptr; h->loop = nullptr;
    if (--lc->n_live == 0) {
      for (hipEvent_t e : lc->ev_sent) if (e) (void)hipEventDestroy(e);
      for (hipEvent_t e : lc->ev_taken) if (e) (void)hipEventDestroy(e);
      delete lc;
    }
  }
  if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
  h->gather_pending[0] = h->gather_pending[1] = false;
  if (h->comm && g_rccl.CommDestroy) { (void)hipStreamSynchronize(h->stream); g_rccl.CommDestroy(h->comm); h->comm = nullptr; }
  if (h->d_obs_full) { (void)hipFree(h->d_obs_full); h->d_obs_full = nullptr; }
  if (h->d_gather_send) { (void)hipFree(h->d_gather_send); h->d_gather_send = nullptr; }
  if (h->d_gather_recv) { (void)hipFree(h->d_gather_recv); h->d_gather_recv = nullptr; }
  h->rank = 0; h->world = 1;
  return GS_OK;
}

// ---- the meshed Newton-Raphson member's host schedule, without a device (mesh_schedule.h) -------------------------------
// header[0..15]: ok, n_levels, n_rows, max_rows_per_wave, n_pivots, msg_units, n_messages, n_accumulators, max_degree,
//                unit_bytes, zero_off, dummy_off, body_off, region_bytes, sizeof(GsMeshItem), n_adj;  why: the reason when ok == 0
int gs_mesh_schedule_dump(const gs_topology* topo, int32_t zero_z_mode, int32_t nw, int32_t ni, int32_t acc_cap, int32_t unit_budget, int32_t region_base,
                          int32_t slot_bytes, int32_t* header, char* why, int32_t why_cap, void* items, int32_t* rowinfo,
                          int32_t* adj_off, double* adj_y) {
  if (!topo || !header) return fail(nullptr, GS_E_INVALID, "topology / header is NULL");
  if (topo->struct_size != (int32_t)sizeof(gs_topology)) return fail(nullptr, GS_E_INVALID, "struct_size mismatch");
  if (nw < 1 || ni < 1 || acc_cap < 1) return fail(nullptr, GS_E_INVALID, "bad arguments");
  HostTopology ht;
  const std::string err = gs_compile_topology(*topo, zero_z_mode, false, true, ht);
  if (!err.empty()) return fail(nullptr, GS_E_INVALID, "topology: %s", err.c_str());
  MeshSchedule S;
  gs_mesh_schedule(ht, nw, ni, 8, region_base, slot_bytes, acc_cap, unit_budget, S);
  const int32_t hd[16] = {S.ok ? 1 : 0, S.n_levels, S.n_rows, S.max_rows_per_wave, S.n_pivots, S.msg_units, S.n_messages, S.n_accumulators,
                          S.max_degree, S.unit_bytes, S.zero_off, S.dummy_off, S.body_off, S.region_bytes, (int32_t)sizeof(GsMeshItem), (int32_t)S.adj_off.size()};
  memcpy(header, hd, sizeof hd);
  if (why && why_cap > 0) { strncpy(why, S.why.c_str(), (size_t)why_cap - 1); why[why_cap - 1] = 0; }
  if (!S.ok) return GS_OK;
  if (items) memcpy(items, S.items.data(), S.items.size() * sizeof(MeshItem));
  if (rowinfo) memcpy(rowinfo, S.rowinfo.data(), S.rowinfo.size() * sizeof(int32_t));
  if (adj_off) memcpy(adj_off, S.adj_off.data(), S.adj_off.size() * sizeof(int32_t));
  if (adj_y) memcpy(adj_y, S.adj_y.data(), S.adj_y.size() * sizeof(double));
  return GS_OK;
}

// The same schedule in the form the kernel reads (GS_MESH_W_*): counts[4] = n_pairs, ytab doubles, adj_ent entries, item words
int gs_mesh_schedule_dump_packed(const gs_topology* topo, int32_t zero_z_mode, int32_t nw, int32_t ni, int32_t acc_cap, int32_t unit_budget, int32_t region_base,
                                 int32_t slot_bytes, int32_t* counts, int32_t* packed, int32_t* rowinfo, double* ytab, int32_t* adj_ent) {
  if (!topo || !counts) return fail(nullptr, GS_E_INVALID, "topology / counts is NULL");
  if (topo->struct_size != (int32_t)sizeof(gs_topology)) return fail(nullptr, GS_E_INVALID, "struct_size mismatch");
  HostTopology ht;
  const std::string err = gs_compile_topology(*topo, zero_z_mode, false, true, ht);
  if (!err.empty()) return fail(nullptr, GS_E_INVALID, "topology: %s", err.c_str());
  MeshSchedule S;
  gs_mesh_schedule(ht, nw, ni, 8, region_base, slot_bytes, acc_cap, unit_budget, S);
  if (!S.ok) return fail(nullptr, GS_E_TOPOLOGY, "%s", S.why.c_str());
  counts[0] = S.n_pairs; counts[1] = (int32_t)S.ytab.size(); counts[2] = (int32_t)S.adj_ent.size(); counts[3] = GS_MESH_WORDS;
  if (packed) memcpy(packed, S.packed.data(), S.packed.size() * sizeof(int32_t));
  if (rowinfo) memcpy(rowinfo, S.rowinfo_packed.data(), S.rowinfo_packed.size() * sizeof(int32_t));
  if (ytab) memcpy(ytab, S.ytab.data(), S.ytab.size() * sizeof(double));
  if (adj_ent) memcpy(adj_ent, S.adj_ent.data(), S.adj_ent.size() * sizeof(int32_t));
  return GS_OK;
}

// The flat-start Newton map of the meshed member's iteration 0 (GsF2Tables::mesh_w), host arithmetic only (no GPU): out = W as a plain
// row-major [2 (n - 1)][n] matrix (column n - 1: the constant term; rows = (d theta, d|V|) of the non-slack buses in bus order), so that
// x = W [P_spec of the non-slack buses in bus order; 1].  Test aid.  GS_E_TOPOLOGY: the network has a bus that is neither the slack nor PQ,
// or the flat-start Jacobian is singular.
int gs_flat_newton_map_dump(const gs_topology* topo, int32_t zero_z_mode, double* out) {
  if (!topo || !out) return fail(nullptr, GS_E_INVALID, "topology / out is NULL");
  if (topo->struct_size != (int32_t)sizeof(gs_topology)) return fail(nullptr, GS_E_INVALID, "struct_size mismatch");
  HostTopology ht;
  const std::string err = gs_compile_topology(*topo, zero_z_mode, false, true, ht);
  if (!err.empty()) return fail(nullptr, GS_E_INVALID, "topology: %s", err.c_str());
  for (int i = 0; i < ht.n; ++i)
    if (i != ht.slack && !(ht.th_free[i] && ht.vm_free[i])) return fail(nullptr, GS_E_TOPOLOGY, "a bus other than the slack is not a PQ bus");
  const int na = ht.n - 1, N2 = 2 * na, K = na + 1, tiles = (N2 + 15) / 16, steps = (K + 3) / 4;
  std::vector<double> wt;
  if (!flat_newton_map(ht, tiles, steps, wt)) return fail(nullptr, GS_E_TOPOLOGY, "the flat-start Jacobian is singular");
  for (int u = 0; u < N2; ++u)
    for (int k = 0; k < K; ++k) out[(size_t)u * K + k] = wt[((size_t)(u / 16) * steps + k / 4) * 64 + (u % 16) + 16 * (k % 4)];
  return GS_OK;
}

// ---- measurement ------------------------------------------------------------------------------------
int gs_debug_stamps(gs_handle* h, uint64_t* cycles_out, int32_t n) {
  if (!h || !cycles_out || n < 1 || n > 16) return fail(h, GS_E_INVALID, "bad arguments");
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (!h->d_stamps) {
    int rc = dev_alloc(h, &h->d_stamps, 16 + 2 * GS_STAMP_BLOCKS);
    if (rc) return rc;
    HIPCHK(h, hipMemset(h->d_stamps, 0, (16 + 2 * GS_STAMP_BLOCKS) * sizeof(unsigned long long)));
    h->SC.stamps = h->d_stamps;
    h->DA.stamps = h->d_stamps;
    h->SA.stamps = h->d_stamps;
    h->SC.stamp_wave = getenv("GS_STAMP_WAVE") ? atoi(getenv("GS_STAMP_WAVE")) : 0;
    h->SC.block_times = getenv("GS_STAMP_BLOCK_TIMES") ? 1 : 0;
    for (int k = 0; k < n; ++k) cycles_out[k] = 0;
    return GS_OK;
  }
  unsigned long long tmp[16];
  HIPCHK(h, hipMemcpy(tmp, h->d_stamps, sizeof tmp, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemset(h->d_stamps, 0, sizeof tmp));
  for (int k = 0; k < n; ++k) cycles_out[k] = tmp[k];
  return GS_OK;
}

// (start, end) of every workgroup of the LAST step launch on the 100 MHz real-time clock (flow2 kernels, armed by
// gs_debug_stamps with GS_STAMP_BLOCK_TIMES set); returns the pairs of the first n_blocks workgroups
int gs_debug_block_times(gs_handle* h, uint64_t* out, int32_t n_blocks) {
  if (!h || !out || n_blocks < 1 || n_blocks > GS_STAMP_BLOCKS) return fail(h, GS_E_INVALID, "bad arguments");
  if (!h->d_stamps) return fail(h, GS_E_STATE, "gs_debug_stamps has not armed the buffer");
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, h->d_stamps + 16, (size_t)n_blocks * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemset(h->d_stamps + 16, 0, (size_t)2 * GS_STAMP_BLOCKS * sizeof(unsigned long long)));
  return GS_OK;
}

int gs_timing_enable(gs_handle* h, int32_t on) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->timing = on == 1;
  h->timing_span = on == 2;
  h->span_open = false;
  h->timed_used = 0;
  return GS_OK;
}

int gs_timing_read(gs_handle* h, double* total_ms, int64_t* launches) {
  if (!h || !total_ms || !launches) return fail(h, GS_E_INVALID, "bad arguments");
  GS_ENTER(h);
  if (h->timing_span) {           // call right after the last launch of the region: the closing event goes behind it on the stream
    for (int k = 0; k < GS_K_COUNT; ++k) { total_ms[k] = 0.0; launches[k] = 0; }
    if (h->span_open) {
      HIPCHK(h, hipEventRecord(h->span_b, h->stream));
      HIPCHK(h, hipEventSynchronize(h->span_b));
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, h->span_a, h->span_b) == hipSuccess) {
        // the whole span is booked on the kernel that was launched most (the step / solve kernel of a measurement loop)
        int best = 0;
        for (int k = 1; k < GS_K_COUNT; ++k) if (h->span_launches[k] > h->span_launches[best]) best = k;
        total_ms[best] = ms;
        for (int k = 0; k < GS_K_COUNT; ++k) launches[k] = h->span_launches[k];
      }
      h->span_open = false;
    }
    return GS_OK;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < GS_K_COUNT; ++k) { total_ms[k] = 0.0; launches[k] = 0; }
  for (size_t i = 0; i < h->timed_used; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->timed[i].a, h->timed[i].b) == hipSuccess) {
      total_ms[h->timed[i].kid] += ms; launches[h->timed[i].kid] += 1;
    }
  }
  h->timed_used = 0;
  return GS_OK;
}


static int debug_rows_map(gs_handle* h, int32_t which, std::vector<int32_t>& map) {
  const GsRows& R = h->R;
  const int row0[GS_ROWS_COUNT] = {R.VM.base, R.LOAD, R.ENVLOAD.base, R.FLOW.base, R.FREQ, R.CONV, R.ITERS, R.MAXMIS, R.LOADP};
  const int stride[GS_ROWS_COUNT] = {2, 1, 2, 2, 1, 1, 1, 1, 1};
  const int width[GS_ROWS_COUNT] = {h->n, h->m, h->m, h->m, 1, 1, 1, 1, h->n_loads};
  map.resize(width[which]);
  for (int k = 0; k < width[which]; ++k) map[k] = row0[which] + stride[which] * k;
  return width[which];
}

int gs_debug_write_rows(gs_handle* h, int32_t which, const double* values) {
  if (!h || !values || which < 0 || which >= GS_ROWS_COUNT) return fail(h, GS_E_INVALID, "bad arguments");
  GS_ENTER(h);
  { int rc0 = ensure_rows(h); if (rc0) return rc0; }
  std::vector<int32_t> map;
  const int C = debug_rows_map(h, which, map);
  if (C <= 0) return GS_OK;
  if ((size_t)h->B * C > h->in_doubles) return fail(h, GS_E_INVALID, "staging buffer too small");
  int32_t* dmap = nullptr;
  HIPCHK(h, hipMalloc((void**)&dmap, C * sizeof(int32_t)));
  int rc = GS_OK;
  if (hipMemcpyAsync(dmap, map.data(), C * sizeof(int32_t), hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = fail(h, GS_E_HIP, "map upload failed");
  if (!rc) rc = unpack_from_host(h, dmap, C, values);
  const hipError_t e = hipStreamSynchronize(h->stream);
  (void)hipFree(dmap);
  if (!rc && e != hipSuccess) rc = fail(h, GS_E_HIP, "row write failed");
  return rc;
}

int gs_debug_read_rows(gs_handle* h, int32_t which, double* values) {
  if (!h || !values || which < 0 || which >= GS_ROWS_COUNT) return fail(h, GS_E_INVALID, "bad arguments");
  GS_ENTER(h);
  { int rc0 = ensure_rows(h); if (rc0) return rc0; }
  std::vector<int32_t> map;
  const int C = debug_rows_map(h, which, map);
  if (C <= 0) return GS_OK;
  if ((size_t)h->B * C > h->out_doubles) return fail(h, GS_E_INVALID, "staging buffer too small");
  int32_t* dmap = nullptr;
  HIPCHK(h, hipMalloc((void**)&dmap, C * sizeof(int32_t)));
  int rc = GS_OK;
  if (hipMemcpyAsync(dmap, map.data(), C * sizeof(int32_t), hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = fail(h, GS_E_HIP, "map upload failed");
  if (!rc) rc = pack_to_host(h, dmap, C, values);
  (void)hipStreamSynchronize(h->stream);
  (void)hipFree(dmap);
  return rc;
}

// ---- linear-approximation fallback ------------------------------------------------------------------
int gs_fallback_linear(gs_handle* h, const double* load_w, const double* gen_w, const double* total_load,
                       const double* total_gen, const uint8_t* mask, uint8_t* applied_out, int32_t* n_applied) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if ((load_w == nullptr) != (gen_w == nullptr)) return fail(h, GS_E_INVALID, "load_w and gen_w go together");
  if ((total_load == nullptr) != (total_gen == nullptr)) return fail(h, GS_E_INVALID, "total_load and total_gen go together");
  if (!load_w && total_load) return fail(h, GS_E_INVALID, "totals without per-bus arrays: with the device state the sums are formed on the device");
  if (!load_w && !h->was_reset) return fail(h, GS_E_STATE, "no environment state on the device: call gs_reset first or pass load_w / gen_w");
  GS_ENTER(h);
  { int rc0 = ensure_rows(h); if (rc0) return rc0; }      // only the selected instances are overwritten: the others' rows must be current
  const int B = h->B, n = h->n;
  int rc = GS_OK;
  if (!h->fb_ready) {
    const HostTopology& ht = h->topo;
    // the order in which _calculate_power_injections fills its dicts (grid_env.py:683-720): load buses by first
    // appearance in the load list, then battery buses not seen before (a charging battery adds a load entry);
    // generator buses likewise, then battery buses (a discharging battery adds a generation entry)
    auto order_of = [&](const std::vector<int32_t>& ptr, const std::vector<int32_t>& idx, int count) {
      std::vector<int32_t> bus_of(count, 0), out; std::vector<char> seen(n, 0);
      for (int i = 0; i < n; ++i) for (int p = ptr[i]; p < ptr[i + 1]; ++p) bus_of[idx[p]] = i;
      for (int d = 0; d < count; ++d) if (!seen[bus_of[d]]) { seen[bus_of[d]] = 1; out.push_back(bus_of[d]); }
      std::vector<int32_t> bat_bus(h->n_bats, 0);
      for (int i = 0; i < n; ++i) for (int p = ht.bb_ptr[i]; p < ht.bb_ptr[i + 1]; ++p) bat_bus[ht.bb_idx[p]] = i;
      for (int q = 0; q < h->n_bats; ++q) if (!seen[bat_bus[q]]) { seen[bat_bus[q]] = 1; out.push_back(bat_bus[q]); }
      return out; };
    const std::vector<int32_t> lo = order_of(ht.bl_ptr, ht.bl_idx, h->n_loads), go = order_of(ht.bg_ptr, ht.bg_idx, h->n_gens);
    if ((rc = dev_upload(h, &h->FB.load_order, lo)) || (rc = dev_upload(h, &h->FB.gen_order, go)) ||
        (rc = dev_upload(h, &h->FB.line_x, h->line_x))) return rc;
    h->FB.n_load_order = (int32_t)lo.size(); h->FB.n_gen_order = (int32_t)go.size();
    if ((rc = dev_alloc(h, &h->fb_load, (size_t)B * n)) || (rc = dev_alloc(h, &h->fb_gen, (size_t)B * n)) ||
        (rc = dev_alloc(h, &h->fb_tl, (size_t)B)) || (rc = dev_alloc(h, &h->fb_tg, (size_t)B)) ||
        (rc = dev_alloc(h, &h->fb_mask, (size_t)B)) || (rc = dev_alloc(h, &h->fb_applied, (size_t)B))) return rc;
    h->fb_ready = true;
  }
  GsFallbackArgs A = h->FB;
  A.env_mode = load_w ? 0 : 1;
  if (h->pz) { A.line_x = h->LP.x; A.line_x_stride = h->m; }       // every instance's own reactances
  if (load_w) {
    HIPCHK(h, hipMemcpyAsync(h->fb_load, load_w, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->fb_gen, gen_w, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    A.load_w = h->fb_load; A.gen_w = h->fb_gen;
    if (total_load) {
      HIPCHK(h, hipMemcpyAsync(h->fb_tl, total_load, (size_t)B * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(h->fb_tg, total_gen, (size_t)B * sizeof(double), hipMemcpyHostToDevice, h->stream));
      A.tot_load = h->fb_tl; A.tot_gen = h->fb_tg;
    }
  }
  if (mask) { HIPCHK(h, hipMemcpyAsync(h->fb_mask, mask, (size_t)B, hipMemcpyHostToDevice, h->stream)); A.mask = h->fb_mask; }
  A.applied = h->fb_applied;
  hipLaunchKernelGGL(gs_k_fallback_linear, dim3(h->groups), dim3(64), 0, h->stream, h->T, h->R, A, h->slab, B);
  HIPCHK(h, hipGetLastError());
  std::vector<int32_t> ap(B);
  HIPCHK(h, hipMemcpyAsync(ap.data(), h->fb_applied, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int32_t cnt = 0;
  for (int b = 0; b < B; ++b) { cnt += ap[b] != 0; if (applied_out) applied_out[b] = ap[b] != 0; }
  if (n_applied) *n_applied = cnt;
  return GS_OK;
}

// ---- post-step checks -------------------------------------------------------------------------------
struct gs_checks {
  gs_handle* h = nullptr;
  GsChecksCfg C{};
  double* prev = nullptr; int32_t* state = nullptr; int32_t* out_i = nullptr; double* out_f = nullptr;
  uint8_t *bus_mask = nullptr, *line_mask = nullptr; double* freq = nullptr; bool use_freq = false, want_masks = true;
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; size_t ev_used = 0;
};

}  // extern "C"  (helpers below have C++ linkage)
namespace {
GsFusedChecks fused_checks_args(gs_handle* h) {
  GsFusedChecks f{};
  if (h->fused) {
    gs_checks* c = h->fused;
    f.C = c->C; f.prev = c->prev; f.state = c->state; f.out_i = c->out_i; f.out_f = c->out_f;
    f.bus_mask = c->want_masks ? c->bus_mask : nullptr; f.line_mask = c->want_masks ? c->line_mask : nullptr;
    f.enabled = 1; f.Bp = h->Bp;
  }
  return f;
}
}  // namespace
extern "C" {

int gs_checks_set_fused(gs_checks* c, int32_t on, int32_t want_masks) {
  if (!c) return fail(nullptr, GS_E_INVALID, "checks object is NULL");
  gs_handle* h = c->h;
  if (on && (h->n >= 65536 || h->m >= 65536)) return fail(h, GS_E_INVALID, "fused checks count in 16 bits: fewer than 65536 buses and lines");
  if (on && h->fused && h->fused != c) return fail(h, GS_E_STATE, "another checks object is already fused into this handle's step");
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  c->want_masks = want_masks != 0;
  if (on) h->fused = c; else if (h->fused == c) h->fused = nullptr;
  return GS_OK;
}

int gs_checks_create(gs_handle* h, const gs_checks_config* cfg, gs_checks** out) {
  if (!h || !cfg || !out) return fail(h, GS_E_INVALID, "handle / config / out is NULL");
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(gs_checks_config)) return fail(h, GS_E_INVALID, "gs_checks_config.struct_size mismatch");
  if (!(cfg->timestep > 0.0)) return fail(h, GS_E_INVALID, "timestep must be positive");
  if (cfg->loading_source != 0 && cfg->loading_source != 1) return fail(h, GS_E_INVALID, "loading_source must be 0 or 1");
  GS_ENTER(h);
  gs_checks* c = new gs_checks();
  c->h = h;
  GsChecksCfg& C = c->C;
  C.c_vlo = cfg->voltage_limits[0]; C.c_vhi = cfg->voltage_limits[1]; C.c_flo = cfg->frequency_limits[0]; C.c_fhi = cfg->frequency_limits[1];
  C.c_load = cfg->line_loading_limit; C.c_rocv = cfg->rate_voltage; C.c_rocf = cfg->rate_frequency; C.dt = cfg->timestep;
  C.m_vlo = cfg->mon_voltage_limits[0]; C.m_vhi = cfg->mon_voltage_limits[1]; C.m_flo = cfg->mon_frequency_limits[0]; C.m_fhi = cfg->mon_frequency_limits[1];
  C.m_load = cfg->mon_line_loading_limit; C.m_evlo = cfg->mon_emergency_voltage[0]; C.m_evhi = cfg->mon_emergency_voltage[1];
  C.m_eflo = cfg->mon_emergency_frequency[0]; C.m_efhi = cfg->mon_emergency_frequency[1];
  C.q_tol = cfg->quality_tolerance;
  C.n = h->n; C.m = h->m; C.rows_total = h->R.total;
  C.row_vm = h->R.VM.base; C.row_qload = h->R.LOAD; C.row_flow = h->R.FLOW.base;
  C.row_cload = cfg->loading_source ? h->R.ENVLOAD.base : h->R.LOAD; C.stride_cload = cfg->loading_source ? 2 : 1;
  C.row_freq = h->R.FREQ; C.row_conv = h->R.CONV; C.row_iters = h->R.ITERS; C.row_maxmis = h->R.MAXMIS;
  const size_t Bp = h->Bp;
  bool ok = hipMalloc((void**)&c->prev, (size_t)h->groups * (h->n + 1) * GS_LANES * sizeof(double)) == hipSuccess &&
            hipMalloc((void**)&c->state, 3 * Bp * sizeof(int32_t)) == hipSuccess &&
            hipMalloc((void**)&c->out_i, (size_t)GS_CI_COUNT * Bp * sizeof(int32_t)) == hipSuccess &&
            hipMalloc((void**)&c->out_f, (size_t)GS_CF_COUNT * Bp * sizeof(double)) == hipSuccess &&
            hipMalloc((void**)&c->bus_mask, std::max<size_t>(1, (size_t)h->groups * h->n * GS_LANES)) == hipSuccess &&
            hipMalloc((void**)&c->line_mask, std::max<size_t>(1, (size_t)h->groups * h->m * GS_LANES)) == hipSuccess &&
            hipMalloc((void**)&c->freq, Bp * sizeof(double)) == hipSuccess;
  ok = ok && hipMemset(c->prev, 0, (size_t)h->groups * (h->n + 1) * GS_LANES * sizeof(double)) == hipSuccess &&
       hipMemset(c->state, 0, 3 * Bp * sizeof(int32_t)) == hipSuccess && hipMemset(c->out_i, 0, (size_t)GS_CI_COUNT * Bp * sizeof(int32_t)) == hipSuccess &&
       hipMemset(c->out_f, 0, (size_t)GS_CF_COUNT * Bp * sizeof(double)) == hipSuccess &&
       hipDeviceSynchronize() == hipSuccess;        // (done before the check kernels, which run on the handle's non-blocking stream)
  if (!ok) { gs_checks_destroy(c); return fail(h, GS_E_NOMEM, "device allocation for the checks failed"); }
  *out = c;
  return GS_OK;
}

void gs_checks_destroy(gs_checks* c) {
  if (!c) return;
  if (c->h->fused == c) c->h->fused = nullptr;
  (void)hipSetDevice(c->h->device);
  (void)hipStreamSynchronize(c->h->stream);
  for (auto& e : c->ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  for (void* p : {(void*)c->prev, (void*)c->state, (void*)c->out_i, (void*)c->out_f, (void*)c->bus_mask, (void*)c->line_mask, (void*)c->freq})
    if (p) (void)hipFree(p);
  delete c;
}

int gs_checks_set_frequency(gs_checks* c, const double* f) {
  if (!c) return fail(nullptr, GS_E_INVALID, "checks object is NULL");
  gs_handle* h = c->h;
  GS_ENTER(h);
  c->use_freq = f != nullptr;
  if (f) { HIPCHK(h, hipMemcpyAsync(c->freq, f, (size_t)h->B * sizeof(double), hipMemcpyHostToDevice, h->stream)); HIPCHK(h, hipStreamSynchronize(h->stream)); }
  return GS_OK;
}

int gs_checks_run(gs_checks* c) {
  if (!c) return fail(nullptr, GS_E_INVALID, "checks object is NULL");
  gs_handle* h = c->h;
  GS_ENTER(h);
  { int rc0 = ensure_rows(h); if (rc0) return rc0; }      // the kernel reads the |V| / loading / flow rows of the last step
  // HIP events only while somebody reads them (gs_checks_timing_enable), and never more than GS_CHECKS_MAX_EVENTS pairs:
  // a per-step safety check over a long run must not grow an event list without bound
  std::pair<hipEvent_t, hipEvent_t>* e = nullptr;
  if (c->timing && c->ev_used < GS_CHECKS_MAX_EVENTS) {
    if (c->ev_used == c->ev.size()) {
      hipEvent_t a, b2;
      HIPCHK(h, hipEventCreate(&a)); HIPCHK(h, hipEventCreate(&b2));
      c->ev.emplace_back(a, b2);
    }
    e = &c->ev[c->ev_used++];
    HIPCHK(h, hipEventRecord(e->first, h->stream));
  }
  hipLaunchKernelGGL(gs_k_checks, dim3(h->groups), dim3(1024), 0, h->stream, c->C, h->slab, c->use_freq ? c->freq : (const double*)nullptr,
                     c->prev, c->state, c->out_i, c->out_f, c->bus_mask, c->line_mask, h->B, h->Bp);
  HIPCHK(h, hipGetLastError());
  if (e) HIPCHK(h, hipEventRecord(e->second, h->stream));
  return GS_OK;
}

int gs_checks_download(gs_checks* c, const gs_checks_view* out) {
  if (!c || !out) return fail(c ? c->h : nullptr, GS_E_INVALID, "checks object / view is NULL");
  gs_handle* h = c->h;
  GS_ENTER(h);
  const size_t Bp = h->Bp, B = h->B;
  std::vector<int32_t> ti; std::vector<double> tf; std::vector<uint8_t> tb, tl;
  if (out->ints) { ti.resize((size_t)GS_CI_COUNT * Bp); HIPCHK(h, hipMemcpyAsync(ti.data(), c->out_i, ti.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream)); }
  if (out->reals) { tf.resize((size_t)GS_CF_COUNT * Bp); HIPCHK(h, hipMemcpyAsync(tf.data(), c->out_f, tf.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream)); }
  if (out->bus_mask && h->n) { tb.resize((size_t)h->groups * h->n * GS_LANES); HIPCHK(h, hipMemcpyAsync(tb.data(), c->bus_mask, tb.size(), hipMemcpyDeviceToHost, h->stream)); }
  if (out->line_mask && h->m) { tl.resize((size_t)h->groups * h->m * GS_LANES); HIPCHK(h, hipMemcpyAsync(tl.data(), c->line_mask, tl.size(), hipMemcpyDeviceToHost, h->stream)); }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (out->ints) for (int k = 0; k < GS_CI_COUNT; ++k) memcpy(out->ints + (size_t)k * B, ti.data() + (size_t)k * Bp, B * sizeof(int32_t));
  if (out->reals) for (int k = 0; k < GS_CF_COUNT; ++k) memcpy(out->reals + (size_t)k * B, tf.data() + (size_t)k * Bp, B * sizeof(double));
  auto untile = [&](const std::vector<uint8_t>& t, uint8_t* dst, int width) {     // [group][row][lane] -> [b][row]
    for (size_t b = 0; b < B; ++b) {
      const size_t g = b / GS_LANES, lane = b % GS_LANES;
      for (int r = 0; r < width; ++r) dst[b * width + r] = t[(g * width + r) * GS_LANES + lane];
    }
  };
  if (out->bus_mask && h->n) untile(tb, out->bus_mask, h->n);
  if (out->line_mask && h->m) untile(tl, out->line_mask, h->m);
  return GS_OK;
}

int gs_checks_reset(gs_checks* c, const uint8_t* mask) {
  if (!c) return fail(nullptr, GS_E_INVALID, "checks object is NULL");
  gs_handle* h = c->h;
  GS_ENTER(h);
  uint8_t* dmask = nullptr;
  if (mask) {
    HIPCHK(h, hipMalloc((void**)&dmask, h->B));
    if (hipMemcpyAsync(dmask, mask, h->B, hipMemcpyHostToDevice, h->stream) != hipSuccess) { (void)hipFree(dmask); return fail(h, GS_E_HIP, "mask upload failed"); }
  }
  hipLaunchKernelGGL(gs_k_checks_reset, dim3((h->B + 255) / 256), dim3(256), 0, h->stream, c->state, (const uint8_t*)dmask, h->B, h->Bp);
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(h->stream);
  if (dmask) (void)hipFree(dmask);
  if (e1 != hipSuccess || e2 != hipSuccess) return fail(h, GS_E_HIP, "checks reset failed");
  return GS_OK;
}

int gs_checks_timing_enable(gs_checks* c, int32_t on) {
  if (!c) return fail(nullptr, GS_E_INVALID, "checks object is NULL");
  GS_ENTER(c->h);
  HIPCHK(c->h, hipStreamSynchronize(c->h->stream));
  c->timing = on != 0; c->ev_used = 0;
  return GS_OK;
}

int gs_checks_timing_read(gs_checks* c, double* total_ms, int64_t* launches) {
  if (!c || !total_ms || !launches) return fail(c ? c->h : nullptr, GS_E_INVALID, "bad arguments");
  gs_handle* h = c->h;
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *total_ms = 0.0; *launches = 0;
  for (size_t k = 0; k < c->ev_used; ++k) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev[k].first, c->ev[k].second) == hipSuccess) { *total_ms += ms; *launches += 1; }
  }
  c->ev_used = 0;
  return GS_OK;
}

}  // extern "C"
