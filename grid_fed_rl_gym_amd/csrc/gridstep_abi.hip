// gridstep_abi.hip -- the handle's life and the step path of the C ABI declared in include/gridstep.h.
//
// Owns: gs_create / gs_destroy (the compiled topology tables, one slab of per-instance rows in HBM, slab[group][row][64 lanes],
// staging buffers for the batch-major <-> batch-innermost layout change, the step's streams), the layout movers, the launch code
// of the solve and of the step (step_kernels), and the entry points that are that path: per-instance line impedances and load
// powers, the solver API, reset / step / download, the host-observation binding, the device-pointer steps, checkpoints.  The handle
// itself and what the other host files share with this one: handle.h.  The policy and the rollout: abi_rollout.hip; the
// all-gather: abi_comm.hip; checks and fallback: abi_checks.hip; dumps, stamps and timing: abi_debug.hip.
// No CPU arithmetic on the data path: every entry point either moves bytes or launches kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "handle.h"

using namespace gsi;

namespace {

thread_local std::string g_last_error;

// ---- layout movers --------------------------------------------------------------------------
int launch_pack(gs_handle* h, const int32_t* map, int C, double* dst) {
  if (C <= 0) return GS_OK;
  LaunchTimer lt(h, GS_K_PACK);
  dim3 grid(h->groups, (C + 63) / 64);
  hipLaunchKernelGGL(gs_k_pack, grid, dim3(256), 0, h->stream, map, h->d_cst, C, h->R.total, h->slab, dst, h->B);
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

// step_kernels: the checks fused into the step kernel's epilogue (gs_checks_set_fused), as the kernel takes them
GsFusedChecks fused_checks_args(gs_handle* h) {
  GsFusedChecks f{};
  if (h->fused) {
    gs_checks* c = h->fused;
    f.C = c->C; f.prev = c->prev; f.state = c->state; f.out_i = c->out_i; f.out_f = c->out_f;
    f.bus_mask = c->want_masks ? c->bus_mask.p : nullptr; f.line_mask = c->want_masks ? c->line_mask.p : nullptr;
    f.enabled = 1; f.Bp = h->Bp;
  }
  return f;
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

// ---- what handle.h declares of this file ------------------------------------------------------
namespace gsi __attribute__((visibility("hidden"))) {

int fail(gs_handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_last_error = buf;
  if (h) h->err = buf;
  return code;
}

// each instance's own static load columns of a per-instance-loads handle (GsPlan::pl) into the observation block dst [B][obs_dim]
int launch_load_columns(gs_handle* h, double* dst) {
  const size_t threads = (size_t)h->B * 2 * h->n_loads;
  hipLaunchKernelGGL(gs_k_load_columns, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->LL.pl, dst, h->B, h->obs_dim,
                     2 * h->n + 2 * h->m + 1, h->n_loads);
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

// obs_out: where the step writes the changing columns of its observation block ([B][obs_dim], constants already in
// place); NULL = the other one of the handle's two observation buffers
int step_kernels(gs_handle* h, const double* d_actions, double* obs_out, const GsRolloutStep* rs) {
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

}  // namespace gsi

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
  fed_detach(h);                  // federations this handle is a client of refuse every further call
  (void)gs_comm_destroy(h);       // the communicator and its buffers, if the handle has one
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
  h->d_actions.release();
  learner_release(h);
  policy_release(h);
  value_release(h);
  q_release(h);
  rollout_release(h);
  dataset_release(h);
  load_release(h);
  if (h->h_pin) (void)hipHostFree(h->h_pin);
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
  h->env_moves += 1;          // (episode accounting: the environment moves outside gs_rollout)
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
  h->env_moves += 1;          // (episode accounting: the environment moves outside gs_rollout)
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
  h->env_moves += 1;          // (episode accounting: the environment moves outside gs_rollout)
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
  h->env_moves += 1;          // (episode accounting: the environment moves outside gs_rollout)
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
  h->env_moves += 1;          // (episode accounting: the environment moves outside gs_rollout)
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
  h->env_moves += 1;          // (episode accounting: the environment moves outside gs_rollout)
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
  int rc = publish(h, h->stream, h->ev_peer2, consumer_stream);
  if (rc) return rc;
  out->observations = h->d_obs2[h->obs_cur];
  out->reward = h->sc_f + (size_t)SF_REWARD * h->Bp;
  out->terminated = h->sc_u + (size_t)SU_TERM * h->Bp;
  out->truncated = h->sc_u + (size_t)SU_TRUNC * h->Bp;
  out->B = h->B; out->obs_dim = h->obs_dim;
  return GS_OK;
}

// doubles that one batch of gs_upload_actions takes in d_actions
static size_t action_batch(const gs_handle* h) { return (size_t)h->B * std::max(h->action_dim, 1); }

int gs_upload_actions(gs_handle* h, const double* actions, int32_t n_batches) {
  if (!h || !actions || n_batches <= 0) return fail(h, GS_E_INVALID, "bad arguments");
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // (always a fresh allocation of exactly n_batches batches: gs_step_device counts them by the buffer's capacity)
  int rc = h->d_actions.alloc(h, action_batch(h) * n_batches, "the uploaded actions");
  if (rc) return rc;
  HIPCHK(h, hipMemcpy(h->d_actions, actions, (size_t)n_batches * h->B * h->action_dim * sizeof(double), hipMemcpyHostToDevice));
  return GS_OK;
}

int gs_step_device(gs_handle* h, int32_t k) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (!h->was_reset) return fail(h, GS_E_STATE, "gs_step_device before gs_reset");
  const int have = (int)(h->d_actions.cap / action_batch(h));      // (0 without an upload, and after one that failed)
  if (k < 0 || k >= have) return fail(h, GS_E_INVALID, "action batch %d not uploaded (have %d)", k, have);
  HIPCHK(h, hipSetDevice(h->device));
  h->env_moves += 1;          // (episode accounting: the environment moves outside gs_rollout)
  return step_kernels(h, h->d_actions + (size_t)k * h->B * h->action_dim);
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
  h->env_moves += 1;          // (episode accounting: the environment moves outside gs_rollout)
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

}  // extern "C"
