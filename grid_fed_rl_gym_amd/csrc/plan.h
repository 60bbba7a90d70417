// plan.h -- host-side planning of a handle: which kernel members serve it, the slab rows, and every table gs_create uploads.
// Pure host C++ (no HIP): gs_create plans, then uploads the plan and launches the flat-start captures; gs_plan_describe
// answers gs_describe's question for a handle that was never created (tests/test_plan.py, no device).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/gridstep.h"
#include "gs_internal.h"
#include "members.h"
#include "topology.h"

// the per-instance scalars gs_k_scalars copies to the host (rows rf / ri / ru of the plan)
enum { SF_REWARD = 0, SF_VMAX, SF_VMIN, SF_LOSSES, SF_EPREW, SF_MAXMIS, SF_COUNT };
enum { SI_VIOL = 0, SI_STEP, SI_ITERS, SI_STATUS, SI_COUNT };
enum { SU_TERM = 0, SU_TRUNC, SU_CONV, SU_VF0, SU_VF1, SU_VF2, SU_VF3, SU_COUNT };

struct GsPlan {
  int err_code = 0;                        // GS_E_TOPOLOGY / GS_E_INVALID when gs_plan rejects
  SolveMember solve = SolveMember::fbs;
  StepMember step = StepMember::none;
  int B = 0, Bp = 0, groups = 0, W = 1;
  int n = 0, m = 0, obs_dim = 0, action_dim = 0, state_dim = 0;
  int n_loads = 0, n_gens = 0, n_bats = 0;
  size_t dyn_lds = 0;
  GsRows R{};
  GsSolveCfg SC{};
  GsEnvCfg EC{};                           // (first_instance: gs_create's)
  double total_load = 0.0;
  GsF2Tables F2{};                         // second-generation step kernels: 64 / f2().iw workgroups per slab group
  std::string flow2_why, mesh_why;         // why no second-generation member took the step ("" = not considered)
  int mesh_levels = 0, mesh_rows = 0, mesh_units = 0, mesh_messages = 0, mesh_accs = 0;
  // nr_dense_mfma: a launch of its own between the two halves of the step / solve
  GsDenseArgs DA{}; int dense_grid = 0; size_t dense_lds = 0; bool dense_blockrow = true, dense_flat = false;
  // nr_sparse_lds (experiments build), launched the same way
  GsSparseArgs SA{}; int sparse_grid = 0; size_t sparse_lds = 0;
  // A step of a second-generation member as two half-grid launches on two streams (gs_handle::split_ok); lean: the step leaves
  // the result rows to be restored from its observation block (gs_handle::rows_stale)
  bool split_ok = false, lean = false;
  int obs_skip0 = 0, obs_skip1 = 0;        // the block of per-instance constants inside an observation

  // ---- host tables, uploaded by gs_create ----
  std::vector<GsItemRec> witems; std::vector<int32_t> wl_ptr, ovf_slot;       // forest sweeps: per-wave work lists
  std::vector<GsInjRec> winj; std::vector<int32_t> wi_ptr;                    // injection records
  std::vector<GsBusRec> wbus; std::vector<int32_t> wb_ptr;                    // mismatch records
  std::vector<GsF2Rec> f2recs; std::vector<int32_t> f2anc; std::vector<double> f2z;
  std::vector<int32_t> fs_slot; std::vector<double> fs_val;                   // buses with a voltage set point (second generation)
  std::vector<double> mesh_w;                                                 // GsF2Tables::mesh_w, empty: none
  std::vector<int32_t> mesh_items, mesh_rowinfo;
  std::vector<int32_t> lu_a_ptr, lu_a, lu_b_ptr, lu_b, lu_c_ptr, lu_c, lu_r_ptr, lu_r;
  std::vector<int32_t> act_bus, act_of, ent_ptr, ent, bent_ptr; std::vector<GsDenseEntry> bent;
  std::vector<double> jinv_t;                                                 // GsDenseArgs::jinv_t, empty: none
  std::vector<int32_t> mo, mvm, mva, mfl, mld, mp, mq, mact, mst; std::vector<double> cst;     // layout maps
  std::vector<int32_t> rf, ri, ru;
#if defined(GS_BUILD_EXPERIMENTS)
  std::vector<int32_t> ipack; std::vector<double> dpack;                      // GsSparseArgs::ipack / dpack
#endif

  // per-instance line impedances (gs_topology::line_r_inst / line_x_inst): the step member's PZ kernels, the tables of
  // gs_k_line_params (GsLineParamArgs); nr_flat: Newton-Raphson's flat-start table is captured (gs_create) and read
  bool pz = false, nr_flat = false;
  std::vector<int32_t> pz_ops_ptr, pz_ops; std::vector<uint8_t> pz_has, pz_zero;

  // per-instance load powers (gs_topology::load_base_inst): the step member's PL kernels read gs_k_load_params' entries
  // (GsLoadParamArgs); such a handle has no block of constant observation columns (obs_skip0 == obs_skip1): its step writes the
  // static load columns itself.  pl_tan: tan(acos(pf)) per load, topology.cpp's expression
  bool pl = false;
  std::vector<double> pl_tan;

  bool second_gen() const { return step != StepMember::none; }
  const StepMemberRow& f2() const { return step_row(step); }
};

// Plans a handle of `batch` instances for a device of `cus` compute units.  Returns "" or the rejection message (out.err_code:
// its GS_E_* code).  Reads the GS_* switches of gs_internal.h.
std::string gs_plan(const gs_topology& topo, const gs_config& cfg, const HostTopology& ht, int batch, int cus, GsPlan& out);
// "" or why per-instance impedances r_inst / x_inst [B][m] break the rules of gs_topology (rows where mask[b] != 0, or all)
std::string gs_check_line_impedances(const gs_topology& topo, int batch, const double* r_inst, const double* x_inst, const uint8_t* mask);
// "" or why per-instance load powers base_inst [B][n_loads] break the rules of gs_topology (rows where mask[b] != 0, or all)
std::string gs_check_load_powers(int n_loads, int batch, const double* base_inst, const uint8_t* mask);
// gs_describe's JSON for a handle with this plan
void gs_plan_format(const GsPlan& p, const HostTopology& ht, char* buf, int buflen);
// GsF2Tables::mesh_w of an all-PQ network (see plan.cpp); false: J0 singular or the sizes do not fit
bool flat_newton_map(const HostTopology& ht, int tiles, int steps, std::vector<double>& wt);
