// members.h -- the kernel members the planner chooses among, each described once.  Plain C++ (no HIP): the planner (plan.cpp)
// reads the shapes and traits, kernels_flow2.hip instantiates the step kernels from the same rows, and the launch tables of
// kernels.h are indexed by these enums.
#pragma once
#include <cstddef>

// The member that solves the load flow (gs_solve, and the step unless a second-generation member takes it); the names are
// gs_describe's "solve_kernel" strings (plan.cpp kSolveName), the kernel stems those of kernels_solve.hip's launch table.
enum class SolveMember { nr_tree, nr_sparse_lu, fbs, nr_dense_pivot, nr_tree_lds, fbs_lds, fbs_flow, nr_dense_mfma, nr_sparse_lds };

// The second-generation step member (kernels_flow2.hip) that runs the environment step instead of the first-generation one.
enum class StepMember {
  none, fbs_flow2s, fbs_flow2h, fbs_flow2x,
#if defined(GS_BUILD_EXPERIMENTS)
  fbs_flow2,
#endif
  nr_flow2s, nr_flow2, nr_mesh2
};
constexpr int kStepMemberCount = (int)StepMember::nr_mesh2 + 1;

// solver family of a step member: sweeps, Newton-Raphson on a radial feeder, Newton-Raphson on a meshed feeder (block LU with
// fill-in, mesh_schedule.h); kernels_flow2.hip's SOLVER template argument
enum { F2_FBS = 0, F2_NR = 1, F2_NRM = 2 };

// A step member's kernels: nw wavefronts per workgroup, iw instances per workgroup (64 / iw sub-groups of a wavefront, each on a
// bus of its own), ni bus items per sub-group; pz: it has the per-instance line impedance kernels gs_k_step*_<name>_pz.
struct StepMemberRow {
  const char* name;         // gs_describe's "kernel"; the kernels are gs_k_step_<name> / gs_k_stepc_<name>
  int solver, nw, ni, iw;
  bool pz;
  constexpr int positions() const { return nw * (64 / iw) * ni; }      // (wave, sub-group, item) positions: buses / bus groups it holds
  constexpr bool newton() const { return solver == F2_NR || solver == F2_NRM; }
};
constexpr StepMemberRow kStepMembers[] = {
    {"none", -1, 0, 0, 64, false},
    {"fbs_flow2s", F2_FBS, 2, 1, 8, true},     // small feeders: 2 waves x 8 sub-groups x 1 bus = 16 positions
    {"fbs_flow2h", F2_FBS, 8, 4, 16, true},    // the default: 16 instances per workgroup, two workgroups per CU, 128 positions
    {"fbs_flow2x", F2_FBS, 8, 8, 16, true},    // wide: eight buses per sub-group (up to 256 buses), one workgroup per CU
#if defined(GS_BUILD_EXPERIMENTS)
    {"fbs_flow2", F2_FBS, 16, 4, 32, false},   // 32 instances per workgroup, the two halves of a wavefront on different buses (GS_FLOW2_IW=32)
#endif
    // 4 waves x 1 item, each a group of 8 buses of one level (2 x 2: 124 M env-steps/s on config 2; 4 x 1: 147 M -- the load draws
    // get waves of their own)
    {"nr_flow2s", F2_NR, 4, 1, 8, true},
    {"nr_flow2", F2_NR, 8, 8, 32, true},       // 8 waves x 2 halves x 8 bus groups (its bus state needs the registers)
    {"nr_mesh2", F2_NRM, 4, 10, 8, false},     // 4 waves x up to 10 rows of 8 sub-groups
};
static_assert(sizeof kStepMembers / sizeof *kStepMembers == (size_t)kStepMemberCount, "one row per StepMember");
constexpr const StepMemberRow& step_row(StepMember s) { return kStepMembers[(int)s]; }
