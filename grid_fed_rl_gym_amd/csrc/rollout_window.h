// rollout_window.h -- the host side of gs_rollout_continue (include/gridstep.h "a sliding window over consecutive rollouts"; DESIGN.md
// section 30): the checks that run before anything is queued, and the schedule of the launches that move the kept steps to the
// front.  No HIP: rollout_window.cpp compiles as plain C++ (tests/native/rollout_window_host.cpp runs it under the sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/gridstep.h"

// what the checks need to know of the handle
struct GsWindowState {
  int32_t T_cur;            // steps of the rollout the handle holds, 0: none
  int32_t action_dim;
  bool was_reset;           // gs_reset has run
  bool policy_set;          // gs_policy_mlp_set has installed a policy
  bool collected;           // the rollout was collected here (gs_rollout / gs_rollout_continue), not installed by gs_rollout_load
  bool moved;               // the environment was moved since that rollout ended
};
// "" or why gs_rollout_continue refuses `c` on a handle in state `s`; *code: GS_E_INVALID or GS_E_STATE
std::string gs_window_check(const gs_rollout_continue_config* c, const GsWindowState& s, int* code);

// One launch of the shift: `rows` steps of an array from step src_row to step dst_row.
struct GsWindowMove { int32_t src_row, dst_row, rows; };
// The launches that move steps T_old - keep .. T_old - 1 + extra of an array to steps 0 .. keep - 1 + extra (extra = 1: obs_seq, which
// has one slot more than the rollout has steps; 0: the others), in the order they are queued on one stream.
//   in place (disjoint = false): source and destination are one buffer.  The shift distance is T_old - keep rows; every entry moves at
//   most that many (and at most `limit`, <= 0: no further limit), so its source and destination do not overlap, and the entries ascend:
//   what an entry overwrites, the entries before it have already moved.  Nothing when the distance or keep is 0.
//   disjoint = true: the destination is another buffer (the window outgrew the capacity): entries of at most `limit` rows.
std::vector<GsWindowMove> gs_window_schedule(int32_t T_old, int32_t keep, int32_t extra, int32_t limit, bool disjoint);

// ---- the kernels' side (kernels_window.hip) ----
// gs_k_window_shift: blockIdx.y = the array; `bytes` bytes from src to dst (not overlapping), 16 bytes a lane where both pointers and
// the count allow, else 8, else single bytes; a grid-stride loop
#define GS_WIN_ARRAYS 5                  // obs_seq, actions, rewards, done flags, log-probabilities
struct GsWindowSeg { const char* src; char* dst; long long bytes; };
struct GsWindowShiftArgs { GsWindowSeg seg[GS_WIN_ARRAYS]; };

// gs_k_window_terms, ONE workgroup of GS_WIN_TERM_THREADS threads, no atomics: the entries k < min(*count, cap_in) of the terminal
// list idx_in with t >= drop, compacted in the order they lie in (a prefix over the keep flags), t -= drop, into idx_out; pos[k] =
// where entry k went, -1: dropped; *n_old = the entries looked at, *count = the entries kept (plus whatever the old count exceeded
// cap_in by, so that an overflow stays one).  idx_in and idx_out are different buffers.
#define GS_WIN_TERM_THREADS 1024
struct GsWindowTermsArgs {
  const int32_t* idx_in; int32_t* idx_out; int32_t* pos; int32_t* count; int32_t* n_old;
  int32_t cap_in, drop;
};
// gs_k_window_term_rows: row k of obs_in to row pos[k] of obs_out (another buffer) for k < *n_old, pos[k] >= 0; a grid-stride loop
struct GsWindowTermRowsArgs { const double* obs_in; double* obs_out; const int32_t* pos; const int32_t* n_old; int32_t D; };
