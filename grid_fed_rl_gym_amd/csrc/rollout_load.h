// rollout_load.h -- the host side of gs_rollout_load (include/gridstep.h): the checks that run before anything
// is allocated or launched, the shape of the staging, and the terminal list in its ascending order.  No HIP: rollout_load.cpp
// compiles as plain C++ (tests/native/rollout_load_host.cpp runs it under the sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/gridstep.h"

// the library's own staging chunk, in bytes of next_observations (the map rides on top)
constexpr size_t GS_LOAD_CHUNK_BYTES = 16u << 20;

// "" or why gs_rollout_load refuses `s` on a handle of B instances with these widths; out (may be NULL): n, n_terminal and the
// terminal capacity the load needs.  Reads s->terminals (T * B bytes) only after every other check has passed.
std::string gs_load_check(const gs_rollout_source* s, int32_t B, int32_t obs_dim, int32_t action_dim, gs_rollout_load_info* out);

// bytes of one source element (s checked)
inline size_t gs_load_elem(const gs_rollout_source& s) { return s.dtype == GS_COMPUTE_F32 ? sizeof(float) : sizeof(double); }

// rows of next_observations per staging chunk: s.chunk_rows, or what GS_LOAD_CHUNK_BYTES hold; at least 1, at most n
int64_t gs_load_chunk_rows(const gs_rollout_source& s, int32_t obs_dim, int64_t n);

// bytes of a staging buffer: chunk_rows rows of obs_dim source elements and their int32 map entries behind them
inline size_t gs_load_stage_bytes(const gs_rollout_source& s, int32_t obs_dim, int64_t chunk_rows) {
  return (size_t)chunk_rows * ((size_t)obs_dim * gs_load_elem(s) + sizeof(int32_t));
}

// ---- the kernels' side (kernels_load.hip) ----
// gs_k_load_next<SRC> over one staged chunk of next_observations: `rows` rows of D source elements at src, row i being transition
// row0 + i, and map[i] behind them.  A row is owned by `lanes` lanes of one wavefront (8 .. 64, gs_load_lanes), lane = column, every
// load and store of a group one run of consecutive elements.  map[i] >= 0: the row goes to term_obs[map[i]]; -1: it is compared,
// by bits, with obs_seq[t + 1][b], which the load has already written.  Rows of t = T - 1 without a final observation ARE slot T
// and are written there, finished or not.  verdict[0] += the live rows that differ, verdict[1] = min over their transition index.
struct GsLoadNextArgs {
  const void* src; const int32_t* map;
  double* obs_seq; double* term_obs; int32_t* verdict;
  long long row0, n;                     // n = T * B
  int32_t rows, D, B, lanes, term_cap, have_final;
};
// lanes per row of D columns: the smallest power of two in 8 .. 64 that covers the row in four loads a lane
inline int gs_load_lanes(int D) { int l = 8; while (l < 64 && 4 * l < D) l *= 2; return l; }
#define GS_LOAD_WAVES 4                  // wavefronts per workgroup of gs_k_load_next

// map[i] for the rows r0 .. r0 + rows - 1 (row = t * B + b): the row's position in the terminal list, -1 for a live row; *k = the
// terminal rows before r0 on entry, before r0 + rows on return.  idx (may be NULL): the list's (t, b) pairs, entry *k onwards.
void gs_load_map_chunk(const uint8_t* terminals, int64_t r0, int64_t rows, int32_t B, int32_t* k, int32_t* map, int32_t* idx);
