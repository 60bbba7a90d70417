// rollout_load.cpp -- the host side of gs_rollout_load (rollout_load.h).  Plain C++, no HIP.
#include "rollout_load.h"

#include <algorithm>
#include <cstdio>

std::string gs_load_check(const gs_rollout_source* s, int32_t B, int32_t obs_dim, int32_t action_dim, gs_rollout_load_info* out) {
  char buf[256];
  if (!s) return "gs_rollout_source is NULL";
  if (s->struct_size != (int32_t)sizeof(gs_rollout_source)) {
    snprintf(buf, sizeof buf, "gs_rollout_source.struct_size is %d, not %zu", s->struct_size, sizeof(gs_rollout_source));
    return buf;
  }
  if (B <= 0 || obs_dim <= 0 || action_dim < 0) {
    snprintf(buf, sizeof buf, "B %d, obs_dim %d, action_dim %d: not a handle's shape", B, obs_dim, action_dim);
    return buf;
  }
  if (s->dtype != GS_COMPUTE_F64 && s->dtype != GS_COMPUTE_F32) {
    snprintf(buf, sizeof buf, "gs_rollout_source.dtype %d is neither GS_COMPUTE_F64 nor GS_COMPUTE_F32", s->dtype);
    return buf;
  }
  if (s->T <= 0) { snprintf(buf, sizeof buf, "gs_rollout_source.T is %d: T <= 0", s->T); return buf; }
  if (s->chunk_rows < 0) { snprintf(buf, sizeof buf, "gs_rollout_source.chunk_rows is %d: chunk_rows < 0", s->chunk_rows); return buf; }
  if (s->flags != 0) { snprintf(buf, sizeof buf, "gs_rollout_source.flags is 0x%x: reserved, must be 0", s->flags); return buf; }
  if (!s->observations) return "gs_rollout_source.observations is NULL";
  if (!s->actions && action_dim > 0) return "gs_rollout_source.actions is NULL (only a handle with action_dim 0 may leave it out)";
  if (!s->rewards) return "gs_rollout_source.rewards is NULL";
  if (!s->next_observations) return "gs_rollout_source.next_observations is NULL";
  if (!s->terminals) return "gs_rollout_source.terminals is NULL";
  // obs_seq has T + 1 slots of B rows, and the kernels over it index rows with int32
  const int64_t n = (int64_t)s->T * B;
  if (n + B > (int64_t)INT32_MAX) {
    snprintf(buf, sizeof buf, "T * B = %lld transitions: beyond what int32 row indices hold with B = %d", (long long)n, B);
    return buf;
  }
  int32_t n_term = 0;
  for (int64_t j = 0; j < n; ++j) {
    const uint8_t f = s->terminals[j];
    if (f > 3) {
      snprintf(buf, sizeof buf, "gs_rollout_source.terminals[%lld][%lld] is %u: above 3 (bit 0 terminated, bit 1 truncated)", (long long)(j / B),
               (long long)(j % B), (unsigned)f);
      return buf;
    }
    n_term += f != 0;
  }
  if (out) { out->n = n; out->n_terminal = n_term; out->term_cap_needed = n_term; }
  return "";
}

int64_t gs_load_chunk_rows(const gs_rollout_source& s, int32_t obs_dim, int64_t n) {
  int64_t rows = s.chunk_rows;
  if (rows <= 0) rows = (int64_t)(GS_LOAD_CHUNK_BYTES / ((size_t)obs_dim * gs_load_elem(s)));
  return std::max<int64_t>(1, std::min(rows, n));
}

void gs_load_map_chunk(const uint8_t* terminals, int64_t r0, int64_t rows, int32_t B, int32_t* k, int32_t* map, int32_t* idx) {
  for (int64_t i = 0; i < rows; ++i) {
    const int64_t j = r0 + i;
    if (terminals[j] == 0) { map[i] = -1; continue; }
    if (idx) { idx[2 * (size_t)*k] = (int32_t)(j / B); idx[2 * (size_t)*k + 1] = (int32_t)(j % B); }
    map[i] = (*k)++;
  }
}
