// The host side of gs_rollout_load that needs no device (csrc/rollout_load.h: gs_load_check, gs_load_chunk_rows, gs_load_map_chunk),
// run stand-alone: every GS_E_INVALID rule, the terminal counts of hand-made flag arrays, the chunking and the ascending terminal
// list.  Prints "ok" lines; exit status 1 on the first mismatch.  tests/test_rollout_load.py builds it together with
// csrc/rollout_load.cpp under the address and undefined-behaviour sanitizers (host compile only) and runs it as a process of its own.
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "rollout_load.h"

static int failures = 0;

static void refused(const gs_rollout_source* s, int B, int D, int A, const char* needle, const char* what) {
  gs_rollout_load_info info{-1, -1, -1};
  const std::string why = gs_load_check(s, B, D, A, &info);
  if (why.empty() || why.find(needle) == std::string::npos || info.n != -1) {
    std::printf("MISMATCH %s: %s\n", what, why.empty() ? "accepted" : why.c_str());
    ++failures;
  }
}

static void counted(const gs_rollout_source& s, int B, int D, int A, int64_t n, int32_t n_term, const char* what) {
  gs_rollout_load_info info{};
  const std::string why = gs_load_check(&s, B, D, A, &info);
  if (!why.empty() || info.n != n || info.n_terminal != n_term || info.term_cap_needed != n_term) {
    std::printf("MISMATCH %s: %s n %lld n_terminal %d cap %d\n", what, why.c_str(), (long long)info.n, info.n_terminal, info.term_cap_needed);
    ++failures;
  }
}

int main() {
  static_assert(sizeof(gs_rollout_source) == 80 && sizeof(gs_rollout_load_info) == 16, "the structs of include/gridstep.h");
  const int T = 4, B = 3, D = 5, A = 2;
  std::vector<double> obs((size_t)(T + 1) * B * D, 0.5), act((size_t)T * B * A, 0.25), rew((size_t)T * B, 1.0);
  std::vector<uint8_t> term((size_t)T * B, 0);
  gs_rollout_source ok{};
  ok.struct_size = (int32_t)sizeof(gs_rollout_source); ok.dtype = GS_COMPUTE_F64; ok.T = T;
  ok.observations = obs.data(); ok.actions = act.data(); ok.rewards = rew.data(); ok.next_observations = obs.data() + (size_t)B * D; ok.terminals = term.data();

  refused(nullptr, B, D, A, "NULL", "NULL source");
  for (int sz : {0, 72, 88, -80}) { gs_rollout_source c = ok; c.struct_size = sz; refused(&c, B, D, A, "struct_size", "struct_size"); }
  for (int dt : {2, -1, 64}) { gs_rollout_source c = ok; c.dtype = dt; refused(&c, B, D, A, "dtype", "dtype"); }
  for (int t : {0, -1, std::numeric_limits<int32_t>::min()}) { gs_rollout_source c = ok; c.T = t; refused(&c, B, D, A, "T <= 0", "T"); }
  for (int r : {-1, std::numeric_limits<int32_t>::min()}) { gs_rollout_source c = ok; c.chunk_rows = r; refused(&c, B, D, A, "chunk_rows < 0", "chunk_rows"); }
  for (uint32_t f : {1u, 0x80000000u}) { gs_rollout_source c = ok; c.flags = f; refused(&c, B, D, A, "flags", "flags"); }
  { gs_rollout_source c = ok; c.observations = nullptr; refused(&c, B, D, A, "observations is NULL", "observations"); }
  { gs_rollout_source c = ok; c.actions = nullptr; refused(&c, B, D, A, "actions is NULL", "actions"); }
  { gs_rollout_source c = ok; c.rewards = nullptr; refused(&c, B, D, A, "rewards is NULL", "rewards"); }
  { gs_rollout_source c = ok; c.next_observations = nullptr; refused(&c, B, D, A, "next_observations is NULL", "next_observations"); }
  { gs_rollout_source c = ok; c.terminals = nullptr; refused(&c, B, D, A, "terminals is NULL", "terminals"); }
  // (refused before a single flag is read: the arrays behind these pointers hold T * B = 12 entries)
  { gs_rollout_source c = ok; c.T = std::numeric_limits<int32_t>::max() / B; refused(&c, B, D, A, "int32 row indices", "T * B at the limit"); }
  { gs_rollout_source c = ok; c.T = std::numeric_limits<int32_t>::max(); refused(&c, B, D, A, "int32 row indices", "T * B beyond int32"); }
  for (int v : {4, 7, 255}) {
    std::vector<uint8_t> bad(term); bad[7] = (uint8_t)v;
    gs_rollout_source c = ok; c.terminals = bad.data();
    refused(&c, B, D, A, "terminals[2][1]", "a flag above 3");
  }
  std::printf("refusals: %s\n", failures ? "FAILED" : "ok");

  const int before = failures;
  counted(ok, B, D, A, 12, 0, "all zero");
  { gs_rollout_source c = ok; c.actions = nullptr; counted(c, B, D, 0, 12, 0, "no actions on a handle without any"); }
  { gs_rollout_source c = ok; c.dtype = GS_COMPUTE_F32; c.chunk_rows = 7; c.final_observation = obs.data(); c.log_probs = rew.data(); counted(c, B, D, A, 12, 0, "float32, optional arrays"); }
  { std::vector<uint8_t> f(term.size(), 3); gs_rollout_source c = ok; c.terminals = f.data(); counted(c, B, D, A, 12, 12, "all 3"); }
  { std::vector<uint8_t> f(term); f.back() = 1; gs_rollout_source c = ok; c.terminals = f.data(); counted(c, B, D, A, 12, 1, "one flag at the last transition"); }
  { std::vector<uint8_t> f(term); f[0] = 2; f[5] = 1; f[6] = 3; gs_rollout_source c = ok; c.terminals = f.data(); counted(c, B, D, A, 12, 3, "mixed flags"); }
  std::printf("counts: %s\n", failures == before ? "ok" : "FAILED");

  // chunks: the caller's rows, the library's own by bytes, never more than there are, never fewer than one
  const int before2 = failures;
  { gs_rollout_source c = ok; c.chunk_rows = 5; if (gs_load_chunk_rows(c, D, 12) != 5) ++failures; }
  { gs_rollout_source c = ok; c.chunk_rows = 500; if (gs_load_chunk_rows(c, D, 12) != 12) ++failures; }
  if (gs_load_chunk_rows(ok, D, 12) != 12) ++failures;
  if (gs_load_chunk_rows(ok, 684, 8192 * 64) != (int64_t)(GS_LOAD_CHUNK_BYTES / (684 * 8))) ++failures;
  { gs_rollout_source c = ok; c.dtype = GS_COMPUTE_F32; if (gs_load_chunk_rows(c, 684, 8192 * 64) != (int64_t)(GS_LOAD_CHUNK_BYTES / (684 * 4))) ++failures; }
  if (gs_load_chunk_rows(ok, 1 << 30, 5) != 1) ++failures;
  if (gs_load_stage_bytes(ok, D, 5) != 5 * (D * 8 + 4)) ++failures;
  if (gs_load_lanes(1) != 8 || gs_load_lanes(32) != 8 || gs_load_lanes(33) != 16 || gs_load_lanes(71) != 32 || gs_load_lanes(684) != 64) ++failures;
  std::printf("chunks: %s\n", failures == before2 ? "ok" : "FAILED");

  // the map and the list, built chunk by chunk: ascending t * B + b whatever the chunk, chunks beginning and ending mid-step
  const int before3 = failures;
  std::vector<uint8_t> f(term);
  f[0] = 2; f[5] = 1; f[6] = 3; f[11] = 1;
  const int32_t want_idx[] = {0, 0, 1, 2, 2, 0, 3, 2}, want_map[] = {0, -1, -1, -1, -1, 1, 2, -1, -1, -1, -1, 3};
  for (int chunk : {1, 2, 5, 11, 12, 13}) {
    std::vector<int32_t> idx(8, -9), map(12, -9), part((size_t)chunk);
    int32_t k = 0;
    for (int r0 = 0; r0 < 12; r0 += chunk) {
      const int rows = 12 - r0 < chunk ? 12 - r0 : chunk;
      gs_load_map_chunk(f.data(), r0, rows, B, &k, part.data(), idx.data());
      std::memcpy(map.data() + r0, part.data(), (size_t)rows * sizeof(int32_t));
    }
    if (k != 4 || std::memcmp(idx.data(), want_idx, sizeof want_idx) || std::memcmp(map.data(), want_map, sizeof want_map)) {
      std::printf("MISMATCH map at chunk %d\n", chunk);
      ++failures;
    }
  }
  { int32_t k = 0; std::vector<int32_t> map(12); gs_load_map_chunk(term.data(), 0, 12, B, &k, map.data(), nullptr); if (k != 0) ++failures; }
  std::printf("map: %s\n", failures == before3 ? "ok" : "FAILED");
  return failures ? 1 : 0;
}
