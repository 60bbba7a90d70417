// abi_load.hip -- gs_rollout_load (include/gridstep.h "a recorded dataset as the handle's rollout"): host
// arrays become the handle's rollout.  The checks and the shape of the staging are rollout_load.cpp's (no HIP there); this file owns
// the staging buffers (gs_handle::Loader) and queues the copies and the kernels of kernels_load.hip.
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "handle.h"
#include "rollout_load.h"

using namespace gsi;

namespace gsi __attribute__((visibility("hidden"))) {

void load_release(gs_handle* h) {
  gs_handle::Loader& ld = h->ld;
  for (int s = 0; s < 2; ++s) {
    if (ld.pin[s]) { (void)hipHostFree(ld.pin[s]); ld.pin[s] = nullptr; }
    ld.dev[s].release();
    if (ld.ev_copied[s]) { (void)hipEventDestroy(ld.ev_copied[s]); ld.ev_copied[s] = nullptr; }
    if (ld.ev_used[s]) { (void)hipEventDestroy(ld.ev_used[s]); ld.ev_used[s] = nullptr; }
    ld.busy[s] = false;
  }
  if (ld.copy) { (void)hipStreamDestroy(ld.copy); ld.copy = nullptr; }
  ld.verdict.release();
  ld.bytes = 0;
}

}  // namespace gsi

namespace {

// two staging buffers of at least `bytes` each, the copy stream, the events and the verdict
int loader_ensure(gs_handle* h, size_t bytes) {
  gs_handle::Loader& ld = h->ld;
  if (!ld.copy) HIPCHK(h, hipStreamCreateWithFlags(&ld.copy, hipStreamNonBlocking));
  for (int s = 0; s < 2; ++s) {
    if (!ld.ev_copied[s]) HIPCHK(h, hipEventCreateWithFlags(&ld.ev_copied[s], hipEventDisableTiming));
    if (!ld.ev_used[s]) HIPCHK(h, hipEventCreateWithFlags(&ld.ev_used[s], hipEventDisableTiming));
  }
  int rc = ld.verdict.grow(h, 2, "the loader's verdict");
  if (rc) return rc;
  if (bytes <= ld.bytes) return GS_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipStreamSynchronize(ld.copy));
  for (int s = 0; s < 2; ++s) {
    if (ld.pin[s]) { (void)hipHostFree(ld.pin[s]); ld.pin[s] = nullptr; }
    ld.dev[s].release();
    ld.busy[s] = false;
  }
  ld.bytes = 0;
  for (int s = 0; s < 2; ++s) {
    if (hipHostMalloc((void**)&ld.pin[s], bytes, hipHostMallocDefault) != hipSuccess) {
      ld.pin[s] = nullptr; (void)hipGetLastError();
      return fail(h, GS_E_NOMEM, "the loader's staging: %zu page-locked bytes are not to be had", bytes);
    }
    if ((rc = ld.dev[s].alloc(h, bytes, "the loader's device chunk"))) return rc;
  }
  ld.bytes = bytes;
  return GS_OK;
}

// the caller's array lies in page-locked memory (hipHostMalloc, hipHostRegister): the copy engine reads it where it is
bool page_locked(const void* p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeHost;
}

// The pipeline of one staged chunk: the host fills buffer s (after whatever used it last is through), the copy stream carries it
// over, the main stream waits for that copy.  stage_begin returns the page-locked buffer to fill; stage_send queues the copy of its
// first `bytes` bytes and makes the main stream wait; the caller launches its kernel on the main stream and calls stage_end.
int stage_begin(gs_handle* h, int s, char** pin) {
  gs_handle::Loader& ld = h->ld;
  if (ld.busy[s]) { HIPCHK(h, hipEventSynchronize(ld.ev_used[s])); ld.busy[s] = false; }
  *pin = ld.pin[s];
  return GS_OK;
}
// (direct: the caller's array is page-locked itself, so its `bytes` bytes go over from where they lie and only the `tail` bytes
// behind them come from the staging buffer)
int stage_send(gs_handle* h, int s, size_t bytes, size_t tail = 0, const void* direct = nullptr) {
  gs_handle::Loader& ld = h->ld;
  if (direct) {
    HIPCHK(h, hipMemcpyAsync(ld.dev[s].p, direct, bytes, hipMemcpyHostToDevice, ld.copy));
    if (tail) HIPCHK(h, hipMemcpyAsync(ld.dev[s].p + bytes, ld.pin[s] + bytes, tail, hipMemcpyHostToDevice, ld.copy));
  } else {
    HIPCHK(h, hipMemcpyAsync(ld.dev[s].p, ld.pin[s], bytes + tail, hipMemcpyHostToDevice, ld.copy));
  }
  HIPCHK(h, hipEventRecord(ld.ev_copied[s], ld.copy));
  HIPCHK(h, hipStreamWaitEvent(h->stream, ld.ev_copied[s], 0));
  return GS_OK;
}
int stage_end(gs_handle* h, int s) {
  gs_handle::Loader& ld = h->ld;
  HIPCHK(h, hipEventRecord(ld.ev_used[s], h->stream));
  ld.busy[s] = true;
  return GS_OK;
}

// dst[0 .. count) = the source array `src` of `count` elements: float64 straight from the caller's memory, float32 through the
// staging and gs_k_load_widen; *turn: which staging buffer is next
int upload_array(gs_handle* h, const gs_rollout_source& s, const void* src, double* dst, size_t count, int* turn) {
  if (!count) return GS_OK;
  if (s.dtype == GS_COMPUTE_F64) {
    HIPCHK(h, hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return GS_OK;
  }
  const size_t per = h->ld.bytes / sizeof(float);
  const bool direct = page_locked(src);
  for (size_t at = 0; at < count; at += per) {
    const size_t n = std::min(per, count - at);
    const int b = (*turn)++ & 1;
    char* pin = nullptr;
    int rc = stage_begin(h, b, &pin);
    if (rc) return rc;
    if (!direct) memcpy(pin, (const float*)src + at, n * sizeof(float));
    if ((rc = stage_send(h, b, n * sizeof(float), 0, direct ? (const float*)src + at : nullptr))) return rc;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(gs_k_load_widen, dim3(blocks), dim3(256), 0, h->stream, (const float*)h->ld.dev[b].p, dst + at, (long long)n);
    HIPCHK(h, hipGetLastError());
    if ((rc = stage_end(h, b))) return rc;
  }
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_rollout_load_check(const gs_rollout_source* s, int32_t B, int32_t obs_dim, int32_t action_dim, gs_rollout_load_info* out) {
  const std::string why = gs_load_check(s, B, obs_dim, action_dim, out);
  return why.empty() ? GS_OK : fail(nullptr, GS_E_INVALID, "%s", why.c_str());
}

int gs_rollout_load(gs_handle* h, const gs_rollout_source* s) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  gs_rollout_load_info info{};
  const std::string why = gs_load_check(s, h->B, h->obs_dim, h->action_dim, &info);
  if (!why.empty()) return fail(h, GS_E_INVALID, "%s", why.c_str());
  GS_ENTER(h);
  const size_t B = h->B, D = h->obs_dim, A = h->action_dim, N = (size_t)info.n, elem = gs_load_elem(*s);
  const int64_t chunk_rows = gs_load_chunk_rows(*s, h->obs_dim, info.n);
  int rc = rollout_ensure(h, s->T, info.term_cap_needed);
  if (rc) return rc;
  if ((rc = loader_ensure(h, gs_load_stage_bytes(*s, h->obs_dim, chunk_rows)))) return rc;
  gs_handle::Rollout& ro = h->ro;
  gs_handle::Loader& ld = h->ld;
  if (s->log_probs && (rc = ro.logp.grow(h, (size_t)ro.T_cap * B, "the rollout's log-probabilities"))) return rc;
  // from here until the verdict the handle holds no rollout: every gate on ro.T refuses
  ro.T = 0; ro.n_term = -1; ro.logp_recorded = false;
  ro.calls += 1;
  ro.const_dirty = true;
  int turn = 0;
  if ((rc = upload_array(h, *s, s->observations, ro.obs_seq, N * D, &turn))) return rc;
  if (s->final_observation && (rc = upload_array(h, *s, s->final_observation, ro.obs_seq + N * D, B * D, &turn))) return rc;
  if ((rc = upload_array(h, *s, s->actions, ro.act, N * A, &turn))) return rc;
  if ((rc = upload_array(h, *s, s->rewards, ro.rew, N, &turn))) return rc;
  if (s->log_probs && (rc = upload_array(h, *s, s->log_probs, ro.logp, N, &turn))) return rc;
  HIPCHK(h, hipMemcpyAsync(ro.done, s->terminals, N, hipMemcpyHostToDevice, h->stream));
  const int32_t verdict0[2] = {0, INT_MAX};
  HIPCHK(h, hipMemcpyAsync(ld.verdict, verdict0, sizeof verdict0, hipMemcpyHostToDevice, h->stream));
  // next_observations, chunk by chunk: the rows, then their map entries; the terminal list's (t, b) pairs are built alongside
  std::vector<int32_t> idx((size_t)info.n_terminal * 2);
  int32_t k = 0;
  GsLoadNextArgs G{};
  G.obs_seq = ro.obs_seq; G.term_obs = ro.term_obs; G.verdict = ld.verdict; G.n = info.n; G.D = h->obs_dim; G.B = h->B;
  G.lanes = gs_load_lanes(h->obs_dim); G.term_cap = ro.term_cap; G.have_final = s->final_observation ? 1 : 0;
  const int per_block = GS_LOAD_WAVES * (64 / G.lanes);
  const bool direct = page_locked(s->next_observations);
  for (int64_t r0 = 0; r0 < info.n; r0 += chunk_rows) {
    const int64_t rows = std::min(chunk_rows, info.n - r0);
    const size_t row_bytes = (size_t)rows * D * elem;
    const int b = turn++ & 1;
    char* pin = nullptr;
    if ((rc = stage_begin(h, b, &pin))) return rc;
    const char* const from = (const char*)s->next_observations + (size_t)r0 * D * elem;
    if (!direct) memcpy(pin, from, row_bytes);
    gs_load_map_chunk(s->terminals, r0, rows, h->B, &k, (int32_t*)(pin + row_bytes), idx.data());
    if ((rc = stage_send(h, b, row_bytes, (size_t)rows * sizeof(int32_t), direct ? from : nullptr))) return rc;
    G.src = ld.dev[b].p; G.map = (const int32_t*)(ld.dev[b].p + row_bytes); G.row0 = r0; G.rows = (int32_t)rows;
    const unsigned blocks = (unsigned)std::min<int64_t>((rows + per_block - 1) / per_block, 8192);
    if (s->dtype == GS_COMPUTE_F32) hipLaunchKernelGGL(gs_k_load_next_f32, dim3(blocks), dim3(64 * GS_LOAD_WAVES), 0, h->stream, G);
    else hipLaunchKernelGGL(gs_k_load_next_f64, dim3(blocks), dim3(64 * GS_LOAD_WAVES), 0, h->stream, G);
    HIPCHK(h, hipGetLastError());
    if ((rc = stage_end(h, b))) return rc;
  }
  if (!idx.empty()) HIPCHK(h, hipMemcpyAsync(ro.term_idx, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(ro.term_count, &info.n_terminal, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  int32_t verdict[2] = {0, 0};
  HIPCHK(h, hipMemcpyAsync(verdict, ld.verdict, sizeof verdict, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ld.busy[0] = ld.busy[1] = false;
  if (verdict[0]) {
    rollout_release(h, true);
    dataset_release(h, true);
    return fail(h, GS_E_INVALID, "gs_rollout_load: %d live transition(s) whose next_observations differ from the observation that follows; the first is (t, b) = "
                "(%d, %d).  The handle holds no rollout.", verdict[0], verdict[1] / h->B, verdict[1] % h->B);
  }
  ro.T = s->T; ro.n_term = info.n_terminal; ro.logp_recorded = s->log_probs != nullptr;
  return GS_OK;
}

}  // extern "C"
