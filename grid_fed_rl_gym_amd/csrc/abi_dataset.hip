// abi_dataset.hip -- the device-resident dataset over the last rollout (include/gridstep.h "gs_dataset_*"; kernels_dataset.hip;
// DESIGN.md section 14): statistics, the terminal map, minibatch gathers.  The dataset's device buffers are made and released here.
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"

using namespace gsi;

namespace gsi __attribute__((visibility("hidden"))) {

void dataset_release(gs_handle* h, bool keep_stats) {
  gs_handle::Dataset& ds = h->ds;
  ds.part.release(); ds.map.release();
  ds.built_on = 0;
  if (keep_stats) return;
  ds.stats.release(); ds.have_stats = false;
  ds.idx.release();
  if (ds.h_idx) { (void)hipHostFree(ds.h_idx); ds.h_idx = nullptr; }
  for (DevBuf<char>& b : ds.batch) b.release();
  if (ds.ev_idx) { (void)hipEventDestroy(ds.ev_idx); ds.ev_idx = nullptr; }
  if (ds.ev_batch) { (void)hipEventDestroy(ds.ev_batch); ds.ev_batch = nullptr; }
  ds.idx_pending = false;
}

// map[0 .. N) of the last rollout's N = T * B transitions: -1, then the rollout's terminal list scattered (the list's length is read on
// the device: no host round trip).  Queued on the handle's stream; the dataset's map and the refresh's (abi_refresh.hip) are made by it.
int terminal_map_fill(gs_handle* h, int32_t* map, long long N) {
  const gs_handle::Rollout& ro = h->ro;
  hipLaunchKernelGGL(gs_k_ds_map_fill, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, map, N);
  HIPCHK(h, hipGetLastError());
  if (ro.term_cap > 0) {
    hipLaunchKernelGGL(gs_k_ds_map_scatter, dim3((unsigned)((ro.term_cap + 255) / 256)), dim3(256), 0, h->stream, map, ro.term_count.p, ro.term_idx.p,
                       ro.term_cap, ro.T, h->B);
    HIPCHK(h, hipGetLastError());
  }
  return GS_OK;
}

}  // namespace gsi

static inline int ds_ct(const gs_handle* h) { return h->obs_dim + h->action_dim + 1; }
static inline int ds_cs(const gs_handle* h) { return (ds_ct(h) + 1) & ~1; }

static int ds_stats_ensure(gs_handle* h) { return h->ds.stats.grow(h, (size_t)2 * ds_cs(h), "the dataset's statistics"); }

// the dataset is built on the rollout the handle holds now
static int ds_current(gs_handle* h, const char* who) {
  if (h->ro.T <= 0) return fail(h, GS_E_STATE, "%s: no rollout has been collected on this handle", who);
  if (h->ds.built_on == 0) return fail(h, GS_E_STATE, "%s before gs_dataset_build", who);
  if (h->ds.built_on != h->ro.calls) return fail(h, GS_E_STATE, "%s: the dataset was built on an earlier rollout (gs_dataset_build again)", who);
  return GS_OK;
}

extern "C" {

int gs_dataset_build(gs_handle* h, uint32_t flags) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if (flags & ~(uint32_t)GS_DATASET_KEEP_STATS) return fail(h, GS_E_INVALID, "gs_dataset_build: unknown flags 0x%x", flags);
  const gs_handle::Rollout& ro = h->ro;
  if (ro.T <= 0 || ro.calls == 0) return fail(h, GS_E_STATE, "gs_dataset_build: no rollout has been collected on this handle");
  const long long N = (long long)ro.T * h->B;
  if (N >= (1ll << 31)) return fail(h, GS_E_INVALID, "gs_dataset_build: %lld transitions (the dataset indexes fewer than 2^31)", N);
  const bool keep = (flags & GS_DATASET_KEEP_STATS) != 0;
  gs_handle::Dataset& ds = h->ds;
  if (keep && !ds.have_stats) return fail(h, GS_E_STATE, "gs_dataset_build(GS_DATASET_KEEP_STATS): the handle holds no statistics");
  GS_ENTER(h);
  const int D = h->obs_dim, A = h->action_dim, Ct = ds_ct(h);
  // the map (terminal_map_fill)
  ds.built_on = 0;
  int rc = ds.map.grow(h, (size_t)N, "the dataset's terminal map");
  if (rc) return rc;
  if ((rc = terminal_map_fill(h, ds.map.p, N))) return rc;
  if (!keep) {
    if ((rc = ds_stats_ensure(h))) return rc;
    const long long chunks = (N + GS_DS_ROWS_PER_CHUNK - 1) / GS_DS_ROWS_PER_CHUNK;
    if ((rc = ds.part.grow(h, (size_t)chunks * Ct * 2, "the dataset's partial statistics"))) return rc;
    GsDsStatArgs S{};
    const auto panels = [](int C) { return C <= 0 ? 0 : ((C & 1) ? (C + 63) / 64 : (C / 2 + 63) / 64); };
    S.m[0] = GsDsMatrix{ro.obs_seq, D, 0, panels(D), 0};
    S.m[1] = GsDsMatrix{ro.act, A, D, panels(A), 0};
    S.m[2] = GsDsMatrix{ro.rew, 1, D + A, 1, 0};
    S.part = ds.part; S.N = N; S.chunks = chunks; S.Ct = Ct;
    const long long blocks = (long long)(S.m[0].panels + S.m[1].panels + 1) * ((chunks + 3) / 4);
    if (blocks >= (1ll << 31)) return fail(h, GS_E_INVALID, "gs_dataset_build: %lld workgroups exceed a launch", blocks);
    hipLaunchKernelGGL(gs_k_ds_chunk_stats, dim3((unsigned)blocks), dim3(256), 0, h->stream, S);
    HIPCHK(h, hipGetLastError());
    // the merge tree, four levels (16 nodes) per launch; the launch that leaves one node files mean and std
    for (long long stride = 1;; stride *= 16) {
      const long long nodes = (chunks + stride - 1) / stride, groups = (nodes + 15) / 16;
      const bool last = groups == 1;
      const long long threads = groups * Ct;
      hipLaunchKernelGGL(gs_k_ds_merge, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, ds.part.p, chunks, Ct, stride, N,
                         S.m[0], S.m[1], S.m[2], last ? ds.stats : (double*)nullptr, last ? ds.stats + ds_cs(h) : (double*)nullptr);
      HIPCHK(h, hipGetLastError());
      if (last) break;
    }
    ds.have_stats = true;
  }
  ds.N = N;
  ds.built_on = ro.calls;
  return GS_OK;
}

int gs_dataset_stats(gs_handle* h, gs_dataset_stats_view* v) {
  if (!h || !v) return fail(h, GS_E_INVALID, "handle / view is NULL");
  if (v->struct_size != (int32_t)sizeof(gs_dataset_stats_view)) return fail(h, GS_E_INVALID, "gs_dataset_stats_view.struct_size %d != %zu", v->struct_size, sizeof(gs_dataset_stats_view));
  int rc = ds_current(h, "gs_dataset_stats");
  if (rc) return rc;
  GS_ENTER(h);
  const int D = h->obs_dim, A = h->action_dim, Cs = ds_cs(h);
  std::vector<double> st((size_t)2 * Cs);
  HIPCHK(h, hipMemcpyAsync(st.data(), h->ds.stats, st.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  v->rows_per_chunk = GS_DS_ROWS_PER_CHUNK; v->n = h->ds.N; v->obs_dim = D; v->action_dim = A;
  if (v->obs_mean) memcpy(v->obs_mean, st.data(), D * sizeof(double));
  if (v->obs_std) memcpy(v->obs_std, st.data() + Cs, D * sizeof(double));
  if (v->act_mean && A) memcpy(v->act_mean, st.data() + D, A * sizeof(double));
  if (v->act_std && A) memcpy(v->act_std, st.data() + Cs + D, A * sizeof(double));
  if (v->reward_mean) *v->reward_mean = st[D + A];
  if (v->reward_std) *v->reward_std = st[Cs + D + A];
  return GS_OK;
}

int gs_dataset_set_stats(gs_handle* h, const gs_dataset_stats_view* v) {
  if (!h || !v) return fail(h, GS_E_INVALID, "handle / view is NULL");
  if (v->struct_size != (int32_t)sizeof(gs_dataset_stats_view)) return fail(h, GS_E_INVALID, "gs_dataset_stats_view.struct_size %d != %zu", v->struct_size, sizeof(gs_dataset_stats_view));
  const int D = h->obs_dim, A = h->action_dim, Cs = ds_cs(h);
  if (v->obs_dim != D || v->action_dim != A) return fail(h, GS_E_INVALID, "gs_dataset_set_stats: sizes (%d, %d) do not match the handle's (%d, %d)", v->obs_dim, v->action_dim, D, A);
  if (!v->obs_mean || !v->obs_std || !v->reward_mean || !v->reward_std || (A > 0 && (!v->act_mean || !v->act_std)))
    return fail(h, GS_E_INVALID, "gs_dataset_set_stats: every statistic must be given");
  std::vector<double> st((size_t)2 * Cs, 0.0);
  memcpy(st.data(), v->obs_mean, D * sizeof(double)); memcpy(st.data() + Cs, v->obs_std, D * sizeof(double));
  if (A) { memcpy(st.data() + D, v->act_mean, A * sizeof(double)); memcpy(st.data() + Cs + D, v->act_std, A * sizeof(double)); }
  st[D + A] = *v->reward_mean; st[Cs + D + A] = *v->reward_std;
  for (int c = 0; c < D + A + 1; ++c) {
    if (!std::isfinite(st[c]) || !std::isfinite(st[Cs + c])) return fail(h, GS_E_INVALID, "gs_dataset_set_stats: column %d is not finite", c);
    if (st[Cs + c] < 0.0) return fail(h, GS_E_INVALID, "gs_dataset_set_stats: standard deviation of column %d is negative", c);
  }
  GS_ENTER(h);
  int rc = ds_stats_ensure(h);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(h->ds.stats, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->ds.have_stats = true;
  return GS_OK;
}

int gs_dataset_sample(gs_handle* h, int32_t n, const int64_t* indices, uint64_t seed, uint64_t draw, int32_t dtype, int32_t normalize,
                      gs_dataset_batch* out, void* consumer_stream) {
  if (!h || !out) return fail(h, GS_E_INVALID, "handle / out is NULL");
  if (n <= 0) return fail(h, GS_E_INVALID, "gs_dataset_sample: n = %d", n);
  if (dtype != GS_COMPUTE_F64 && dtype != GS_COMPUTE_F32) return fail(h, GS_E_INVALID, "gs_dataset_sample: unknown dtype %d", dtype);
  int rc = ds_current(h, "gs_dataset_sample");
  if (rc) return rc;
  gs_handle::Dataset& ds = h->ds;
  const gs_handle::Rollout& ro = h->ro;
  if (normalize && !ds.have_stats) return fail(h, GS_E_STATE, "gs_dataset_sample: the handle holds no statistics");
  const long long N = ds.N;
  if (indices)
    for (int i = 0; i < n; ++i)
      if (indices[i] < 0 || indices[i] >= N) return fail(h, GS_E_INVALID, "gs_dataset_sample: index %lld (position %d) outside [0, %lld)", (long long)indices[i], i, N);
  GS_ENTER(h);
  if ((rc = ds_stats_ensure(h))) return rc;
  const int D = h->obs_dim, A = h->action_dim;
  if (!ds.ev_idx) HIPCHK(h, hipEventCreateWithFlags(&ds.ev_idx, hipEventDisableTiming));
  if (ds.idx.cap < (size_t)n) {      // idx and its page-locked twin grow together: both, or neither is left
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ds.idx_pending = false;
    if (ds.h_idx) { (void)hipHostFree(ds.h_idx); ds.h_idx = nullptr; }
    if ((rc = ds.idx.alloc(h, (size_t)n, "the dataset's sample indices"))) return rc;
    if (hipHostMalloc((void**)&ds.h_idx, (size_t)n * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) {
      ds.h_idx = nullptr; ds.idx.release(); (void)hipGetLastError();
      return fail(h, GS_E_NOMEM, "the dataset's sample indices: %zu page-locked bytes do not fit", (size_t)n * sizeof(int32_t));
    }
  }
  // the handle's own output buffers, where the caller gave none (grown before anything of this call is queued)
  const size_t esz = dtype == GS_COMPUTE_F32 ? sizeof(float) : sizeof(double);
  const size_t widths[5] = {(size_t)D, (size_t)std::max(A, 1), 1, (size_t)D, 1};
  void** const slots[5] = {&out->observations, &out->actions, &out->rewards, &out->next_observations, &out->terminals};
  void* dst[5];
  for (int k = 0; k < 5; ++k) {
    dst[k] = *slots[k];
    if (dst[k]) continue;
    if ((rc = ds.batch[k].grow(h, (size_t)n * widths[k] * esz, "the dataset's batch"))) return rc;
    dst[k] = ds.batch[k].p;
  }
  if (indices) {
    if (ds.idx_pending) { HIPCHK(h, hipEventSynchronize(ds.ev_idx)); ds.idx_pending = false; }   // the staging copy of the call before
    for (int i = 0; i < n; ++i) ds.h_idx[i] = (int32_t)indices[i];
    HIPCHK(h, hipMemcpyAsync(ds.idx, ds.h_idx, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(ds.ev_idx, h->stream));
    ds.idx_pending = true;
  } else {
    hipLaunchKernelGGL(gs_k_ds_draw, dim3((unsigned)(((n + 3) / 4 + 255) / 256)), dim3(256), 0, h->stream, ds.idx.p, (int)n, N, seed, draw);
    HIPCHK(h, hipGetLastError());
  }
  GsDsGatherArgs G{};
  G.idx = ds.idx; G.map = ds.map;
  G.obs_seq = ro.obs_seq; G.act = ro.act; G.rew = ro.rew; G.done = ro.done; G.term_obs = ro.term_obs;
  G.stats = ds.stats;
  G.out_obs = dst[0]; G.out_act = dst[1]; G.out_rew = dst[2]; G.out_next = dst[3]; G.out_term = dst[4];
  G.N = N; G.n = n; G.B = h->B; G.D = D; G.A = A; G.Ct = ds_ct(h); G.Cs = ds_cs(h); G.term_cap = ro.term_cap; G.normalize = normalize ? 1 : 0;
  // column pairs (16-byte loads, 16- or 8-byte stores) where every row of every array starts on such a boundary
  const uintptr_t align = 2 * esz - 1;
  G.vec2 = (D % 2 == 0) && !((uintptr_t)dst[0] & align) && !((uintptr_t)dst[3] & align);
  const dim3 grid((unsigned)((n + GS_DS_GATHER_ROWS - 1) / GS_DS_GATHER_ROWS)), block(64 * GS_DS_GATHER_ROWS);
  if (dtype == GS_COMPUTE_F32) hipLaunchKernelGGL(gs_k_ds_gather_f32, grid, block, 0, h->stream, G);
  else hipLaunchKernelGGL(gs_k_ds_gather_f64, grid, block, 0, h->stream, G);
  HIPCHK(h, hipGetLastError());
  if ((rc = publish(h, h->stream, ds.ev_batch, consumer_stream))) return rc;
  for (int k = 0; k < 5; ++k) *slots[k] = dst[k];
  return GS_OK;
}

}  // extern "C"
