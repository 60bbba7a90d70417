// abi_comm.hip -- the observation all-gather of the C ABI (include/gridstep.h): gs_comm_* and gs_allgather_obs*.  Two transports
// behind the same compaction, slots, expansion and events: RCCL, resolved at run time with dlopen (the library does not link
// against it), and an in-process one among the handles of one process.  gs_comm_destroy releases the communicator and
// the gather buffers of gs_comm_init*; the exchange stream and its events stay for a later init and go with the handle (gs_destroy).
#include <dlfcn.h>

#include <cstring>
#include <string>
#include <vector>

#include "handle.h"

using namespace gsi;

namespace {

// ---- RCCL entry points resolved at run time -------------------------------------------------
typedef struct { char internal[128]; } gs_ncclUniqueId;
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

}  // namespace

extern "C" {

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
  int rc = publish(h, h->comm_stream, h->ev_full, consumer_stream);
  if (rc) return rc;
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
  dev_free(h->d_obs_full); dev_free(h->d_gather_send); dev_free(h->d_gather_recv);
  h->rank = 0; h->world = 1;
  return GS_OK;
}

}  // extern "C"
