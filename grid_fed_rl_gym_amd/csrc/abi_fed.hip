// abi_fed.hip -- the federation (include/gridstep.h "the federation"): gs_fed_create joins the learners of K
// handles of one device, gs_fed_measure / gs_fed_aggregate / gs_fed_set_global queue the kernels of kernels_fed.hip on the
// federation's own stream, ordered against the clients' streams by events, gs_fed_stats / _info / _download read what they left.
// The federation owns the global parameters and its scratch; of a client it keeps the handle and the learner's generation, and
// takes the buffers' addresses from the handle on every call.
#include <cmath>
#include <cstring>
#include <vector>

#include "fed.h"
#include "handle.h"

using namespace gsi;

static_assert(sizeof(gs_fed_round) == 64, "gs_fed_round: two int32, two pointers, three doubles, a uint64, a uint32, an int32");
static_assert(GS_FED_BLOCK == GS_TR_RED_THREADS * GS_TR_RED_PER_THREAD, "the federation's reductions take the learner's 1024 parameters a workgroup");

struct GS_HIDDEN gs_fed {
  int device = 0, net = 0, K = 0, activation = 0, blocks = 0;
  gs_handle* h[GS_FED_MAX_CLIENTS] = {};        // NULL: the client was destroyed
  uint64_t gen[GS_FED_MAX_CLIENTS] = {};        // of the client's learner at gs_fed_create
  GsFedShape S{};
  hipStream_t stream = nullptr;
  hipEvent_t ev_client[GS_FED_MAX_CLIENTS] = {}, ev_done = nullptr, ev_stage = nullptr;
  DevBuf<float> g;                              // [P] the global parameters
  DevBuf<GsFedClient> table; std::vector<GsFedClient> h_table;      // what the device holds is h_table
  DevBuf<double> blocksum, gram, stats; DevBuf<uint8_t> pairs;
  float* h_stage = nullptr; bool stage_pending = false;             // page-locked [P]: gs_fed_set_global's host parameters
  uint64_t rounds = 0;
  double last_noise_std = 0.0; uint32_t last_round = 0; int last_n = 0;
};

namespace {

GsFedClient client_of(gs_handle::Learner& L) {
  GsFedClient c{};
  c.params = L.params; c.m = L.m; c.v = L.v;
  for (int l = 0; l < L.net.n_layers; ++l) {
    c.w[l] = const_cast<float*>(L.net.L[l].w); c.b[l] = const_cast<float*>(L.net.L[l].b);
    c.t[l] = l ? const_cast<float*>(L.net.T[l].w) : nullptr;
  }
  return c;
}

// every client still holds the learner the federation was created on; else GS_E_STATE naming the client
int check_clients(gs_fed* f, const char* who) {
  for (int k = 0; k < f->K; ++k) {
    if (!f->h[k]) return fail(nullptr, GS_E_STATE, "%s: client %d was destroyed (gs_fed_destroy, then a new federation)", who, k);
    const gs_handle::Learner& L = f->h[k]->learner[f->net];
    if (!L.live) return fail(nullptr, GS_E_STATE, "%s: client %d holds no learner for %s any more (its network was installed again)", who, k, net_name(f->net));
    if (L.gen != f->gen[k]) return fail(nullptr, GS_E_STATE, "%s: the learner of client %d was created again since gs_fed_create", who, k);
  }
  return GS_OK;
}

// a list of participants: 1 <= n <= K, every index in range and named once
int check_participants(gs_fed* f, const int32_t* part, int n, const char* who) {
  if (!part) return fail(nullptr, GS_E_INVALID, "%s: participants is NULL", who);
  if (n < 1 || n > f->K) return fail(nullptr, GS_E_INVALID, "%s: %d participants outside 1 .. %d", who, n, f->K);
  bool seen[GS_FED_MAX_CLIENTS] = {};
  for (int k = 0; k < n; ++k) {
    if (part[k] < 0 || part[k] >= f->K) return fail(nullptr, GS_E_INVALID, "%s: participant %d outside 0 .. %d", who, part[k], f->K - 1);
    if (seen[part[k]]) return fail(nullptr, GS_E_INVALID, "%s: participant %d is named twice", who, part[k]);
    seen[part[k]] = true;
  }
  return GS_OK;
}

// The table of the clients' buffers as the handles hold them now; uploaded when it differs from what the device holds (it does not
// while the learners live: a learner's buffers are its own from create to drop)
int refresh_table(gs_fed* f) {
  std::vector<GsFedClient> now((size_t)f->K);
  for (int k = 0; k < f->K; ++k) now[k] = client_of(f->h[k]->learner[f->net]);
  if (!f->h_table.empty() && !memcmp(now.data(), f->h_table.data(), now.size() * sizeof(GsFedClient))) return GS_OK;
  HIPCHK(nullptr, hipStreamSynchronize(f->stream));
  HIPCHK(nullptr, hipMemcpy(f->table, now.data(), now.size() * sizeof(GsFedClient), hipMemcpyHostToDevice));
  f->h_table = now;
  return GS_OK;
}

// the federation's stream waits for what every client's stream holds
int wait_for_clients(gs_fed* f) {
  for (int k = 0; k < f->K; ++k) {
    gs_handle* h = f->h[k];
    int rc = join_streams(h);
    if (rc) return rc;
    HIPCHK(nullptr, hipEventRecord(f->ev_client[k], h->stream));
    HIPCHK(nullptr, hipStreamWaitEvent(f->stream, f->ev_client[k], 0));
  }
  return GS_OK;
}

// every client's stream waits for what the federation's stream holds
int release_clients(gs_fed* f) {
  HIPCHK(nullptr, hipEventRecord(f->ev_done, f->stream));
  for (int k = 0; k < f->K; ++k) HIPCHK(nullptr, hipStreamWaitEvent(f->h[k]->stream, f->ev_done, 0));
  return GS_OK;
}

// queues the sums of `entries` pairs of the participants `part` (pairs: device [entries][2], NULL: the diagonal) into f->gram
int launch_gram(gs_fed* f, const uint8_t* part, int n, const uint8_t* pairs, int entries, const GsFedSumArgs* coef) {
  GsFedGramArgs G{};
  G.clients = f->table; G.g = f->g; G.blocksum = f->blocksum; G.P = f->S.P; G.blocks = f->blocks; G.pairs = pairs;
  memcpy(G.part, part, (size_t)n);
  hipLaunchKernelGGL(gs_k_fed_gram, dim3(f->blocks, entries), dim3(GS_FED_RED_THREADS), 0, f->stream, G);
  HIPCHK(nullptr, hipGetLastError());
  GsFedSumArgs S = coef ? *coef : GsFedSumArgs{};
  S.blocksum = f->blocksum; S.out = f->gram; S.blocks = f->blocks; S.stats = f->stats;
  hipLaunchKernelGGL(gs_k_fed_sum, dim3(entries), dim3(GS_FED_SUM_THREADS), 0, f->stream, S);
  HIPCHK(nullptr, hipGetLastError());
  return GS_OK;
}

int launch_apply(gs_fed* f, const uint8_t* part, int n, const gs_fed_round* r) {
  GsFedApplyArgs A{};
  A.S = f->S; A.clients = f->table; A.g = f->g; A.stats = f->stats; A.n_clients = f->K; A.n = n; A.net = f->net;
  if (n) memcpy(A.part, part, (size_t)n);
  if (r) { A.noise_std = r->noise_std; A.seed = r->seed; A.round = r->round; A.reset_moments = r->reset_moments != 0; }
  hipLaunchKernelGGL(gs_k_fed_apply, dim3((f->S.P + GS_FED_APPLY_THREADS - 1) / GS_FED_APPLY_THREADS), dim3(GS_FED_APPLY_THREADS), 0, f->stream, A);
  HIPCHK(nullptr, hipGetLastError());
  return GS_OK;
}

void fed_free(gs_fed* f) {
  for (int k = 0; k < f->K; ++k) {
    if (f->h[k]) { auto& v = f->h[k]->feds; v.erase(std::remove(v.begin(), v.end(), f), v.end()); }
    if (f->ev_client[k]) (void)hipEventDestroy(f->ev_client[k]);
  }
  if (f->ev_done) (void)hipEventDestroy(f->ev_done);
  if (f->ev_stage) (void)hipEventDestroy(f->ev_stage);
  if (f->h_stage) (void)hipHostFree(f->h_stage);
  if (f->stream) (void)hipStreamDestroy(f->stream);
  delete f;      // (its DevBufs go here)
}

}  // namespace

namespace gsi __attribute__((visibility("hidden"))) {

// gs_destroy of a client: its federations lose it (every call but gs_fed_destroy is GS_E_STATE from now on).  What a federation
// queued on the client's buffers the client's stream has waited for, and gs_destroy waits for that stream.
void fed_detach(gs_handle* h) {
  for (gs_fed* f : h->feds)
    for (int k = 0; k < f->K; ++k)
      if (f->h[k] == h) f->h[k] = nullptr;
  h->feds.clear();
}

}  // namespace gsi

extern "C" {

int gs_fed_create(gs_handle* const* clients, int32_t n_clients, int32_t net, gs_fed** out) {
  if (!clients || !out) return fail(nullptr, GS_E_INVALID, "gs_fed_create: clients / out is NULL");
  *out = nullptr;
  if (n_clients < 1 || n_clients > GS_FED_MAX_CLIENTS) return fail(nullptr, GS_E_INVALID, "gs_fed_create: %d clients outside 1 .. %d", n_clients, (int)GS_FED_MAX_CLIENTS);
  if (net < 0 || net >= GS_LEARNER_COUNT) return fail(nullptr, GS_E_INVALID, "gs_fed_create: unknown net %d", net);
  for (int k = 0; k < n_clients; ++k) {
    if (!clients[k]) return fail(nullptr, GS_E_INVALID, "gs_fed_create: client %d is NULL", k);
    for (int i = 0; i < k; ++i)
      if (clients[i] == clients[k]) return fail(nullptr, GS_E_INVALID, "gs_fed_create: clients %d and %d are one handle", i, k);
    if (clients[k]->device != clients[0]->device)
      return fail(nullptr, GS_E_INVALID, "gs_fed_create: client %d lies on device %d, client 0 on device %d", k, clients[k]->device, clients[0]->device);
  }
  Installed I[GS_FED_MAX_CLIENTS]{};           // (a live learner's network is installed: every *_set* entry drops the learner first)
  for (int k = 0; k < n_clients; ++k)
    if (!clients[k]->learner[net].live || !installed(clients[k], net, I[k]))
      return fail(nullptr, GS_E_STATE, "gs_fed_create: client %d holds no learner for %s", k, net_name(net));
  const GsTrainNet& N0 = clients[0]->learner[net].net;
  const std::vector<double>& norm0 = *I[0].norm;
  for (int k = 1; k < n_clients; ++k) {
    const GsTrainNet& N = clients[k]->learner[net].net;
    bool same = N.n_layers == N0.n_layers && N.activation == N0.activation && N.P == N0.P;
    for (int l = 0; same && l <= N0.n_layers; ++l) same = N.dims[l] == N0.dims[l];
    for (int l = 0; same && l < N0.n_layers; ++l)
      same = N.L[l].kb == N0.L[l].kb && N.L[l].nt == N0.L[l].nt && N.p_off[l] == N0.p_off[l] && (!l || N.T[l].kb == N0.T[l].kb);
    if (!same) return fail(nullptr, GS_E_INVALID, "gs_fed_create: client %d differs from client 0 in layers, widths or activation", k);
    const std::vector<double>& norm = *I[k].norm;
    if (norm.size() != norm0.size() || (!norm.empty() && memcmp(norm.data(), norm0.data(), norm.size() * sizeof(double))))
      return fail(nullptr, GS_E_INVALID, "gs_fed_create: the observation normalisation of client %d differs from client 0's", k);
  }
  HIPCHK(nullptr, hipSetDevice(clients[0]->device));
  gs_fed* f = new gs_fed;
  f->device = clients[0]->device; f->net = net; f->K = n_clients; f->activation = N0.activation;
  GsFedShape& S = f->S;
  S.n_layers = N0.n_layers; S.P = N0.P;
  for (int l = 0; l <= N0.n_layers; ++l) S.dims[l] = N0.dims[l];
  for (int l = 0; l < N0.n_layers; ++l) { S.p_off[l] = N0.p_off[l]; S.kb[l] = N0.L[l].kb; S.kbt[l] = l ? N0.T[l].kb : 0; }
  f->blocks = (S.P + GS_FED_BLOCK - 1) / GS_FED_BLOCK;
  for (int k = 0; k < n_clients; ++k) { f->h[k] = nullptr; f->gen[k] = clients[k]->learner[net].gen; }
  const size_t pair_cap = (size_t)n_clients * (n_clients + 1) / 2;
  int rc = alloc_all(nullptr, "the federation's buffers", f->g.want((size_t)S.P), f->table.want((size_t)n_clients), f->blocksum.want(pair_cap * f->blocks),
                     f->gram.want(pair_cap), f->stats.want(3 * GS_FED_MAX_CLIENTS), f->pairs.want(2 * pair_cap));
  bool ok = rc == GS_OK;
  ok = ok && hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&f->ev_done, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&f->ev_stage, hipEventDisableTiming) == hipSuccess;
  for (int k = 0; ok && k < n_clients; ++k) ok = hipEventCreateWithFlags(&f->ev_client[k], hipEventDisableTiming) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&f->h_stage, (size_t)S.P * sizeof(float), hipHostMallocDefault) == hipSuccess;
  // g = client 0's master parameters, once what is queued on its stream has run
  gs_handle* h0 = clients[0];
  ok = ok && join_streams(h0) == GS_OK && hipStreamSynchronize(h0->stream) == hipSuccess;
  ok = ok && hipMemcpy(f->g, h0->learner[net].params, (size_t)S.P * sizeof(float), hipMemcpyDeviceToDevice) == hipSuccess;
  ok = ok && hipMemset(f->stats, 0, 3 * GS_FED_MAX_CLIENTS * sizeof(double)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    if (rc == GS_OK) rc = fail(nullptr, GS_E_HIP, "gs_fed_create: %s", hipGetErrorString(hipGetLastError()));
    fed_free(f);
    return rc;
  }
  for (int k = 0; k < n_clients; ++k) { f->h[k] = clients[k]; clients[k]->feds.push_back(f); }
  if ((rc = refresh_table(f))) { fed_free(f); return rc; }
  *out = f;
  return GS_OK;
}

int gs_fed_destroy(gs_fed* f) {
  if (!f) return fail(nullptr, GS_E_INVALID, "gs_fed_destroy: the federation is NULL");
  (void)hipSetDevice(f->device);
  if (f->stream) (void)hipStreamSynchronize(f->stream);
  fed_free(f);
  return GS_OK;
}

int gs_fed_info(gs_fed* f, gs_fed_info_out* out) {
  if (!f || !out) return fail(nullptr, GS_E_INVALID, "gs_fed_info: the federation / out is NULL");
  int rc = check_clients(f, "gs_fed_info");
  if (rc) return rc;
  *out = gs_fed_info_out{};
  out->n_clients = f->K; out->net = f->net; out->param_count = f->S.P; out->rounds = (int64_t)f->rounds; out->block_params = GS_FED_BLOCK;
  return GS_OK;
}

int gs_fed_set_global(gs_fed* f, const float* params) {
  if (!f) return fail(nullptr, GS_E_INVALID, "gs_fed_set_global: the federation is NULL");
  int rc = check_clients(f, "gs_fed_set_global");
  if (rc) return rc;
  HIPCHK(nullptr, hipSetDevice(f->device));
  if ((rc = refresh_table(f))) return rc;
  if (params) {
    if (f->stage_pending) HIPCHK(nullptr, hipEventSynchronize(f->ev_stage));      // (the previous upload has left the staging block)
    memcpy(f->h_stage, params, (size_t)f->S.P * sizeof(float));
    HIPCHK(nullptr, hipMemcpyAsync(f->g, f->h_stage, (size_t)f->S.P * sizeof(float), hipMemcpyHostToDevice, f->stream));
    HIPCHK(nullptr, hipEventRecord(f->ev_stage, f->stream));
    f->stage_pending = true;
  }
  if ((rc = wait_for_clients(f))) return rc;
  if ((rc = launch_apply(f, nullptr, 0, nullptr))) return rc;
  return release_clients(f);
}

int gs_fed_measure(gs_fed* f, const int32_t* participants, int32_t n, double* gram) {
  if (!f || !gram) return fail(nullptr, GS_E_INVALID, "gs_fed_measure: the federation / gram is NULL");
  int rc = check_clients(f, "gs_fed_measure");
  if (rc) return rc;
  if ((rc = check_participants(f, participants, n, "gs_fed_measure"))) return rc;
  HIPCHK(nullptr, hipSetDevice(f->device));
  if ((rc = refresh_table(f))) return rc;
  uint8_t part[GS_FED_MAX_CLIENTS] = {};
  std::vector<uint8_t> pairs;
  for (int i = 0; i < n; ++i) {
    part[i] = (uint8_t)participants[i];
    for (int k = i; k < n; ++k) { pairs.push_back((uint8_t)i); pairs.push_back((uint8_t)k); }
  }
  const int entries = (int)(pairs.size() / 2);
  std::vector<double> tri((size_t)entries);
  HIPCHK(nullptr, hipMemcpyAsync(f->pairs, pairs.data(), pairs.size(), hipMemcpyHostToDevice, f->stream));
  if ((rc = wait_for_clients(f))) return rc;
  if ((rc = launch_gram(f, part, n, f->pairs, entries, nullptr))) return rc;
  HIPCHK(nullptr, hipMemcpyAsync(tri.data(), f->gram, tri.size() * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(nullptr, hipStreamSynchronize(f->stream));
  for (int e = 0; e < entries; ++e) {
    const int i = pairs[2 * e], k = pairs[2 * e + 1];
    gram[(size_t)i * n + k] = tri[e]; gram[(size_t)k * n + i] = tri[e];
  }
  return GS_OK;
}

int gs_fed_aggregate(gs_fed* f, const gs_fed_round* r) {
  if (!f || !r) return fail(nullptr, GS_E_INVALID, "gs_fed_aggregate: the federation / round is NULL");
  if (r->struct_size != (int32_t)sizeof(gs_fed_round))
    return fail(nullptr, GS_E_INVALID, "gs_fed_round struct_size %d != %d", r->struct_size, (int)sizeof(gs_fed_round));
  int rc = check_clients(f, "gs_fed_aggregate");
  if (rc) return rc;
  const int n = r->n_participants;
  if ((rc = check_participants(f, r->participants, n, "gs_fed_aggregate"))) return rc;
  if (!r->weights) return fail(nullptr, GS_E_INVALID, "gs_fed_aggregate: weights is NULL");
  const double vals[] = {r->clip_norm, r->noise_std, r->server_lr};
  for (double x : vals)
    if (!std::isfinite(x) || x < 0.0) return fail(nullptr, GS_E_INVALID, "gs_fed_aggregate: clip_norm, noise_std and server_lr must be finite and >= 0");
  double W = 0.0;
  for (int k = 0; k < n; ++k) {
    if (!std::isfinite(r->weights[k]) || r->weights[k] < 0.0) return fail(nullptr, GS_E_INVALID, "gs_fed_aggregate: weight %d is not finite or negative", k);
    W = W + r->weights[k];
  }
  if (!(W > 0.0) || !std::isfinite(W)) return fail(nullptr, GS_E_INVALID, "gs_fed_aggregate: the weights sum to %g", W);
  HIPCHK(nullptr, hipSetDevice(f->device));
  if ((rc = refresh_table(f))) return rc;
  uint8_t part[GS_FED_MAX_CLIENTS] = {};
  GsFedSumArgs C{};
  C.coef = 1; C.clip_norm = r->clip_norm;
  for (int k = 0; k < n; ++k) { part[k] = (uint8_t)r->participants[k]; C.u[k] = r->server_lr * (r->weights[k] / W); }
  if ((rc = wait_for_clients(f))) return rc;
  if ((rc = launch_gram(f, part, n, nullptr, n, &C))) return rc;
  if ((rc = launch_apply(f, part, n, r))) return rc;
  if (r->reset_moments)
    for (int k = 0; k < f->K; ++k) f->h[k]->learner[f->net].steps = 0;
  f->rounds += 1; f->last_noise_std = r->noise_std; f->last_round = r->round; f->last_n = n;
  return release_clients(f);
}

int gs_fed_stats(gs_fed* f, gs_fed_stats_out* out) {
  if (!f || !out) return fail(nullptr, GS_E_INVALID, "gs_fed_stats: the federation / out is NULL");
  int rc = check_clients(f, "gs_fed_stats");
  if (rc) return rc;
  if (!f->rounds) return fail(nullptr, GS_E_STATE, "gs_fed_stats: no round has run");
  HIPCHK(nullptr, hipSetDevice(f->device));
  double st[3 * GS_FED_MAX_CLIENTS];
  HIPCHK(nullptr, hipMemcpyAsync(st, f->stats, sizeof(st), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(nullptr, hipStreamSynchronize(f->stream));
  *out = gs_fed_stats_out{};
  for (int k = 0; k < f->last_n; ++k) {
    out->norm[k] = st[k]; out->clip_scale[k] = st[GS_FED_MAX_CLIENTS + k]; out->coefficient[k] = st[2 * GS_FED_MAX_CLIENTS + k];
  }
  out->noise_std = f->last_noise_std; out->rounds = (int64_t)f->rounds; out->round = f->last_round; out->n = f->last_n;
  return GS_OK;
}

int gs_fed_download(gs_fed* f, float* global_params) {
  if (!f || !global_params) return fail(nullptr, GS_E_INVALID, "gs_fed_download: the federation / global_params is NULL");
  int rc = check_clients(f, "gs_fed_download");
  if (rc) return rc;
  HIPCHK(nullptr, hipSetDevice(f->device));
  HIPCHK(nullptr, hipMemcpyAsync(global_params, f->g, (size_t)f->S.P * sizeof(float), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(nullptr, hipStreamSynchronize(f->stream));
  return GS_OK;
}

}  // extern "C"
