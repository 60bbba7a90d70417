// abi_debug.hip -- test aids and measurement of the C ABI (include/gridstep.h): the host schedules of the meshed member without a
// device (gs_mesh_schedule_dump*, gs_flat_newton_map_dump), cycle stamps, per-launch timing, and reads / writes of single rows.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "handle.h"
#include "mesh_schedule.h"
#include "fastmath.h"

using namespace gsi;

extern "C" {

// ---- the meshed Newton-Raphson member's host schedule, without a device (mesh_schedule.h) -------------------------------
// header[0..15]: ok, n_levels, n_rows, max_rows_per_wave, n_pivots, msg_units, n_messages, n_accumulators, max_degree,
//                unit_bytes, zero_off, dummy_off, body_off, region_bytes, sizeof(GsMeshItem), n_adj;  why: the reason when ok == 0
int gs_mesh_schedule_dump(const gs_topology* topo, int32_t zero_z_mode, int32_t nw, int32_t ni, int32_t acc_cap, int32_t unit_budget, int32_t region_base,
                          int32_t slot_bytes, int32_t* header, char* why, int32_t why_cap, void* items, int32_t* rowinfo,
                          int32_t* adj_off, double* adj_y) {
  if (!topo || !header) return fail(nullptr, GS_E_INVALID, "topology / header is NULL");
  if (topo->struct_size != (int32_t)sizeof(gs_topology)) return fail(nullptr, GS_E_INVALID, "struct_size mismatch");
  if (nw < 1 || ni < 1 || acc_cap < 1) return fail(nullptr, GS_E_INVALID, "bad arguments");
  HostTopology ht;
  const std::string err = gs_compile_topology(*topo, zero_z_mode, false, true, ht);
  if (!err.empty()) return fail(nullptr, GS_E_INVALID, "topology: %s", err.c_str());
  MeshSchedule S;
  gs_mesh_schedule(ht, nw, ni, 8, region_base, slot_bytes, acc_cap, unit_budget, S);
  const int32_t hd[16] = {S.ok ? 1 : 0, S.n_levels, S.n_rows, S.max_rows_per_wave, S.n_pivots, S.msg_units, S.n_messages, S.n_accumulators,
                          S.max_degree, S.unit_bytes, S.zero_off, S.dummy_off, S.body_off, S.region_bytes, (int32_t)sizeof(GsMeshItem), (int32_t)S.adj_off.size()};
  memcpy(header, hd, sizeof hd);
  if (why && why_cap > 0) { strncpy(why, S.why.c_str(), (size_t)why_cap - 1); why[why_cap - 1] = 0; }
  if (!S.ok) return GS_OK;
  if (items) memcpy(items, S.items.data(), S.items.size() * sizeof(MeshItem));
  if (rowinfo) memcpy(rowinfo, S.rowinfo.data(), S.rowinfo.size() * sizeof(int32_t));
  if (adj_off) memcpy(adj_off, S.adj_off.data(), S.adj_off.size() * sizeof(int32_t));
  if (adj_y) memcpy(adj_y, S.adj_y.data(), S.adj_y.size() * sizeof(double));
  return GS_OK;
}

// The same schedule in the form the kernel reads (GS_MESH_W_*): counts[4] = n_pairs, ytab doubles, adj_ent entries, item words
int gs_mesh_schedule_dump_packed(const gs_topology* topo, int32_t zero_z_mode, int32_t nw, int32_t ni, int32_t acc_cap, int32_t unit_budget, int32_t region_base,
                                 int32_t slot_bytes, int32_t* counts, int32_t* packed, int32_t* rowinfo, double* ytab, int32_t* adj_ent) {
  if (!topo || !counts) return fail(nullptr, GS_E_INVALID, "topology / counts is NULL");
  if (topo->struct_size != (int32_t)sizeof(gs_topology)) return fail(nullptr, GS_E_INVALID, "struct_size mismatch");
  HostTopology ht;
  const std::string err = gs_compile_topology(*topo, zero_z_mode, false, true, ht);
  if (!err.empty()) return fail(nullptr, GS_E_INVALID, "topology: %s", err.c_str());
  MeshSchedule S;
  gs_mesh_schedule(ht, nw, ni, 8, region_base, slot_bytes, acc_cap, unit_budget, S);
  if (!S.ok) return fail(nullptr, GS_E_TOPOLOGY, "%s", S.why.c_str());
  counts[0] = S.n_pairs; counts[1] = (int32_t)S.ytab.size(); counts[2] = (int32_t)S.adj_ent.size(); counts[3] = GS_MESH_WORDS;
  if (packed) memcpy(packed, S.packed.data(), S.packed.size() * sizeof(int32_t));
  if (rowinfo) memcpy(rowinfo, S.rowinfo_packed.data(), S.rowinfo_packed.size() * sizeof(int32_t));
  if (ytab) memcpy(ytab, S.ytab.data(), S.ytab.size() * sizeof(double));
  if (adj_ent) memcpy(adj_ent, S.adj_ent.data(), S.adj_ent.size() * sizeof(int32_t));
  return GS_OK;
}

// The flat-start Newton map of the meshed member's iteration 0 (GsF2Tables::mesh_w), host arithmetic only (no GPU): out = W as a plain
// row-major [2 (n - 1)][n] matrix (column n - 1: the constant term; rows = (d theta, d|V|) of the non-slack buses in bus order), so that
// x = W [P_spec of the non-slack buses in bus order; 1].  Test aid.  GS_E_TOPOLOGY: the network has a bus that is neither the slack nor PQ,
// or the flat-start Jacobian is singular.
int gs_flat_newton_map_dump(const gs_topology* topo, int32_t zero_z_mode, double* out) {
  if (!topo || !out) return fail(nullptr, GS_E_INVALID, "topology / out is NULL");
  if (topo->struct_size != (int32_t)sizeof(gs_topology)) return fail(nullptr, GS_E_INVALID, "struct_size mismatch");
  HostTopology ht;
  const std::string err = gs_compile_topology(*topo, zero_z_mode, false, true, ht);
  if (!err.empty()) return fail(nullptr, GS_E_INVALID, "topology: %s", err.c_str());
  for (int i = 0; i < ht.n; ++i)
    if (i != ht.slack && !(ht.th_free[i] && ht.vm_free[i])) return fail(nullptr, GS_E_TOPOLOGY, "a bus other than the slack is not a PQ bus");
  const int na = ht.n - 1, N2 = 2 * na, K = na + 1, tiles = (N2 + 15) / 16, steps = (K + 3) / 4;
  std::vector<double> wt;
  if (!flat_newton_map(ht, tiles, steps, wt)) return fail(nullptr, GS_E_TOPOLOGY, "the flat-start Jacobian is singular");
  for (int u = 0; u < N2; ++u)
    for (int k = 0; k < K; ++k) out[(size_t)u * K + k] = wt[((size_t)(u / 16) * steps + k / 4) * 64 + (u % 16) + 16 * (k % 4)];
  return GS_OK;
}

// ---- measurement ------------------------------------------------------------------------------------
int gs_debug_stamps(gs_handle* h, uint64_t* cycles_out, int32_t n) {
  if (!h || !cycles_out || n < 1 || n > 16) return fail(h, GS_E_INVALID, "bad arguments");
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (!h->d_stamps) {
    int rc = dev_alloc(h, &h->d_stamps, 16 + 2 * GS_STAMP_BLOCKS);
    if (rc) return rc;
    HIPCHK(h, hipMemset(h->d_stamps, 0, (16 + 2 * GS_STAMP_BLOCKS) * sizeof(unsigned long long)));
    h->SC.stamps = h->d_stamps;
    h->DA.stamps = h->d_stamps;
    h->SA.stamps = h->d_stamps;
    h->SC.stamp_wave = getenv("GS_STAMP_WAVE") ? atoi(getenv("GS_STAMP_WAVE")) : 0;
    h->SC.block_times = getenv("GS_STAMP_BLOCK_TIMES") ? 1 : 0;
    for (int k = 0; k < n; ++k) cycles_out[k] = 0;
    return GS_OK;
  }
  unsigned long long tmp[16];
  HIPCHK(h, hipMemcpy(tmp, h->d_stamps, sizeof tmp, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemset(h->d_stamps, 0, sizeof tmp));
  for (int k = 0; k < n; ++k) cycles_out[k] = tmp[k];
  return GS_OK;
}

// (start, end) of every workgroup of the LAST step launch on the 100 MHz real-time clock (flow2 kernels, armed by
// gs_debug_stamps with GS_STAMP_BLOCK_TIMES set); returns the pairs of the first n_blocks workgroups
int gs_debug_block_times(gs_handle* h, uint64_t* out, int32_t n_blocks) {
  if (!h || !out || n_blocks < 1 || n_blocks > GS_STAMP_BLOCKS) return fail(h, GS_E_INVALID, "bad arguments");
  if (!h->d_stamps) return fail(h, GS_E_STATE, "gs_debug_stamps has not armed the buffer");
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, h->d_stamps + 16, (size_t)n_blocks * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemset(h->d_stamps + 16, 0, (size_t)2 * GS_STAMP_BLOCKS * sizeof(unsigned long long)));
  return GS_OK;
}

int gs_timing_enable(gs_handle* h, int32_t on) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->timing = on == 1;
  h->timing_span = on == 2;
  h->span_open = false;
  h->timed_used = 0;
  return GS_OK;
}

int gs_timing_read(gs_handle* h, double* total_ms, int64_t* launches) {
  if (!h || !total_ms || !launches) return fail(h, GS_E_INVALID, "bad arguments");
  GS_ENTER(h);
  if (h->timing_span) {           // call right after the last launch of the region: the closing event goes behind it on the stream
    for (int k = 0; k < GS_K_COUNT; ++k) { total_ms[k] = 0.0; launches[k] = 0; }
    if (h->span_open) {
      HIPCHK(h, hipEventRecord(h->span_b, h->stream));
      HIPCHK(h, hipEventSynchronize(h->span_b));
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, h->span_a, h->span_b) == hipSuccess) {
        // the whole span is booked on the kernel that was launched most (the step / solve kernel of a measurement loop)
        int best = 0;
        for (int k = 1; k < GS_K_COUNT; ++k) if (h->span_launches[k] > h->span_launches[best]) best = k;
        total_ms[best] = ms;
        for (int k = 0; k < GS_K_COUNT; ++k) launches[k] = h->span_launches[k];
      }
      h->span_open = false;
    }
    return GS_OK;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < GS_K_COUNT; ++k) { total_ms[k] = 0.0; launches[k] = 0; }
  for (size_t i = 0; i < h->timed_used; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->timed[i].a, h->timed[i].b) == hipSuccess) {
      total_ms[h->timed[i].kid] += ms; launches[h->timed[i].kid] += 1;
    }
  }
  h->timed_used = 0;
  return GS_OK;
}


static int debug_rows_map(gs_handle* h, int32_t which, std::vector<int32_t>& map) {
  const GsRows& R = h->R;
  const int row0[GS_ROWS_COUNT] = {R.VM.base, R.LOAD, R.ENVLOAD.base, R.FLOW.base, R.FREQ, R.CONV, R.ITERS, R.MAXMIS, R.LOADP};
  const int stride[GS_ROWS_COUNT] = {2, 1, 2, 2, 1, 1, 1, 1, 1};
  const int width[GS_ROWS_COUNT] = {h->n, h->m, h->m, h->m, 1, 1, 1, 1, h->n_loads};
  map.resize(width[which]);
  for (int k = 0; k < width[which]; ++k) map[k] = row0[which] + stride[which] * k;
  return width[which];
}

int gs_debug_write_rows(gs_handle* h, int32_t which, const double* values) {
  if (!h || !values || which < 0 || which >= GS_ROWS_COUNT) return fail(h, GS_E_INVALID, "bad arguments");
  GS_ENTER(h);
  { int rc0 = ensure_rows(h); if (rc0) return rc0; }
  std::vector<int32_t> map;
  const int C = debug_rows_map(h, which, map);
  if (C <= 0) return GS_OK;
  if ((size_t)h->B * C > h->in_doubles) return fail(h, GS_E_INVALID, "staging buffer too small");
  DevBuf<int32_t> dmap;
  int rc = dmap.alloc(h, C, "the row map");
  if (rc) return rc;
  if (hipMemcpyAsync(dmap, map.data(), C * sizeof(int32_t), hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = fail(h, GS_E_HIP, "map upload failed");
  if (!rc) rc = unpack_from_host(h, dmap, C, values);
  const hipError_t e = hipStreamSynchronize(h->stream);      // (before `dmap` goes)
  if (!rc && e != hipSuccess) rc = fail(h, GS_E_HIP, "row write failed");
  return rc;
}

int gs_debug_read_rows(gs_handle* h, int32_t which, double* values) {
  if (!h || !values || which < 0 || which >= GS_ROWS_COUNT) return fail(h, GS_E_INVALID, "bad arguments");
  GS_ENTER(h);
  { int rc0 = ensure_rows(h); if (rc0) return rc0; }
  std::vector<int32_t> map;
  const int C = debug_rows_map(h, which, map);
  if (C <= 0) return GS_OK;
  if ((size_t)h->B * C > h->out_doubles) return fail(h, GS_E_INVALID, "staging buffer too small");
  DevBuf<int32_t> dmap;
  int rc = dmap.alloc(h, C, "the row map");
  if (rc) return rc;
  if (hipMemcpyAsync(dmap, map.data(), C * sizeof(int32_t), hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = fail(h, GS_E_HIP, "map upload failed");
  if (!rc) rc = pack_to_host(h, dmap, C, values);
  (void)hipStreamSynchronize(h->stream);      // (before `dmap` goes)
  return rc;
}

}  // extern "C"

// ---- fastmath.h on the device, element by element (tests/test_gpu_exact_math.py) ------------------------------------------
// thread i takes element i, so the caller decides which elements share a wavefront: gs_sqrt_fast's choice between its short path
// and the general square root is per wavefront
__global__ void __launch_bounds__(256) gs_k_debug_fastmath(int op, long long n, const double* __restrict__ a, const double* __restrict__ b,
                                                           double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = a[i];
  double r;
  switch (op) {
    case GS_FASTMATH_SQRT: r = gs_sqrt_fast(x); break;
    case GS_FASTMATH_DIV: r = gs_div_fast(x, b[i]); break;
    case GS_FASTMATH_LOG01: r = gs_log01(x); break;
    default: r = gs_sqrt_core(x); break;
  }
  out[i] = r;
}

extern "C" int gs_debug_fastmath(int32_t op, int64_t n, const double* in_a, const double* in_b, double* out) {
  if (op < 0 || op >= GS_FASTMATH_COUNT || n < 1 || n > (1 << 24) || !in_a || !out || (op == GS_FASTMATH_DIV && !in_b))
    return fail(nullptr, GS_E_INVALID, "bad arguments");
  const size_t bytes = (size_t)n * sizeof(double);
  double *da = nullptr, *db = nullptr, *dout = nullptr;
  bool ok = hipMalloc(&da, bytes) == hipSuccess && hipMalloc(&dout, bytes) == hipSuccess && (!in_b || hipMalloc(&db, bytes) == hipSuccess);
  ok = ok && hipMemcpy(da, in_a, bytes, hipMemcpyHostToDevice) == hipSuccess && (!in_b || hipMemcpy(db, in_b, bytes, hipMemcpyHostToDevice) == hipSuccess);
  if (ok) {
    hipLaunchKernelGGL(gs_k_debug_fastmath, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (int)op, (long long)n, da, db, dout);
    ok = hipGetLastError() == hipSuccess && hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost) == hipSuccess;
  }
  (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
  return ok ? GS_OK : fail(nullptr, GS_E_HIP, "gs_debug_fastmath: allocation, copy or launch failed");
}
