// abi_checks.hip -- what follows a step on the device (include/gridstep.h): the linear fallback for rejected load flows
// (gs_fallback_linear, kernels_fallback.hip) and the post-step checks (gs_checks_*, kernels_checks.hip; struct gs_checks: handle.h).
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "handle.h"

using namespace gsi;

namespace {
constexpr size_t GS_CHECKS_MAX_EVENTS = 4096;
}  // namespace

extern "C" {

// ---- linear-approximation fallback ------------------------------------------------------------------
int gs_fallback_linear(gs_handle* h, const double* load_w, const double* gen_w, const double* total_load,
                       const double* total_gen, const uint8_t* mask, uint8_t* applied_out, int32_t* n_applied) {
  if (!h) return fail(nullptr, GS_E_INVALID, "handle is NULL");
  if ((load_w == nullptr) != (gen_w == nullptr)) return fail(h, GS_E_INVALID, "load_w and gen_w go together");
  if ((total_load == nullptr) != (total_gen == nullptr)) return fail(h, GS_E_INVALID, "total_load and total_gen go together");
  if (!load_w && total_load) return fail(h, GS_E_INVALID, "totals without per-bus arrays: with the device state the sums are formed on the device");
  if (!load_w && !h->was_reset) return fail(h, GS_E_STATE, "no environment state on the device: call gs_reset first or pass load_w / gen_w");
  GS_ENTER(h);
  { int rc0 = ensure_rows(h); if (rc0) return rc0; }      // only the selected instances are overwritten: the others' rows must be current
  const int B = h->B, n = h->n;
  int rc = GS_OK;
  if (!h->fb_ready) {
    const HostTopology& ht = h->topo;
    // the order in which _calculate_power_injections fills its dicts (grid_env.py:683-720): load buses by first
    // appearance in the load list, then battery buses not seen before (a charging battery adds a load entry);
    // generator buses likewise, then battery buses (a discharging battery adds a generation entry)
    auto order_of = [&](const std::vector<int32_t>& ptr, const std::vector<int32_t>& idx, int count) {
      std::vector<int32_t> bus_of(count, 0), out; std::vector<char> seen(n, 0);
      for (int i = 0; i < n; ++i) for (int p = ptr[i]; p < ptr[i + 1]; ++p) bus_of[idx[p]] = i;
      for (int d = 0; d < count; ++d) if (!seen[bus_of[d]]) { seen[bus_of[d]] = 1; out.push_back(bus_of[d]); }
      std::vector<int32_t> bat_bus(h->n_bats, 0);
      for (int i = 0; i < n; ++i) for (int p = ht.bb_ptr[i]; p < ht.bb_ptr[i + 1]; ++p) bat_bus[ht.bb_idx[p]] = i;
      for (int q = 0; q < h->n_bats; ++q) if (!seen[bat_bus[q]]) { seen[bat_bus[q]] = 1; out.push_back(bat_bus[q]); }
      return out; };
    const std::vector<int32_t> lo = order_of(ht.bl_ptr, ht.bl_idx, h->n_loads), go = order_of(ht.bg_ptr, ht.bg_idx, h->n_gens);
    if ((rc = dev_upload(h, &h->FB.load_order, lo)) || (rc = dev_upload(h, &h->FB.gen_order, go)) ||
        (rc = dev_upload(h, &h->FB.line_x, h->line_x))) return rc;
    h->FB.n_load_order = (int32_t)lo.size(); h->FB.n_gen_order = (int32_t)go.size();
    if ((rc = dev_alloc(h, &h->fb_load, (size_t)B * n)) || (rc = dev_alloc(h, &h->fb_gen, (size_t)B * n)) ||
        (rc = dev_alloc(h, &h->fb_tl, (size_t)B)) || (rc = dev_alloc(h, &h->fb_tg, (size_t)B)) ||
        (rc = dev_alloc(h, &h->fb_mask, (size_t)B)) || (rc = dev_alloc(h, &h->fb_applied, (size_t)B))) return rc;
    h->fb_ready = true;
  }
  GsFallbackArgs A = h->FB;
  A.env_mode = load_w ? 0 : 1;
  if (h->pz) { A.line_x = h->LP.x; A.line_x_stride = h->m; }       // every instance's own reactances
  if (load_w) {
    HIPCHK(h, hipMemcpyAsync(h->fb_load, load_w, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->fb_gen, gen_w, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    A.load_w = h->fb_load; A.gen_w = h->fb_gen;
    if (total_load) {
      HIPCHK(h, hipMemcpyAsync(h->fb_tl, total_load, (size_t)B * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(h->fb_tg, total_gen, (size_t)B * sizeof(double), hipMemcpyHostToDevice, h->stream));
      A.tot_load = h->fb_tl; A.tot_gen = h->fb_tg;
    }
  }
  if (mask) { HIPCHK(h, hipMemcpyAsync(h->fb_mask, mask, (size_t)B, hipMemcpyHostToDevice, h->stream)); A.mask = h->fb_mask; }
  A.applied = h->fb_applied;
  hipLaunchKernelGGL(gs_k_fallback_linear, dim3(h->groups), dim3(64), 0, h->stream, h->T, h->R, A, h->slab, B);
  HIPCHK(h, hipGetLastError());
  std::vector<int32_t> ap(B);
  HIPCHK(h, hipMemcpyAsync(ap.data(), h->fb_applied, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int32_t cnt = 0;
  for (int b = 0; b < B; ++b) { cnt += ap[b] != 0; if (applied_out) applied_out[b] = ap[b] != 0; }
  if (n_applied) *n_applied = cnt;
  return GS_OK;
}

// ---- post-step checks -------------------------------------------------------------------------------
int gs_checks_set_fused(gs_checks* c, int32_t on, int32_t want_masks) {
  if (!c) return fail(nullptr, GS_E_INVALID, "checks object is NULL");
  gs_handle* h = c->h;
  if (on && (h->n >= 65536 || h->m >= 65536)) return fail(h, GS_E_INVALID, "fused checks count in 16 bits: fewer than 65536 buses and lines");
  if (on && h->fused && h->fused != c) return fail(h, GS_E_STATE, "another checks object is already fused into this handle's step");
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  c->want_masks = want_masks != 0;
  if (on) h->fused = c; else if (h->fused == c) h->fused = nullptr;
  return GS_OK;
}

int gs_checks_create(gs_handle* h, const gs_checks_config* cfg, gs_checks** out) {
  if (!h || !cfg || !out) return fail(h, GS_E_INVALID, "handle / config / out is NULL");
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(gs_checks_config)) return fail(h, GS_E_INVALID, "gs_checks_config.struct_size mismatch");
  if (!(cfg->timestep > 0.0)) return fail(h, GS_E_INVALID, "timestep must be positive");
  if (cfg->loading_source != 0 && cfg->loading_source != 1) return fail(h, GS_E_INVALID, "loading_source must be 0 or 1");
  GS_ENTER(h);
  gs_checks* c = new gs_checks();
  c->h = h;
  GsChecksCfg& C = c->C;
  C.c_vlo = cfg->voltage_limits[0]; C.c_vhi = cfg->voltage_limits[1]; C.c_flo = cfg->frequency_limits[0]; C.c_fhi = cfg->frequency_limits[1];
  C.c_load = cfg->line_loading_limit; C.c_rocv = cfg->rate_voltage; C.c_rocf = cfg->rate_frequency; C.dt = cfg->timestep;
  C.m_vlo = cfg->mon_voltage_limits[0]; C.m_vhi = cfg->mon_voltage_limits[1]; C.m_flo = cfg->mon_frequency_limits[0]; C.m_fhi = cfg->mon_frequency_limits[1];
  C.m_load = cfg->mon_line_loading_limit; C.m_evlo = cfg->mon_emergency_voltage[0]; C.m_evhi = cfg->mon_emergency_voltage[1];
  C.m_eflo = cfg->mon_emergency_frequency[0]; C.m_efhi = cfg->mon_emergency_frequency[1];
  C.q_tol = cfg->quality_tolerance;
  C.n = h->n; C.m = h->m; C.rows_total = h->R.total;
  C.row_vm = h->R.VM.base; C.row_qload = h->R.LOAD; C.row_flow = h->R.FLOW.base;
  C.row_cload = cfg->loading_source ? h->R.ENVLOAD.base : h->R.LOAD; C.stride_cload = cfg->loading_source ? 2 : 1;
  C.row_freq = h->R.FREQ; C.row_conv = h->R.CONV; C.row_iters = h->R.ITERS; C.row_maxmis = h->R.MAXMIS;
  const size_t Bp = h->Bp, prev_n = (size_t)h->groups * (h->n + 1) * GS_LANES;
  int rc = alloc_all(h, "the checks' buffers", c->prev.want(prev_n), c->state.want(3 * Bp), c->out_i.want((size_t)GS_CI_COUNT * Bp),
                     c->out_f.want((size_t)GS_CF_COUNT * Bp), c->bus_mask.want((size_t)h->groups * h->n * GS_LANES),
                     c->line_mask.want((size_t)h->groups * h->m * GS_LANES), c->freq.want(Bp));
  if (rc) { gs_checks_destroy(c); return rc; }
  const bool ok = hipMemset(c->prev, 0, prev_n * sizeof(double)) == hipSuccess &&
                  hipMemset(c->state, 0, 3 * Bp * sizeof(int32_t)) == hipSuccess && hipMemset(c->out_i, 0, (size_t)GS_CI_COUNT * Bp * sizeof(int32_t)) == hipSuccess &&
                  hipMemset(c->out_f, 0, (size_t)GS_CF_COUNT * Bp * sizeof(double)) == hipSuccess &&
                  hipDeviceSynchronize() == hipSuccess;        // (done before the check kernels, which run on the handle's non-blocking stream)
  if (!ok) { gs_checks_destroy(c); return fail(h, GS_E_HIP, "zeroing the checks' buffers failed"); }
  *out = c;
  return GS_OK;
}

void gs_checks_destroy(gs_checks* c) {
  if (!c) return;
  if (c->h->fused == c) c->h->fused = nullptr;
  (void)hipSetDevice(c->h->device);
  (void)hipStreamSynchronize(c->h->stream);
  for (auto& e : c->ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  delete c;      // (its buffers with it: the device is current and the stream idle)
}

int gs_checks_set_frequency(gs_checks* c, const double* f) {
  if (!c) return fail(nullptr, GS_E_INVALID, "checks object is NULL");
  gs_handle* h = c->h;
  GS_ENTER(h);
  c->use_freq = f != nullptr;
  if (f) { HIPCHK(h, hipMemcpyAsync(c->freq, f, (size_t)h->B * sizeof(double), hipMemcpyHostToDevice, h->stream)); HIPCHK(h, hipStreamSynchronize(h->stream)); }
  return GS_OK;
}

int gs_checks_run(gs_checks* c) {
  if (!c) return fail(nullptr, GS_E_INVALID, "checks object is NULL");
  gs_handle* h = c->h;
  GS_ENTER(h);
  { int rc0 = ensure_rows(h); if (rc0) return rc0; }      // the kernel reads the |V| / loading / flow rows of the last step
  // HIP events only while somebody reads them (gs_checks_timing_enable), and never more than GS_CHECKS_MAX_EVENTS pairs:
  // a per-step safety check over a long run must not grow an event list without bound
  std::pair<hipEvent_t, hipEvent_t>* e = nullptr;
  if (c->timing && c->ev_used < GS_CHECKS_MAX_EVENTS) {
    if (c->ev_used == c->ev.size()) {
      hipEvent_t a, b2;
      HIPCHK(h, hipEventCreate(&a)); HIPCHK(h, hipEventCreate(&b2));
      c->ev.emplace_back(a, b2);
    }
    e = &c->ev[c->ev_used++];
    HIPCHK(h, hipEventRecord(e->first, h->stream));
  }
  hipLaunchKernelGGL(gs_k_checks, dim3(h->groups), dim3(1024), 0, h->stream, c->C, h->slab, c->use_freq ? c->freq.p : (const double*)nullptr,
                     c->prev.p, c->state.p, c->out_i.p, c->out_f.p, c->bus_mask.p, c->line_mask.p, h->B, h->Bp);
  HIPCHK(h, hipGetLastError());
  if (e) HIPCHK(h, hipEventRecord(e->second, h->stream));
  return GS_OK;
}

int gs_checks_download(gs_checks* c, const gs_checks_view* out) {
  if (!c || !out) return fail(c ? c->h : nullptr, GS_E_INVALID, "checks object / view is NULL");
  gs_handle* h = c->h;
  GS_ENTER(h);
  const size_t Bp = h->Bp, B = h->B;
  std::vector<int32_t> ti; std::vector<double> tf; std::vector<uint8_t> tb, tl;
  if (out->ints) { ti.resize((size_t)GS_CI_COUNT * Bp); HIPCHK(h, hipMemcpyAsync(ti.data(), c->out_i, ti.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream)); }
  if (out->reals) { tf.resize((size_t)GS_CF_COUNT * Bp); HIPCHK(h, hipMemcpyAsync(tf.data(), c->out_f, tf.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream)); }
  if (out->bus_mask && h->n) { tb.resize((size_t)h->groups * h->n * GS_LANES); HIPCHK(h, hipMemcpyAsync(tb.data(), c->bus_mask, tb.size(), hipMemcpyDeviceToHost, h->stream)); }
  if (out->line_mask && h->m) { tl.resize((size_t)h->groups * h->m * GS_LANES); HIPCHK(h, hipMemcpyAsync(tl.data(), c->line_mask, tl.size(), hipMemcpyDeviceToHost, h->stream)); }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (out->ints) for (int k = 0; k < GS_CI_COUNT; ++k) memcpy(out->ints + (size_t)k * B, ti.data() + (size_t)k * Bp, B * sizeof(int32_t));
  if (out->reals) for (int k = 0; k < GS_CF_COUNT; ++k) memcpy(out->reals + (size_t)k * B, tf.data() + (size_t)k * Bp, B * sizeof(double));
  auto untile = [&](const std::vector<uint8_t>& t, uint8_t* dst, int width) {     // [group][row][lane] -> [b][row]
    for (size_t b = 0; b < B; ++b) {
      const size_t g = b / GS_LANES, lane = b % GS_LANES;
      for (int r = 0; r < width; ++r) dst[b * width + r] = t[(g * width + r) * GS_LANES + lane];
    }
  };
  if (out->bus_mask && h->n) untile(tb, out->bus_mask, h->n);
  if (out->line_mask && h->m) untile(tl, out->line_mask, h->m);
  return GS_OK;
}

int gs_checks_reset(gs_checks* c, const uint8_t* mask) {
  if (!c) return fail(nullptr, GS_E_INVALID, "checks object is NULL");
  gs_handle* h = c->h;
  GS_ENTER(h);
  DevBuf<uint8_t> dmask;
  if (mask) {
    int rc = dmask.alloc(h, h->B, "the checks' reset mask");
    if (rc) return rc;
    if (hipMemcpyAsync(dmask, mask, h->B, hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail(h, GS_E_HIP, "mask upload failed");
  }
  hipLaunchKernelGGL(gs_k_checks_reset, dim3((h->B + 255) / 256), dim3(256), 0, h->stream, c->state.p, (const uint8_t*)dmask.p, h->B, h->Bp);
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(h->stream);      // (before `dmask` goes)
  if (e1 != hipSuccess || e2 != hipSuccess) return fail(h, GS_E_HIP, "checks reset failed");
  return GS_OK;
}

int gs_checks_timing_enable(gs_checks* c, int32_t on) {
  if (!c) return fail(nullptr, GS_E_INVALID, "checks object is NULL");
  GS_ENTER(c->h);
  HIPCHK(c->h, hipStreamSynchronize(c->h->stream));
  c->timing = on != 0; c->ev_used = 0;
  return GS_OK;
}

int gs_checks_timing_read(gs_checks* c, double* total_ms, int64_t* launches) {
  if (!c || !total_ms || !launches) return fail(c ? c->h : nullptr, GS_E_INVALID, "bad arguments");
  gs_handle* h = c->h;
  GS_ENTER(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *total_ms = 0.0; *launches = 0;
  for (size_t k = 0; k < c->ev_used; ++k) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev[k].first, c->ev[k].second) == hipSuccess) { *total_ms += ms; *launches += 1; }
  }
  c->ev_used = 0;
  return GS_OK;
}

}  // extern "C"
