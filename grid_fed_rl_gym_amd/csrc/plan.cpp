// plan.cpp -- host-side planning of a handle (plan.h): member selection, slab rows, work lists, second-generation tables, the
// sparse-LU level schedule, the dense block entries, the flat-start inverse Jacobians and the layout maps.
#include "plan.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <map>

#include "mesh_schedule.h"

namespace {

std::string reject(GsPlan& p, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  p.err_code = code;
  return buf;
}

// gs_describe's names of the first-generation members, in enum order (the second generation's: kStepMembers)
const char* const kSolveName[] = {"nr_tree", "nr_sparse_lu", "fbs", "nr_dense_pivot", "nr_tree_lds", "fbs_lds", "fbs_flow", "nr_dense_mfma", "nr_sparse_lds"};
static_assert(sizeof kSolveName / sizeof *kSolveName == (size_t)SolveMember::nr_sparse_lds + 1, "kSolveName");

// devices at bus i, in the reference's accumulation order (grid_env.py:689-718): GsInjRec and GsF2Rec
template <typename Rec>
void device_fields(const HostTopology& ht, int i, Rec& r) {
  r.nl = ht.bl_ptr[i + 1] - ht.bl_ptr[i]; r.ng = ht.bg_ptr[i + 1] - ht.bg_ptr[i]; r.nb = ht.bb_ptr[i + 1] - ht.bb_ptr[i];
  if (r.nl > 0) r.l0 = ht.bl_idx[ht.bl_ptr[i]];
  if (r.nl > 1) r.l1 = ht.bl_idx[ht.bl_ptr[i] + 1];
  if (r.ng > 0) r.g0 = ht.bg_idx[ht.bg_ptr[i]];
  if (r.ng > 1) r.g1 = ht.bg_idx[ht.bg_ptr[i] + 1];
  if (r.nb > 0) r.b0 = ht.bb_idx[ht.bb_ptr[i]];
  if (r.nb > 1) r.b1 = ht.bb_idx[ht.bb_ptr[i] + 1];
}

// Ji = J^-1 (both N x N, row-major) by Gauss-Jordan with partial pivoting; J is destroyed.  false: a zero or non-finite pivot.
bool gauss_jordan_inverse(std::vector<double>& J, int N, std::vector<double>& Ji) {
  Ji.assign((size_t)N * N, 0.0);
  for (int u = 0; u < N; ++u) Ji[(size_t)u * N + u] = 1.0;
  for (int c = 0; c < N; ++c) {
    int pr = c;
    for (int r = c + 1; r < N; ++r) if (std::fabs(J[(size_t)r * N + c]) > std::fabs(J[(size_t)pr * N + c])) pr = r;
    const double pv = J[(size_t)pr * N + c];
    if (!(pv != 0.0) || !std::isfinite(pv)) return false;
    if (pr != c)
      for (int k = 0; k < N; ++k) { std::swap(J[(size_t)pr * N + k], J[(size_t)c * N + k]); std::swap(Ji[(size_t)pr * N + k], Ji[(size_t)c * N + k]); }
    const double ip = 1.0 / pv;
    for (int k = 0; k < N; ++k) { J[(size_t)c * N + k] *= ip; Ji[(size_t)c * N + k] *= ip; }
    for (int r = 0; r < N; ++r) {
      if (r == c) continue;
      const double f = J[(size_t)r * N + c];
      if (f == 0.0) continue;
      for (int k = 0; k < N; ++k) { J[(size_t)r * N + k] -= f * J[(size_t)c * N + k]; Ji[(size_t)r * N + k] -= f * Ji[(size_t)c * N + k]; }
    }
  }
  return true;
}

size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// LDS carve-up shared by the second-generation members; returns the total
size_t f2_layout(const gs_topology& topo, const HostTopology& ht, GsF2Tables& F, int NW, int IW, size_t second_region_min, size_t n_table_ints,
                 int zcols, size_t z_bytes = 0) {
  const int nsl = ht.n + 3;
  const size_t SB = (size_t)(IW + 1) * 16;
  size_t off = up16((size_t)nsl * SB);
  F.off_tile = (int32_t)off;
  off += up16(std::max<size_t>({(size_t)nsl * SB, second_region_min, (size_t)ht.m * SB, (size_t)(topo.n_loads + 4) * IW * sizeof(double)}));
  F.off_anc = (int32_t)off; off += up16(n_table_ints * 4);
  F.off_z = (int32_t)off; off += up16(std::max((size_t)nsl * zcols * 8, z_bytes));
  F.off_prof = (int32_t)off; off += up16(24 * sizeof(double));
  F.env_genp = 0; F.env_curt = topo.n_gens; F.env_batp = 2 * topo.n_gens; F.env_soc = 2 * topo.n_gens + topo.n_bats;
  F.off_env = (int32_t)off; off += up16((size_t)(2 * topo.n_gens + 2 * topo.n_bats + 1) * IW * sizeof(double));
  F.off_red = (int32_t)off; off += 2 * (size_t)NW * IW * sizeof(double);
  F.off_atom = (int32_t)off; off += 8 * (size_t)IW * sizeof(unsigned long long) + 16 * (size_t)IW * sizeof(uint32_t);
  F.lds_bytes = (int32_t)off; F.n_slots = nsl; F.slack = ht.slack;
  return off;
}

// ---- the member of gs_solve, the waves per group and the first-generation LDS ----
std::string plan_solve(const gs_config& cfg, const HostTopology& ht, bool auto_w, GsPlan& p) {
  if (cfg.solver_kind == GS_SOLVER_FBS) {
    if (!ht.fbs_ok) return reject(p, GS_E_TOPOLOGY, "FBS: %s", ht.fbs_why.c_str());
    p.solve = SolveMember::fbs;
    const size_t msg_bytes = (size_t)2 * ht.max_level_width * 6 * GS_LANES * sizeof(double);
    if (msg_bytes + 24576 <= 160 * 1024 && !GS_EXPERIMENT_ENV("GS_NO_LDS_TREE")) { p.solve = SolveMember::fbs_lds; p.dyn_lds = msg_bytes; }
    // dataflow sweeps: one 16-byte-per-lane message slot and one flag word per bus in LDS, at most 8 buses per wave
    // (their state lives in registers); flat start only
    const size_t flow_bytes = (size_t)ht.n * 2 * GS_LANES * sizeof(double) + (size_t)ht.n * sizeof(int32_t);
    const int n_items = ht.is_forest ? ht.lvl_ptr[ht.n_levels] : 0;
    // its LDS footprint allows one group per CU whatever W is, so a batch of any size runs it with all 16 waves
    if (auto_w && n_items > 8 * p.W && n_items <= 8 * GS_MAX_WAVES) p.W = GS_MAX_WAVES;
    if (!cfg.fbs_warm_start && flow_bytes + 24576 <= 160 * 1024 && (n_items + p.W - 1) / p.W <= 8 && !getenv("GS_NO_FLOW")) {
      p.solve = SolveMember::fbs_flow; p.dyn_lds = flow_bytes; }
    return "";
  }
  if (cfg.solver_kind != GS_SOLVER_NR) return reject(p, GS_E_INVALID, "unknown solver_kind %d", cfg.solver_kind);
  if (cfg.linear_solver == GS_LINSOLVE_TREE && !ht.is_forest)
    return reject(p, GS_E_TOPOLOGY, "tree elimination requested but the active network has loops");
  int ls = cfg.linear_solver;
  if (ls == GS_LINSOLVE_AUTO)
    ls = (cfg.jacobian_mode == GS_JACOBIAN_AS_CODED) ? GS_LINSOLVE_DENSE_PIVOT : (ht.is_forest ? GS_LINSOLVE_TREE : GS_LINSOLVE_SPARSE_LU);
  // meshed network whose sparse block LU would fill in (more than a quarter of all blocks): dense LU on the matrix cores
  const int na_ = ht.n_active;
  const bool mfma_fits = cfg.jacobian_mode == GS_JACOBIAN_EXACT && na_ >= 1 && 2 * na_ <= 256 && !GS_EXPERIMENT_ENV("GS_NO_DENSE_MFMA");
  if (ls == GS_LINSOLVE_DENSE_MFMA && !mfma_fits)
    return reject(p, GS_E_TOPOLOGY, "dense_mfma needs the exact Jacobian and at most 128 non-slack buses (have %d)", na_);
  if (cfg.linear_solver == GS_LINSOLVE_AUTO && ls == GS_LINSOLVE_SPARSE_LU && mfma_fits && (long long)ht.lu_n_slots * 4 > (long long)na_ * na_)
    ls = GS_LINSOLVE_DENSE_MFMA;
  // meshed network with few loops: the sparse block LU of an instance in LDS, when its blocks fit beside a second workgroup's
  // (one instance: its blocks + 7 doubles per bus; the shared schedule is about 2.5 x the blocks in bytes: two instances at least)
  const size_t sparse_need = ((size_t)4 * (ht.lu_n_slots + ht.n) + (size_t)7 * ht.n) * sizeof(double);
  const bool sparse_fits = ht.has_lu && !ht.is_forest && ht.lu_n_piv > 0 && ht.n <= 256 && sparse_need <= 32 * 1024;
#if !defined(GS_BUILD_EXPERIMENTS)
  if (ls == GS_LINSOLVE_SPARSE_LDS)
    return reject(p, GS_E_INVALID, "linear_solver sparse_lds is an experiment (measured, never AUTO's choice): build the library with `make EXPERIMENTS=1`");
#endif
  if (ls == GS_LINSOLVE_SPARSE_LDS && !sparse_fits)
    return reject(p, GS_E_TOPOLOGY, "sparse_lds needs a meshed network of at most 256 buses whose block LU fits 32 KB of LDS (%zu bytes here)", sparse_need);
  // (AUTO does not take it: measured on the 123-bus feeder with 26 loops it reaches 12.9 M env-steps/s against the slab-row
  // kernel's 17.7 M -- four instances per CU, each a chain of 7-to-40-lane steps, lose to 64 instances per workgroup on full
  // lanes, bytes or not; DESIGN.md section 7.  GS_SPARSE_LDS_AUTO=1 makes AUTO take it, for measurements.)
  if (cfg.linear_solver == GS_LINSOLVE_AUTO && ls == GS_LINSOLVE_SPARSE_LU && sparse_fits && GS_EXPERIMENT_ENV("GS_SPARSE_LDS_AUTO"))
    ls = GS_LINSOLVE_SPARSE_LDS;
  p.solve = ls == GS_LINSOLVE_TREE ? SolveMember::nr_tree : ls == GS_LINSOLVE_SPARSE_LU ? SolveMember::nr_sparse_lu
          : ls == GS_LINSOLVE_DENSE_MFMA ? SolveMember::nr_dense_mfma : ls == GS_LINSOLVE_SPARSE_LDS ? SolveMember::nr_sparse_lds
          : SolveMember::nr_dense_pivot;
  // forest sweeps through LDS messages when two adjacent levels fit next to the 24 KB static block
  const size_t msg_bytes = (size_t)2 * ht.max_level_width * 6 * GS_LANES * sizeof(double);
  if (p.solve == SolveMember::nr_tree && msg_bytes + 24576 <= 160 * 1024 && !GS_EXPERIMENT_ENV("GS_NO_LDS_TREE")) {
    p.solve = SolveMember::nr_tree_lds; p.dyn_lds = msg_bytes; }
  return "";
}

// ---- rows: scratch rows are allocated only for the member that uses them (the slab is what the step streams through L2 /
// Infinity Cache, so every unused row costs residency) ----
void plan_rows(const HostTopology& ht, GsPlan& p) {
  GsRows& R = p.R;
  int r = 0;
  auto take = [&](int count) { int at = r; r += count; return at; };
  auto take_even = [&](int count) { r = (r + 1) & ~1; return take(count); };          // blocks whose entries pair up
  auto take_pair = [&](GsFam2& a, GsFam2& b2, int count) { r = (r + 1) & ~1; a.base = r; b2.base = r + 1; r += 2 * count; };
  const int n = p.n, m = p.m;
  take_pair(R.P, R.Q, n); take_pair(R.VM, R.VA, n); take_pair(R.FLOW, R.ENVLOAD, m); R.LOAD = take(m);
  R.LOSSES = take(1); R.MAXMIS = take(1); R.ITERS = take(1); R.CONV = take(1); R.STATUS = take(1);
  const SolveMember s = p.solve;
  const bool k_tree = s == SolveMember::nr_tree, k_lu = s == SolveMember::nr_sparse_lu, k_dense = s == SolveMember::nr_dense_pivot,
             k_tree_lds = s == SolveMember::nr_tree_lds, k_fbs = s == SolveMember::fbs || s == SolveMember::fbs_lds || s == SolveMember::fbs_flow;
  const bool k_rhs = k_tree || k_lu || k_dense;
  take_pair(R.E, R.F, n); take_pair(R.PC, R.QC, n);
  take_pair(R.R0, R.R1, k_rhs ? n : 0); take_pair(R.X0, R.X1, k_rhs ? n : 0);
  R.RVM = take(n);
  R.SV = take_even(k_tree || k_tree_lds ? 2 * n : 0); R.QV = take_even(k_tree ? 2 * n : 0);
  R.TB = take_even(k_tree || k_tree_lds ? 4 * n : 0); R.CB = take_even(k_tree ? 4 * n : 0);
  take_pair(R.JR, R.JI, k_fbs ? n : 0);
  R.LU = take_even(k_lu ? 4 * ht.lu_n_slots : 0);
  R.LUD = take_even(k_lu ? 4 * n : 0);
  const int dnN = ht.dn_N;
  R.DA = take(k_dense ? dnN * dnN : 0);
  R.DB = take(k_dense ? dnN : 0); R.DX = take(k_dense ? dnN : 0);
  R.DPERM = take(k_dense ? dnN : 0);
  R.TIME = take(1); R.STEP = take(1); R.VIOL = take(1); R.TOTLOSS = take(1); R.EPREW = take(1); R.FREQ = take(1);
  R.IRR = take(1); R.WIND = take(1); R.TEMP = take(1); R.CLOUD = take(1); R.SEEDLO = take(1); R.SEEDHI = take(1);
  R.SOC = take(p.n_bats); R.BATP = take(p.n_bats); R.CURT = take(p.n_gens); R.GENP = take(p.n_gens);
  R.REWARD = take(1); R.TERM = take(1); R.TRUNC = take(1); R.VMAX = take(1); R.VMIN = take(1); R.VFLAGS = take(4);
  R.ACT = take(p.action_dim); R.LOADP = take_even(p.n_loads + 1);   // written in pairs by the load-noise draws
  R.total = (r + 1) & ~1;        // rows are stored in pairs (GS_ELEM)
}

// ---- per-wave work lists of the first-generation kernels: forest items, injections, mismatch records ----
void plan_work_lists(const HostTopology& ht, GsPlan& p) {
  const int W = p.W;
  const bool flow = p.solve == SolveMember::fbs_flow;      // messages by bus index, items dealt for equal item counts per wave
  p.wl_ptr.assign(W + 1, 0);
  if (ht.is_forest) {
    const int maxw = ht.max_level_width;
    std::vector<int> owner(ht.lvl_ptr[ht.n_levels], 0);
    {
      std::vector<int> load(W, 0);
      for (int lv = 0; lv < ht.n_levels; ++lv)
        for (int t = ht.lvl_ptr[lv]; t < ht.lvl_ptr[lv + 1]; ++t) {
          int w = (t - ht.lvl_ptr[lv]) % W;
          if (flow) { w = 0; for (int v = 1; v < W; ++v) if (load[v] < load[w]) w = v; }
          owner[t] = w; ++load[w];
        }
    }
    for (int w = 0; w < W; ++w) {
      p.wl_ptr[w] = (int)p.witems.size();
      for (int lv = 0; lv < ht.n_levels; ++lv)
        for (int t = ht.lvl_ptr[lv]; t < ht.lvl_ptr[lv + 1]; ++t) {
          if (owner[t] != w) continue;
          GsItemRec r{};
          const int i = ht.lvl_bus[t], par = ht.parent[i];
          r.bus = i; r.parent = par; r.level = lv;
          r.slot = (lv & 1) * maxw + (t - ht.lvl_ptr[lv]);
          r.parent_slot = par >= 0 ? ((lv + 1) & 1) * maxw + ht.lvl_pos[par] : 0;
          r.flags = (ht.th_free[i] ? 1 : 0) | (ht.vm_free[i] ? 2 : 0) |
                    (par >= 0 && ht.th_free[par] ? 4 : 0) | (par >= 0 && ht.vm_free[par] ? 8 : 0);
          r.n_children = ht.child_ptr[i + 1] - ht.child_ptr[i];
          r.ovf0 = (int)p.ovf_slot.size();
          for (int q = 0; q < r.n_children; ++q) {
            const int ch = ht.child_idx[ht.child_ptr[i] + q];
            const int cs = flow ? ch : ((lv - 1) & 1) * maxw + ht.lvl_pos[ch];
            if (q < GS_ITEM_CHILDREN) r.child_slot[q] = cs; else p.ovf_slot.push_back(cs);
          }
          if (par >= 0) { r.g = ht.G[ht.parent_pos[i]]; r.b = ht.B[ht.parent_pos[i]]; }
          r.gd = ht.Gd[i]; r.bd = ht.Bd[i];
          if (p.solve == SolveMember::fbs_lds || flow) {       // FBS flavour: parent includes the slack, (g, b) := z = 1 / y
            const int fp = ht.fbs_parent[i], pos = ht.fbs_parent_pos[i];
            const double yr = -ht.G[pos], yi = -ht.B[pos], yd = yr * yr + yi * yi;
            r.g = yr / yd; r.b = -yi / yd;
            r.gd = yr; r.bd = yi;
            if (par < 0) { r.parent = fp; r.flags |= 16; }
          }
          p.witems.push_back(r);
        }
    }
    p.wl_ptr[W] = (int)p.witems.size();
  }

  p.wi_ptr.assign(W + 1, 0);
  for (int w = 0; w < W; ++w) {
    p.wi_ptr[w] = (int)p.winj.size();
    // dataflow sweep kernel: a wave builds the injections of the buses it solves, in item order, straight into the
    // solver's registers (a bus that is nobody's item -- the slack -- needs no injection there)
    std::vector<int> mine;
    if (flow) for (int k = p.wl_ptr[w]; k < p.wl_ptr[w + 1]; ++k) mine.push_back(p.witems[k].bus);
    else for (int i = w; i < ht.n; i += W) mine.push_back(i);
    for (int i : mine) {
      GsInjRec r{};
      r.bus = i;
      device_fields(ht, i, r);
      r.generic = (r.nl > 2 || r.ng > 2 || r.nb > 2) ? 1 : 0;
      p.winj.push_back(r);
    }
  }
  p.wi_ptr[W] = (int)p.winj.size();

  // mismatch records: each bus' Ybus row in chunks of GS_ELL_K entries (same entry order as the CSR row); buses are dealt to
  // the waves longest row first so that every wave gets about the same number of records
  p.wb_ptr.assign(W + 1, 0);
  std::vector<int> order(ht.n), nrec(ht.n);
  for (int i = 0; i < ht.n; ++i) { order[i] = i; nrec[i] = std::max(1, (ht.row_ptr[i + 1] - ht.row_ptr[i] + GS_ELL_K - 1) / GS_ELL_K); }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b2) { return nrec[a] > nrec[b2]; });
  std::vector<std::vector<int>> mine(W);
  std::vector<int> load(W, 0);
  for (int i : order) {
    int best = 0;
    for (int w = 1; w < W; ++w) if (load[w] < load[best]) best = w;
    mine[best].push_back(i); load[best] += nrec[i];
  }
  for (int w = 0; w < W; ++w) {
    p.wb_ptr[w] = (int)p.wbus.size();
    std::sort(mine[w].begin(), mine[w].end());
    for (int i : mine[w]) {
      const int p0 = ht.row_ptr[i], p1 = ht.row_ptr[i + 1];
      for (int c0 = 0; c0 < nrec[i]; ++c0) {
        GsBusRec r{};
        r.bus = i;
        r.flags = (ht.th_free[i] ? 1 : 0) | (ht.vm_free[i] ? 2 : 0) | (c0 + 1 < nrec[i] ? 4 : 0) | (c0 > 0 ? 8 : 0);
        for (int k = 0; k < GS_ELL_K; ++k) {
          const int q = p0 + c0 * GS_ELL_K + k;
          if (q < p1) { r.col[k] = ht.col[q]; r.G[k] = ht.G[q]; r.B[k] = ht.B[q]; }
          else { r.col[k] = i; r.G[k] = 0.0; r.B[k] = 0.0; }
        }
        p.wbus.push_back(r);
      }
    }
  }
  p.wb_ptr[W] = (int)p.wbus.size();
}

// ---- second-generation step kernels (kernels_flow2.hip): IW instances per workgroup, NW waves, NI buses per sub-group ----
void plan_second_gen(const gs_topology& topo, const gs_config& cfg, const HostTopology& ht, bool auto_w, GsPlan& p) {
  int max_dev = 0, max_ch = 0;
  for (int i = 0; i < ht.n; ++i) {
    max_dev = std::max({max_dev, ht.bl_ptr[i + 1] - ht.bl_ptr[i], ht.bg_ptr[i + 1] - ht.bg_ptr[i], ht.bb_ptr[i + 1] - ht.bb_ptr[i]});
    if (ht.is_forest) max_ch = std::max(max_ch, ht.child_ptr[i + 1] - ht.child_ptr[i]);
  }
  const int SL_ZERO = ht.n, SL_ONE = ht.n + 1, SL_DUMMY = ht.n + 2, nsl = ht.n + 3;
  GsF2Tables& F = p.F2;

  // -- sweep solver: one record per position of the preorder of the tree below the slack
  // (eligible wherever the first-generation dataflow kernel is, and -- with the number of waves left to the library -- for
  // feeders beyond its 128 buses)
  if (p.solve == SolveMember::fbs_flow || (cfg.solver_kind == GS_SOLVER_FBS && auto_w && !cfg.fbs_warm_start && ht.is_forest && ht.fbs_ok &&
                                           ht.lvl_ptr[ht.n_levels] > 8 * GS_MAX_WAVES && !getenv("GS_NO_FLOW"))) {
    std::string& why = p.flow2_why;
    std::vector<int> order, size(ht.n, 1), depth(ht.n, 0);
    {
      std::vector<std::vector<int>> kids(ht.n);
      std::vector<int> roots;
      for (int lv = ht.n_levels - 1; lv >= 0; --lv)
        for (int t = ht.lvl_ptr[lv]; t < ht.lvl_ptr[lv + 1]; ++t) {
          const int i = ht.lvl_bus[t], fp = ht.fbs_parent[i];
          if (fp == ht.slack) roots.push_back(i); else kids[fp].push_back(i);
        }
      std::sort(roots.begin(), roots.end());
      for (auto& k : kids) std::sort(k.begin(), k.end());
      std::vector<std::pair<int, int>> stack;
      for (int ri = (int)roots.size() - 1; ri >= 0; --ri) stack.push_back({roots[ri], 1});
      while (!stack.empty()) {
        auto [i, d] = stack.back(); stack.pop_back();
        order.push_back(i); depth[i] = d;
        for (int q = (int)kids[i].size() - 1; q >= 0; --q) stack.push_back({kids[i][q], d + 1});
      }
      for (int q = (int)order.size() - 1; q >= 0; --q) { const int i = order[q], fp = ht.fbs_parent[i]; if (fp != ht.slack) size[fp] += size[i]; }
    }
    const int N = (int)order.size();
    int max_depth = 1;
    for (int i : order) max_depth = std::max(max_depth, depth[i]);
    // forward sweep by pointer jumping, radix 4: round r adds the partial sums of the ancestors 4^r, 2 * 4^r and 3 * 4^r up
    int n_jump = 0;
    while ((1 << (2 * n_jump)) < max_depth) ++n_jump;
    n_jump = std::max(2, (n_jump + 1) & ~1);                         // even: the last round then reads the second buffer
    // small feeders: 8 instances per workgroup, the eight sub-groups of a wavefront on eight buses; 129 ... 256 buses: eight
    // buses per sub-group; default: 16 instances per workgroup, two workgroups per CU (GS_FLOW2_IW=32 asks for the
    // 32-instance member, one per CU)
    const bool small = N <= step_row(StepMember::fbs_flow2s).positions() && !getenv("GS_NO_FLOW2_SMALL");
    const bool wide = !small && N > step_row(StepMember::fbs_flow2h).positions();
    StepMember sm = small ? StepMember::fbs_flow2s : wide ? StepMember::fbs_flow2x : StepMember::fbs_flow2h;
#if defined(GS_BUILD_EXPERIMENTS)
    if (sm == StepMember::fbs_flow2h && GS_EXPERIMENT_ENV("GS_FLOW2_IW") && atoi(GS_EXPERIMENT_ENV("GS_FLOW2_IW")) == 32) sm = StepMember::fbs_flow2;
#endif
    const int NW = step_row(sm).nw, IW = step_row(sm).iw, NPOS = step_row(sm).positions();
    const size_t off = f2_layout(topo, ht, F, NW, IW, 0, (size_t)n_jump * nsl * 4, 2);
    F.n_jump = n_jump;
    if (getenv("GS_NO_FLOW2")) why = "disabled by GS_NO_FLOW2";
    else if (N > NPOS) why = "more than " + std::to_string(NPOS) + " buses below the slack";
    // (the second-generation sweeps hold their stopping criterion, the summed mismatch, in 2^-44 pu fixed point: below ~1e-10 the
    // threshold is a handful of units and every lane's rounding shows; the first-generation kernels compare in double precision)
    else if (!(cfg.tolerance >= 1e-10)) why = "tolerance below 1e-10";
    else if (N != ht.lvl_ptr[ht.n_levels]) why = "part of the forest does not hang off the slack bus";
    else if (max_dev > 2) why = "more than two devices of a kind at one bus";
    else if (off > 160 * 1024) why = "LDS tables do not fit";
    else if (ht.n < 2 || ht.m < 1 || N < 1) why = "trivial network";
    if (why.empty()) {
      p.step = sm;
      GsF2Rec idle{}; idle.bus = SL_DUMMY; idle.parent = SL_ONE; idle.last = SL_DUMMY;
      p.f2recs.assign((size_t)NPOS, idle);
      p.f2z.assign((size_t)nsl * 2, 0.0);
      p.f2anc.assign((size_t)n_jump * nsl * 4, SL_ZERO);            // [round][slot][4]: the slot's ancestors 1, 2, 3 steps of 4^round up (no ancestor: ZERO)
      std::vector<int> up1((size_t)nsl, SL_ZERO);                    // parent slot of every slot (the slack's children: ZERO)
      for (int q = 0; q < N; ++q) {
        GsF2Rec& r = p.f2recs[q];
        const int i = order[q];
        const int fp = ht.fbs_parent[i], pos = ht.fbs_parent_pos[i];
        const double yr = -ht.G[pos], yi = -ht.B[pos], yd = yr * yr + yi * yi;      // branch admittance = -Y_ip; z = 1 / y
        r.bus = i; r.parent = fp; r.flags = 1 | (fp == ht.slack ? 2 : 0); r.last = order[q + size[i] - 1]; r.level = depth[i];
        r.zr = yr / yd; r.zi = -yi / yd; r.yr = yr; r.yi = yi;
        p.f2z[2 * (size_t)i] = r.zr; p.f2z[2 * (size_t)i + 1] = r.zi;
        up1[i] = fp == ht.slack ? SL_ZERO : fp;
        device_fields(ht, i, r);
      }
      std::vector<int> step = up1;                                   // ancestor 4^round steps up
      for (int r = 0; r < n_jump; ++r) {
        for (int sidx = 0; sidx < nsl; ++sidx) {
          int a = sidx;
          for (int k = 0; k < 3; ++k) { a = step[a]; p.f2anc[((size_t)r * nsl + sidx) * 4 + k] = a; }
        }
        std::vector<int> nxt((size_t)nsl);
        for (int sidx = 0; sidx < nsl; ++sidx) nxt[sidx] = step[step[step[step[sidx]]]];
        step.swap(nxt);
      }
    }
  }

  // -- Newton-Raphson: every (wave, item) holds a group of HV = 64 / IW buses of ONE level of the tree
  if (p.solve == SolveMember::nr_tree_lds && ht.fbs_ok) {
    std::string& why = p.flow2_why;
    bool all_pq = true, off_slack = true;
    for (int i = 0; i < ht.n; ++i) {
      if (i != ht.slack && ht.lvl_pos[i] >= 0 && !(ht.th_free[i] && ht.vm_free[i])) all_pq = false;
      if (i != ht.slack && ht.lvl_pos[i] < 0) off_slack = false;                       // a bus outside the forest
      if (ht.lvl_pos[i] >= 0 && ht.parent[i] < 0 && ht.fbs_parent[i] != ht.slack) off_slack = false;
    }
    auto deal = [&](int NW, int HV, std::vector<std::vector<std::vector<int>>>& mine, std::vector<std::vector<int>>& mine_lv) {
      mine.assign(NW, {}); mine_lv.assign(NW, {});
      for (int lv = 0; lv < ht.n_levels; ++lv)
        for (int t = ht.lvl_ptr[lv]; t < ht.lvl_ptr[lv + 1]; t += HV) {
          int w = 0;
          for (int v = 1; v < NW; ++v) if (mine[v].size() < mine[w].size()) w = v;
          std::vector<int> grp;
          for (int q = 0; q < HV; ++q) grp.push_back(t + q < ht.lvl_ptr[lv + 1] ? ht.lvl_bus[t + q] : -1);
          mine[w].push_back(grp); mine_lv[w].push_back(lv);
        }
      int mx = 0;
      for (auto& v : mine) mx = std::max<int>(mx, (int)v.size());
      return mx;
    };
    std::vector<std::vector<std::vector<int>>> mine; std::vector<std::vector<int>> mine_lv;
    const StepMemberRow& rs = step_row(StepMember::nr_flow2s);
    const StepMember sm = !getenv("GS_NO_FLOW2_SMALL") && deal(rs.nw, 64 / rs.iw, mine, mine_lv) <= rs.ni ? StepMember::nr_flow2s : StepMember::nr_flow2;
    const int NW = step_row(sm).nw, NI = step_row(sm).ni, IW = step_row(sm).iw, HV = 64 / IW;
    const int max_items = deal(NW, HV, mine, mine_lv);
    const int NPOS = step_row(sm).positions(), maxw = ht.max_level_width;
    // the ring's zero entry: behind the ring's two parities and behind the K slots that share the region
    const size_t ring_entry = (size_t)3 * IW * 16;
    const int ring_zero = (int)std::max<size_t>((size_t)2 * maxw, ((size_t)nsl * (IW + 1) * 16 + ring_entry - 1) / ring_entry);
    const size_t ring_bytes = (size_t)(ring_zero + 1) * ring_entry;
    const int pos_off = (2 * (ht.n + 1) * GS_F2_CHILDREN + nsl + 3) & ~3;
    const int n_ints = pos_off + NPOS * 4;
    const size_t off = f2_layout(topo, ht, F, NW, IW, ring_bytes, (size_t)n_ints, 4);
    F.n_jump = 0; F.n_levels = ht.n_levels; F.pos_off = pos_off; F.n_anc_ints = n_ints; F.ring_zero = ring_zero;
    if (getenv("GS_NO_FLOW2")) why = "disabled by GS_NO_FLOW2";
    else if (cfg.jacobian_mode != GS_JACOBIAN_EXACT) why = "as-coded Jacobian";
    else if (!all_pq) why = "a bus below the slack is not a PQ bus";
    else if (!off_slack) why = "part of the network does not hang off the slack bus";
    else if (max_items > NI) why = "more than " + std::to_string(NI) + " bus groups per wave";
    else if (max_ch > GS_F2_CHILDREN) why = "a bus has more than " + std::to_string(GS_F2_CHILDREN) + " children";
    else if (max_dev > 2) why = "more than two devices of a kind at one bus";
    else if (off > 160 * 1024) why = "LDS tables do not fit";
    else if (ht.n < 2 || ht.m < 1) why = "trivial network";
    if (why.empty()) {
      p.step = sm;
      GsF2Rec idle{}; idle.bus = SL_DUMMY; idle.parent = SL_ONE; idle.last = SL_DUMMY; idle.level = -1;
      p.f2recs.assign((size_t)NPOS, idle);
      p.f2z.assign((size_t)nsl * 4, 0.0);
      p.f2anc.assign((size_t)n_ints, 0);
      // rows of n + 1 buses (row n: idle positions); entries beyond a bus's children name the ZERO slot / the ring's zero entry
      int32_t* child_bus = p.f2anc.data(); int32_t* child_ring = child_bus + (ht.n + 1) * GS_F2_CHILDREN; int32_t* nch = child_ring + (ht.n + 1) * GS_F2_CHILDREN;
      std::fill(child_bus, child_bus + (ht.n + 1) * GS_F2_CHILDREN, SL_ZERO);
      std::fill(child_ring, child_ring + (ht.n + 1) * GS_F2_CHILDREN, ring_zero);
      int32_t* pos_tab = p.f2anc.data() + pos_off;
      std::vector<int> level_of(ht.n, 0);
      for (int lv = 0; lv < ht.n_levels; ++lv) for (int t = ht.lvl_ptr[lv]; t < ht.lvl_ptr[lv + 1]; ++t) level_of[ht.lvl_bus[t]] = lv;
      auto ring_of = [&](int i) { return (level_of[i] & 1) * maxw + ht.lvl_pos[i]; };
      for (int i = 0; i < ht.n; ++i) {
        nch[i] = ht.child_ptr[i + 1] - ht.child_ptr[i];
        for (int q = ht.child_ptr[i]; q < ht.child_ptr[i + 1]; ++q) {
          const int c = ht.child_idx[q];
          child_bus[i * GS_F2_CHILDREN + (q - ht.child_ptr[i])] = c; child_ring[i * GS_F2_CHILDREN + (q - ht.child_ptr[i])] = ring_of(c);
        }
        if (ht.lvl_pos[i] >= 0) {
          const int pos = ht.fbs_parent_pos[i];
          p.f2z[4 * (size_t)i] = ht.G[pos]; p.f2z[4 * (size_t)i + 1] = ht.B[pos]; p.f2z[4 * (size_t)i + 2] = ht.Gd[i]; p.f2z[4 * (size_t)i + 3] = ht.Bd[i];
        }
      }
      for (int q = 0; q < NPOS; ++q) { pos_tab[4 * q] = SL_DUMMY; pos_tab[4 * q + 1] = SL_ONE; pos_tab[4 * q + 2] = 0; pos_tab[4 * q + 3] = 0; }
      for (int w = 0; w < NW; ++w)
        for (int j = 0; j < (int)mine[w].size(); ++j) {
          int grp_maxch = 0;
          for (int i : mine[w][j]) if (i >= 0) grp_maxch = std::max(grp_maxch, ht.child_ptr[i + 1] - ht.child_ptr[i]);
          for (int hh = 0; hh < HV; ++hh) {
            const int q = (w * HV + hh) * NI + j;
            GsF2Rec& r = p.f2recs[q];
            r.level = mine_lv[w][j]; r.pad1 = grp_maxch;        // most children of the group's buses
            const int i = mine[w][j][hh];
            if (i < 0) continue;
            const int fp = ht.fbs_parent[i];
            r.bus = i; r.parent = fp; r.flags = 1 | (fp == ht.slack ? 2 : 0); r.last = i;
            pos_tab[4 * q] = i; pos_tab[4 * q + 1] = fp; pos_tab[4 * q + 2] = ring_of(i); pos_tab[4 * q + 3] = fp == ht.slack ? 0 : ring_of(fp);
            device_fields(ht, i, r);
          }
        }
    }
  }

  // -- Newton-Raphson on a meshed feeder: the block LU as rows of lane items (mesh_schedule.h), 8 instances per workgroup
  if (p.solve == SolveMember::nr_sparse_lu && !ht.is_forest) {
    std::string& why = p.mesh_why;
    const StepMemberRow& row = step_row(StepMember::nr_mesh2);
    const int NW = row.nw, NI = row.ni, IW = row.iw, HV = 64 / IW;
    bool all_pq = true;
    for (int i = 0; i < ht.n; ++i) if (i != ht.slack && !(ht.th_free[i] && ht.vm_free[i])) all_pq = false;
    // every bus needs a path to the slack over the lines the Ybus holds (an open zero-impedance line is none): the block of an
    // islanded bus is exactly singular at the flat start, which the member's iteration 0 reads from a table without testing det
    std::vector<char> seen(ht.n, 0);
    {
      std::vector<int> todo{ht.slack};
      seen[ht.slack] = 1;
      while (!todo.empty()) {
        const int u = todo.back(); todo.pop_back();
        for (int q = ht.row_ptr[u]; q < ht.row_ptr[u + 1]; ++q) if (!seen[ht.col[q]]) { seen[ht.col[q]] = 1; todo.push_back(ht.col[q]); }
      }
    }
    const bool connected = std::find(seen.begin(), seen.end(), 0) == seen.end();
    const bool want_w = !getenv("GS_NR_NO_FLAT") && ht.n <= 128;         // iteration 0 as a matrix product (below)
    MeshSchedule S;
    if (getenv("GS_NO_FLOW2") || getenv("GS_NO_MESH2")) why = "disabled by GS_NO_FLOW2 / GS_NO_MESH2";
    else if (cfg.jacobian_mode != GS_JACOBIAN_EXACT) why = "as-coded Jacobian";
    else if (!all_pq) why = "a bus other than the slack is not a PQ bus";
    else if (ht.fixed_v[ht.slack] == 0) why = "no typed slack bus";
    else if (max_dev > 2) why = "more than two devices of a kind at one bus";
    else if (ht.n < 2 || ht.m < 1) why = "trivial network";
    else if (!connected) why = "island without a path to the slack";
    else {
      const int off_tile = (int)up16((size_t)nsl * (IW + 1) * 16);          // where f2_layout puts the region (below)
      // message units that leave room for a second workgroup on the CU: 80 KB less everything else the workgroup keeps in LDS
      // (an estimate: the Ybus tables' size is known only from the schedule; f2_layout below decides)
      const size_t fixed = up16((size_t)nsl * (IW + 1) * 16) + (size_t)6 * 16 * IW + (size_t)NW * 16 * 16 * IW + (size_t)nsl * IW * 8 +
                           (size_t)(ht.nnz + 8) * 8 + (size_t)(ht.nnz + nsl + 4) * 16 + 4096;
      const int unit_budget = fixed < 80 * 1024 ? (int)((80 * 1024 - fixed) / (16 * IW)) : 1;
      gs_mesh_schedule(ht, NW, NI, IW, off_tile, (IW + 1) * 16, GS_MESH_ACC, unit_budget, S);
      if (!S.ok) why = S.why;
    }
    if (why.empty()) {
      // ints staged at off_anc: every bus's neighbour list; doubles at off_z: the Ybus entries of the pairs, then of the diagonal per slot
      size_t off = f2_layout(topo, ht, F, NW, IW, (size_t)S.region_bytes, S.adj_ent.size(), 0, S.ytab.size() * sizeof(double));
      F.off_scr = (int32_t)off; off += (size_t)NW * 16 * 16 * IW;           // exchange scratch: 16 units per wave
      F.mesh_off_p = (int32_t)off; off += (size_t)nsl * IW * sizeof(double);   // P_spec by voltage slot
      F.lds_bytes = (int32_t)off;
      if (off > 160 * 1024) why = "LDS tables do not fit";
    }
    // A network the member would take, connected, whose flat-start Jacobian still does not invert on the host (up to 128 buses: the
    // W product's map): refused rather than run on a flat-start table that no iteration checks.  Beyond 128 buses no map is built
    // and the captured table is read at iteration 0 without a det test; there the connectivity rule above is the only guard.
    if (why.empty() && want_w && !flat_newton_map(ht, 16, 32, p.mesh_w)) { why = "flat-start Jacobian is singular"; p.mesh_w.clear(); }
    if (why.empty()) {
      p.step = StepMember::nr_mesh2;
      // ---- iteration 0 as a matrix product (GsF2Tables::mesh_w): the flat-start Jacobian, inverted once on the host
      if (want_w) { F.mesh_w_steps = 32; F.mesh_slack = ht.slack; }
      p.mesh_levels = S.n_levels; p.mesh_rows = S.n_rows; p.mesh_units = S.msg_units; p.mesh_messages = S.n_messages; p.mesh_accs = S.n_accumulators;
      F.n_jump = 0; F.n_levels = S.n_levels; F.pos_off = 0; F.n_anc_ints = (int32_t)S.adj_ent.size(); F.ring_zero = 0;
      F.mesh_nz = (int32_t)S.ytab.size(); F.mesh_pairs = S.n_pairs;
      p.f2anc = S.adj_ent; p.f2z = S.ytab;
      GsF2Rec idle{}; idle.bus = SL_DUMMY; idle.parent = SL_ONE; idle.last = SL_DUMMY; idle.level = -1;
      p.f2recs.assign((size_t)NW * HV * NI, idle);
      for (int w = 0; w < NW; ++w) for (int j = 0; j < NI; ++j) for (int hh = 0; hh < HV; ++hh) {
        const GsMeshItem& it = S.items[((size_t)w * NI + j) * HV + hh];
        if (!(it.flags & GS_MESH_F_PIVOT)) continue;
        GsF2Rec& r = p.f2recs[((size_t)w * HV + hh) * NI + j];        // position of (wave, sub-group, row) in the frame's numbering
        r.bus = it.bus; r.parent = SL_ONE; r.flags = 1; r.last = it.bus; r.level = S.rowinfo[((size_t)w * NI + j) * 4];
        device_fields(ht, it.bus, r);
      }
      p.mesh_items = S.packed; p.mesh_rowinfo = S.rowinfo_packed;
    }
  }

  if (p.second_gen()) {
    // buses with a voltage set point, for the kernels' flat start (the slack; the first entry travels inside the argument block)
    for (int i = 0; i < ht.n; ++i) if (ht.fixed_v[i]) { p.fs_slot.push_back(i); p.fs_val.push_back(ht.v_set[i]); }
    F.n_fixed = (int32_t)p.fs_slot.size();
    F.fixed_slot0 = p.fs_slot.empty() ? 0 : p.fs_slot[0]; F.fixed_val0 = p.fs_val.empty() ? 1.0 : p.fs_val[0];
  }
}

typedef std::vector<std::pair<int32_t, std::vector<std::pair<int32_t, int32_t>>>> LevelTargets;
// Level L of the sparse block elimination: item(t, k, slot) for every (pivot t at bus k, neighbour block slot) in pivot order, slot -1
// first (the pivot's singularity test); returns the updates by target code (>= 0 an off-diagonal slot, -1 - i the diagonal block of
// bus i, -1 - n - i the right-hand side of bus i), longest list first
template <typename Item>
LevelTargets level_targets(const HostTopology& ht, int L, Item item) {
  std::map<int32_t, std::vector<std::pair<int32_t, int32_t>>> tgt;
  for (int t = 0; t < ht.lu_n_piv; ++t) {
    if (ht.lu_piv_level[t] != L) continue;
    const int k = ht.lu_piv_bus[t];
    item(t, k, -1);
    for (int q = ht.lu_nb_ptr[t]; q < ht.lu_nb_ptr[t + 1]; ++q) {
      item(t, k, ht.lu_nb_jk[q]);
      tgt[-(1 + ht.n + ht.lu_nb_bus[q])].push_back({ht.lu_nb_jk[q], k});          // r_i -= (A_ik D_k^-1) r_k
    }
    for (int q = ht.lu_pair_ptr[t]; q < ht.lu_pair_ptr[t + 1]; ++q) tgt[ht.lu_pair_ij[q]].push_back({ht.lu_pair_ik[q], ht.lu_pair_kj[q]});
  }
  LevelTargets order(tgt.begin(), tgt.end());
  std::stable_sort(order.begin(), order.end(), [](const auto& x, const auto& y) { return x.second.size() > y.second.size(); });
  return order;
}

// ---- level schedule of the sparse block LU for the handle's W waves (kernels_solve.hip, linsolve_lu) ----
void plan_lu_schedule(const HostTopology& ht, GsPlan& p) {
  const int NL = ht.lu_n_levels, Wn = p.W;
  std::vector<std::vector<std::vector<int32_t>>> A(Wn, std::vector<std::vector<int32_t>>(NL)), Bs(Wn, std::vector<std::vector<int32_t>>(NL)),
      Cs(Wn, std::vector<std::vector<int32_t>>(NL)), Rs(Wn, std::vector<std::vector<int32_t>>(NL));
  for (int L = 0; L < NL; ++L) {
    // phase A: one item per (pivot, neighbour), plus one per pivot for the singularity test; dealt round-robin.  Phase C: the
    // level's pivots, round-robin
    int turn = 0, tc = 0;
    const LevelTargets order = level_targets(ht, L, [&](int t, int k, int slot) {
      auto& a = A[turn++ % Wn][L]; a.push_back(k); a.push_back(slot);
      if (slot < 0) Cs[tc++ % Wn][L].push_back(t);
    });
    // phase B: targets dealt to the wave with the fewest updates so far in this level
    std::vector<int> load(Wn, 0);
    for (auto& e : order) {
      int w = 0;
      for (int v = 1; v < Wn; ++v) if (load[v] < load[w]) w = v;
      load[w] += (int)e.second.size() + 1;
      auto& b = Bs[w][L];
      b.push_back(e.first); b.push_back((int32_t)e.second.size());
      for (auto& u : e.second) { b.push_back(u.first); b.push_back(u.second); }
      if (e.first < -ht.n) {      // the right-hand-side records alone: all iteration 0 needs (GsTables::lu_flat)
        auto& rr = Rs[w][L];
        rr.push_back(e.first); rr.push_back((int32_t)e.second.size());
        for (auto& u : e.second) { rr.push_back(u.first); rr.push_back(u.second); }
      }
    }
  }
  auto flatten = [&](std::vector<std::vector<std::vector<int32_t>>>& X, std::vector<int32_t>& ptr, std::vector<int32_t>& flat, int unit) {
    for (int w = 0; w < Wn; ++w) {
      for (int L = 0; L < NL; ++L) { ptr.push_back((int32_t)flat.size() / unit); flat.insert(flat.end(), X[w][L].begin(), X[w][L].end()); }
      ptr.push_back((int32_t)flat.size() / unit);
    }
  };
  flatten(A, p.lu_a_ptr, p.lu_a, 2); flatten(Bs, p.lu_b_ptr, p.lu_b, 1); flatten(Cs, p.lu_c_ptr, p.lu_c, 1); flatten(Rs, p.lu_r_ptr, p.lu_r, 1);
}

// ---- dense block LU on the matrix cores (kernels_dense.hip): unknown numbering, Jacobian blocks by column panel, launch shape,
// and the inverse of the flat-start Jacobian ----
std::string plan_dense(const gs_config& cfg, const HostTopology& ht, int cus, GsPlan& p) {
  GsDenseArgs& D = p.DA;
  p.act_of.assign(ht.n, -1);
  for (int i = 0; i < ht.n; ++i) if (ht.th_free[i] || ht.vm_free[i]) { p.act_of[i] = (int32_t)p.act_bus.size(); p.act_bus.push_back(i); }
  const std::vector<int32_t>& act_of = p.act_of;
  const int na = (int)p.act_bus.size(), NB = (2 * na + 63) / 64;
  // (panel by panel, block row by block row inside a panel: the panel form reads a panel's range, the block-row form a block's)
  p.ent_ptr.assign(NB + 1, 0); p.bent_ptr.assign((size_t)NB * NB + 1, 0);
  for (int pnl = 0; pnl < NB; ++pnl) {
    p.ent_ptr[pnl] = (int32_t)p.ent.size() / 3;
    for (int blk = 0; blk < NB; ++blk) {
      p.bent_ptr[(size_t)pnl * NB + blk] = (int32_t)p.ent.size() / 3;
      for (int i = 0; i < ht.n; ++i) {
        if (act_of[i] < 0 || (2 * act_of[i]) / 64 != blk) continue;
        for (int q = ht.row_ptr[i]; q < ht.row_ptr[i + 1]; ++q) {
          const int j = ht.col[q];
          if (act_of[j] < 0 || (2 * act_of[j]) / 64 != pnl) continue;
          p.ent.push_back(i); p.ent.push_back(j); p.ent.push_back(q);
          GsDenseEntry e{};
          e.ib = i; e.jb = j;
          e.dst = ((2 * act_of[i] - 64 * blk) * 66 + (2 * act_of[j] - 64 * pnl)) | (ht.th_free[i] ? 1 << 16 : 0) | (ht.vm_free[i] ? 1 << 17 : 0) |
                  (ht.th_free[j] ? 1 << 18 : 0) | (ht.vm_free[j] ? 1 << 19 : 0);
          e.g = i == j ? ht.Gd[i] : ht.G[q]; e.b = i == j ? ht.Bd[i] : ht.B[q];
          p.bent.push_back(e);
        }
      }
    }
  }
  if (p.bent.empty()) p.bent.push_back(GsDenseEntry{});
  p.ent_ptr[NB] = p.bent_ptr[(size_t)NB * NB] = (int32_t)p.ent.size() / 3;
  D.n = ht.n; D.na = na; D.NB = NB; D.max_it = cfg.max_iterations; D.jacobian_exact = 1; D.rows_total = p.R.total;
  D.tol = cfg.tolerance; D.alpha = cfg.acceleration_factor;
  D.R = p.R;
  // persistent grid, instances strided over it.  Block-row form: two block buffers in LDS, two workgroups per CU; panel form (GS_DENSE_PANEL=1
  // in a build with the experiments): the whole 64-column panel in LDS, one workgroup per CU
  const size_t NP = (size_t)64 * NB;
  p.dense_blockrow = !GS_EXPERIMENT_ENV("GS_DENSE_PANEL");
  if (p.dense_blockrow) {
    p.dense_grid = std::max(1, std::min(p.B, 2 * cus));
    p.dense_lds = ((size_t)2 * 64 * 66 + NP + (size_t)8 * ((ht.n + 1) & ~1) + 8) * sizeof(double);
  } else {
    p.dense_grid = std::max(1, std::min(p.B, cus));
    p.dense_lds = (NP * 66 + NP + (size_t)8 * ((ht.n + 1) & ~1) + 2 * 528 + 8) * sizeof(double);
  }
  if (p.dense_lds > 160 * 1024 - 256) return reject(p, GS_E_TOPOLOGY, "dense_mfma: %zu bytes of LDS needed", p.dense_lds);
  // the flat-start Jacobian is the same for every instance: gs_create factors it once with the solver kernel itself
  // (bit-identical to what iteration 0 of every solve would compute; GS_DENSE_NO_FLAT=1 keeps it per solve)
  p.dense_flat = !getenv("GS_DENSE_NO_FLAT");
  // ---- and its inverse, for iteration 0 as one product (GsDenseArgs::jinv_t): the same entries as the kernel's assembly
  // (power_flow.py:243-287, exact sign; fixed components and padding unknowns: identity rows and columns), flat start
  if (p.dense_flat && p.dense_blockrow) {
    const int n_ = ht.n, NPd = 64 * NB;
    std::vector<double> v0(n_, 1.0), Pc(n_, 0.0), Qc(n_, 0.0), Jm((size_t)NPd * NPd, 0.0), Ji;
    for (int i = 0; i < n_; ++i) if (ht.fixed_v[i]) v0[i] = ht.v_set[i];
    for (int i = 0; i < n_; ++i)
      for (int q = ht.row_ptr[i]; q < ht.row_ptr[i + 1]; ++q) {
        const int j = ht.col[q];
        Pc[i] += v0[i] * v0[j] * ht.G[q]; Qc[i] -= v0[i] * v0[j] * ht.B[q];
      }
    for (int u = 0; u < NPd; ++u) Jm[(size_t)u * NPd + u] = 1.0;              // padding / fixed components
    for (int i = 0; i < n_; ++i) {
      const int a = act_of[i];
      if (a < 0) continue;
      const bool thi = ht.th_free[i] != 0, vfi = ht.vm_free[i] != 0;
      const double vi = v0[i], vvb = vi * vi * ht.Bd[i];
      Jm[(size_t)(2 * a) * NPd + 2 * a] = thi ? (-Qc[i] - vvb) : 1.0;
      Jm[(size_t)(2 * a) * NPd + 2 * a + 1] = (thi && vfi) ? (Pc[i] / vi + vi * ht.Gd[i]) : 0.0;
      Jm[(size_t)(2 * a + 1) * NPd + 2 * a] = (thi && vfi) ? (Pc[i] - vi * vi * ht.Gd[i]) : 0.0;
      Jm[(size_t)(2 * a + 1) * NPd + 2 * a + 1] = vfi ? (Qc[i] / vi - vi * ht.Bd[i]) : 1.0;
      for (int q = ht.row_ptr[i]; q < ht.row_ptr[i + 1]; ++q) {
        const int j = ht.col[q];
        if (j == i || act_of[j] < 0) continue;
        const int aj = act_of[j];
        const bool thj = ht.th_free[j] != 0, vfj = ht.vm_free[j] != 0;
        const double aa = vi * v0[j], gs_bc = -ht.B[q] * aa, gc_bs = ht.G[q] * aa;
        if (thi && thj) Jm[(size_t)(2 * a) * NPd + 2 * aj] = gs_bc;
        if (thi && vfj) Jm[(size_t)(2 * a) * NPd + 2 * aj + 1] = gc_bs / v0[j];
        if (vfi && thj) Jm[(size_t)(2 * a + 1) * NPd + 2 * aj] = -gc_bs;
        if (vfi && vfj) Jm[(size_t)(2 * a + 1) * NPd + 2 * aj + 1] = gs_bc / v0[j];
      }
    }
    if (gauss_jordan_inverse(Jm, NPd, Ji)) {
      p.jinv_t.resize((size_t)NPd * NPd);
      for (int u = 0; u < NPd; ++u)
        for (int c = 0; c < NPd; ++c) p.jinv_t[(size_t)c * NPd + u] = Ji[(size_t)u * NPd + c];
    }
  }
  return "";
}

#if defined(GS_BUILD_EXPERIMENTS)
// ---- sparse block LU in LDS (kernels_sparse.hip): the level schedule without the split over waves, packed for LDS ----
std::string plan_sparse_lds(const gs_config& cfg, const HostTopology& ht, int cus, GsPlan& p) {
  GsSparseArgs& Sp = p.SA;
  const int NL = ht.lu_n_levels;
  std::vector<int32_t> a_ptr{0}, a, b_ptr{0}, b_rec, b_pair, r_ptr{0}, r_rec, r_pair, c_ptr{0}, cc;
  for (int L = 0; L < NL; ++L) {
    // (the records longest first: the lanes of one pass then carry records of similar length)
    const LevelTargets order = level_targets(ht, L, [&](int t, int k, int slot) { a.push_back(k); a.push_back(slot); if (slot < 0) cc.push_back(t); });
    for (auto& e : order) {
      b_rec.push_back(e.first); b_rec.push_back((int32_t)e.second.size()); b_rec.push_back((int32_t)b_pair.size() / 2);
      for (auto& u : e.second) { b_pair.push_back(u.first); b_pair.push_back(u.second); }
      if (e.first < -ht.n) {
        r_rec.push_back(e.first); r_rec.push_back((int32_t)e.second.size()); r_rec.push_back((int32_t)r_pair.size() / 2);
        for (auto& u : e.second) { r_pair.push_back(u.first); r_pair.push_back(u.second); }
      }
    }
    a_ptr.push_back((int32_t)a.size() / 2); b_ptr.push_back((int32_t)b_rec.size() / 3); r_ptr.push_back((int32_t)r_rec.size() / 3);
    c_ptr.push_back((int32_t)cc.size());
  }
  Sp.n = ht.n; Sp.n_slots = ht.lu_n_slots; Sp.n_orig = ht.lu_n_orig; Sp.n_piv = ht.lu_n_piv; Sp.n_levels = NL;
  Sp.max_it = cfg.max_iterations; Sp.jacobian_exact = cfg.jacobian_mode == GS_JACOBIAN_EXACT ? 1 : 0; Sp.rows_total = p.R.total;
  Sp.tol = cfg.tolerance; Sp.alpha = cfg.acceleration_factor;
  // one packed copy of everything the elimination chases pointers through: staged into LDS once per workgroup
  auto addi = [&](const std::vector<int32_t>& v) { const int32_t o = (int32_t)p.ipack.size(); p.ipack.insert(p.ipack.end(), v.begin(), v.end()); return o; };
  auto addd = [&](const std::vector<double>& v) { const int32_t o = (int32_t)p.dpack.size(); p.dpack.insert(p.dpack.end(), v.begin(), v.end()); return o; };
  Sp.o_row_ptr = addi(ht.row_ptr); Sp.o_col = addi(ht.col); Sp.o_th_free = addi(ht.th_free); Sp.o_vm_free = addi(ht.vm_free); Sp.o_fixed_v = addi(ht.fixed_v);
  Sp.o_piv_bus = addi(ht.lu_piv_bus); Sp.o_nb_ptr = addi(ht.lu_nb_ptr); Sp.o_nb_bus = addi(ht.lu_nb_bus); Sp.o_nb_kj = addi(ht.lu_nb_kj);
  Sp.o_a_ptr = addi(a_ptr); Sp.o_a = addi(a); Sp.o_b_ptr = addi(b_ptr); Sp.o_b_rec = addi(b_rec); Sp.o_b_pair = addi(b_pair);
  Sp.o_r_ptr = addi(r_ptr); Sp.o_r_rec = addi(r_rec); Sp.o_r_pair = addi(r_pair); Sp.o_c_ptr = addi(c_ptr); Sp.o_c = addi(cc);
  Sp.od_G = addd(ht.G); Sp.od_B = addd(ht.B); Sp.od_Gd = addd(ht.Gd); Sp.od_Bd = addd(ht.Bd); Sp.od_vset = addd(ht.v_set);
  Sp.ipack_n = (int32_t)p.ipack.size(); Sp.dpack_n = (int32_t)p.dpack.size();
  Sp.R = p.R;
  const size_t shared_bytes = ((((size_t)Sp.dpack_n + 1) & ~(size_t)1) * 8 + (size_t)Sp.ipack_n * 4 + 15) & ~(size_t)15;
  Sp.wave_bytes = (int32_t)((((size_t)4 * (ht.lu_n_slots + ht.n) + (size_t)7 * ht.n) * sizeof(double) + 15) & ~(size_t)15);
  int waves = (int)((160 * 1024 - 512 - (long long)shared_bytes) / Sp.wave_bytes);
  if (const char* e = GS_EXPERIMENT_ENV("GS_SPARSE_LDS_WAVES")) waves = std::min(waves, atoi(e));
  waves = std::max(0, std::min(4, waves));
  if (waves < 1 || ht.n > 256)
    return reject(p, GS_E_TOPOLOGY, "sparse_lds: the schedule (%zu bytes) and one instance (%d bytes) do not fit the LDS, or more than 256 buses", shared_bytes, Sp.wave_bytes);
  Sp.waves = waves;
  p.sparse_lds = shared_bytes + (size_t)waves * Sp.wave_bytes;
  p.sparse_grid = std::max(1, std::min((p.B + waves - 1) / waves, cus));      // persistent: one workgroup per CU, instances strided over the wavefronts
  return "";
}
#endif

// ---- layout maps: observation / state columns -> slab rows, and the per-instance scalar rows ----
std::string plan_maps(const HostTopology& ht, GsPlan& p) {
  const GsRows& R = p.R;
  const int n = p.n, m = p.m;
  p.mvm.resize(n); p.mva.resize(n); p.mfl.resize(m); p.mld.resize(m); p.mp.resize(n); p.mq.resize(n); p.mact.resize(p.action_dim);
  std::vector<int32_t>& mo = p.mo; std::vector<int32_t>& mst = p.mst; std::vector<double>& cst = p.cst;
  for (int i = 0; i < n; ++i) { mo.push_back(R.VM + i); mo.push_back(R.VA + i); }          // grid_env.py:758-759
  for (int k = 0; k < m; ++k) { mo.push_back(R.FLOW + k); mo.push_back(R.ENVLOAD + k); }   // :762-763
  mo.push_back(R.FREQ);                                                                     // :766
  for (int l = 0; l < p.n_loads; ++l) {                                                     // :769-770 (static values)
    cst.push_back(ht.load_base[l]); mo.push_back(-(int)cst.size());
    cst.push_back(ht.load_q[l]); mo.push_back(-(int)cst.size());
  }
  for (int g = 0; g < p.n_gens; ++g) mo.push_back(R.GENP + g);                               // :773-777
  for (int q = 0; q < p.n_bats; ++q) { mo.push_back(R.SOC + q); mo.push_back(R.BATP + q); }  // :780-781
  for (int i = 0; i < n; ++i) { p.mvm[i] = R.VM + i; p.mva[i] = R.VA + i; p.mp[i] = R.P + i; p.mq[i] = R.Q + i; }
  for (int k = 0; k < m; ++k) { p.mfl[k] = R.FLOW + k; p.mld[k] = R.LOAD + k; }
  for (int a = 0; a < p.action_dim; ++a) p.mact[a] = R.ACT + a;
  for (int s : {R.TIME, R.STEP, R.VIOL, R.TOTLOSS, R.EPREW, R.FREQ, R.IRR, R.WIND, R.TEMP, R.CLOUD, R.SEEDLO, R.SEEDHI}) mst.push_back(s);
  for (int q = 0; q < p.n_bats; ++q) mst.push_back(R.SOC + q);
  for (int q = 0; q < p.n_bats; ++q) mst.push_back(R.BATP + q);
  for (int g = 0; g < p.n_gens; ++g) mst.push_back(R.CURT + g);
  for (int i = 0; i < n; ++i) mst.push_back(R.VM + i);
  for (int i = 0; i < n; ++i) mst.push_back(R.VA + i);
  for (int k = 0; k < m; ++k) mst.push_back(R.FLOW + k);
  for (int k = 0; k < m; ++k) mst.push_back(R.ENVLOAD + k);
  {   // the constants of an observation form one block (the static load powers); the step kernel skips it
    int c0 = 0;
    while (c0 < (int)mo.size() && mo[c0] >= 0) ++c0;
    int c1 = c0;
    while (c1 < (int)mo.size() && mo[c1] < 0) ++c1;
    bool one_block = true;
    for (int c = c1; c < (int)mo.size(); ++c) one_block = one_block && mo[c] >= 0;
    // (per-instance load powers: no column is the same for every instance -- the step writes them all, the copies move them all)
    if (one_block && !GS_EXPERIMENT_ENV("GS_PACK_ALL_COLUMNS") && !p.pl) { p.obs_skip0 = c0; p.obs_skip1 = c1; }
  }
  if ((int)mo.size() != p.obs_dim || (int)mst.size() != p.state_dim) return reject(p, GS_E_INVALID, "internal: layout map size mismatch");
  p.rf.resize(SF_COUNT); p.ri.resize(SI_COUNT); p.ru.resize(SU_COUNT);
  p.rf[SF_REWARD] = R.REWARD; p.rf[SF_VMAX] = R.VMAX; p.rf[SF_VMIN] = R.VMIN; p.rf[SF_LOSSES] = R.LOSSES; p.rf[SF_EPREW] = R.EPREW; p.rf[SF_MAXMIS] = R.MAXMIS;
  p.ri[SI_VIOL] = R.VIOL; p.ri[SI_STEP] = R.STEP; p.ri[SI_ITERS] = R.ITERS; p.ri[SI_STATUS] = R.STATUS;
  p.ru[SU_TERM] = R.TERM; p.ru[SU_TRUNC] = R.TRUNC; p.ru[SU_CONV] = R.CONV;
  for (int v = 0; v < 4; ++v) p.ru[SU_VF0 + v] = R.VFLAGS + v;
  return "";
}

}  // namespace

// The first Newton step from the flat start as a constant linear map of the injections (GsF2Tables::mesh_w): for a network whose
// buses other than the slack are all PQ buses,  x = J0^-1 (S_spec - S_calc(flat)) = W [P_spec; 1]  with Q_spec = 0 -- W = the
// angle-equation columns of J0^-1 and the constant term, (2 (n - 1)) x n.  J0: the exact Jacobian (power_flow.py:243-287) at |V| = 1,
// angle 0 (the slack at its set point), inverted by Gauss-Jordan with partial pivoting.  Output in the operand order of
// v_mfma_f64_16x16x4: [tiles row tiles][steps k-steps][64 lanes], A[row = lane & 15][k = lane >> 4], zero-padded.
bool flat_newton_map(const HostTopology& ht, int tiles, int steps, std::vector<double>& wt) {
  const int n_ = ht.n, sl = ht.slack, na = n_ - 1, N2 = 2 * na, K = na + 1;
  if (na < 1 || N2 > 16 * tiles || K > 4 * steps) return false;
  std::vector<double> v0(n_, 1.0);
  if (ht.fixed_v[sl]) v0[sl] = ht.v_set[sl];
  auto act = [&](int i) { return i < sl ? i : i - 1; };
  std::vector<double> Pc(n_, 0.0), Qc(n_, 0.0), J((size_t)N2 * N2, 0.0), Ji;
  for (int i = 0; i < n_; ++i)
    for (int q = ht.row_ptr[i]; q < ht.row_ptr[i + 1]; ++q) {
      const int j = ht.col[q];
      const double g = i == j ? ht.Gd[i] : ht.G[q], bq = i == j ? ht.Bd[i] : ht.B[q];
      Pc[i] += v0[i] * v0[j] * g; Qc[i] -= v0[i] * v0[j] * bq;
    }
  for (int i = 0; i < n_; ++i) {
    if (i == sl) continue;
    const int a = act(i);
    const double vi = v0[i];
    J[(size_t)(2 * a) * N2 + 2 * a] = -Qc[i] - vi * vi * ht.Bd[i];
    J[(size_t)(2 * a) * N2 + 2 * a + 1] = Pc[i] / vi + vi * ht.Gd[i];
    J[(size_t)(2 * a + 1) * N2 + 2 * a] = Pc[i] - vi * vi * ht.Gd[i];
    J[(size_t)(2 * a + 1) * N2 + 2 * a + 1] = Qc[i] / vi - vi * ht.Bd[i];
    for (int q = ht.row_ptr[i]; q < ht.row_ptr[i + 1]; ++q) {
      const int j = ht.col[q];
      if (j == i || j == sl) continue;
      const int aj = act(j);
      const double aa = vi * v0[j], gs_bc = -ht.B[q] * aa, gc_bs = ht.G[q] * aa;
      J[(size_t)(2 * a) * N2 + 2 * aj] += gs_bc; J[(size_t)(2 * a) * N2 + 2 * aj + 1] += gc_bs / v0[j];
      J[(size_t)(2 * a + 1) * N2 + 2 * aj] += -gc_bs; J[(size_t)(2 * a + 1) * N2 + 2 * aj + 1] += gs_bc / v0[j];
    }
  }
  if (!gauss_jordan_inverse(J, N2, Ji)) return false;
  std::vector<double> cst(N2, 0.0);
  for (int u = 0; u < N2; ++u)
    for (int a2 = 0; a2 < na; ++a2) {
      const int bus = a2 < sl ? a2 : a2 + 1;
      cst[u] -= Ji[(size_t)u * N2 + 2 * a2] * Pc[bus] + Ji[(size_t)u * N2 + 2 * a2 + 1] * Qc[bus];
    }
  wt.assign((size_t)tiles * steps * 64, 0.0);
  for (int t = 0; t < tiles; ++t)
    for (int s2 = 0; s2 < steps; ++s2)
      for (int ln = 0; ln < 64; ++ln) {
        const int u = 16 * t + (ln & 15), k = 4 * s2 + (ln >> 4);
        if (u < N2 && k < K) wt[((size_t)t * steps + s2) * 64 + ln] = k < na ? Ji[(size_t)u * N2 + 2 * k] : cst[u];
      }
  return true;
}

// ---- per-instance line impedances: only the second-generation radial members take them (their topology tables stay valid; the
// instance's numbers come from gs_k_line_params).  The branch entry Y(s, parent) and the diagonal Y(s, s) of every slot that has
// one in the shared tables, as the line-order lists of topology.cpp's add() calls that reach it.
std::string plan_line_params(const gs_topology& topo, const gs_config& cfg, const HostTopology& ht, GsPlan& p) {
  if (!p.f2().pz) {
    std::string why = !p.flow2_why.empty() ? p.flow2_why : !p.mesh_why.empty() ? p.mesh_why
                    : p.step == StepMember::nr_mesh2 ? "a meshed network (nr_mesh2)"
                    : cfg.solver_kind == GS_SOLVER_FBS && cfg.fbs_warm_start ? "warm start"
                    : cfg.solver_kind == GS_SOLVER_NR && cfg.jacobian_mode != GS_JACOBIAN_EXACT ? "as-coded Jacobian"
                    : !ht.is_forest ? "a meshed network" : std::string("the step runs on ") + kSolveName[(int)p.solve];
    return "per-instance line impedances need a second-generation radial step member: " + why;
  }
  const bool newton = p.f2().newton();
  const int nsl = ht.n + 3, m = ht.m;
  p.pz_zero.assign((size_t)m, 0);
  for (int k = 0; k < m; ++k) p.pz_zero[k] = std::hypot(topo.r[k], topo.x[k]) > 1e-12 ? 0 : 1;
  p.pz_has.assign((size_t)nsl, 0);
  for (int i = 0; i < ht.n; ++i)
    if (i != ht.slack && ht.lvl_pos[i] >= 0 && ht.fbs_parent[i] >= 0) p.pz_has[i] = 1;
  // the ops of one Ybus entry (a, c): add(i, j, -y), add(j, i, -y), add(i, i, y), add(j, j, y) of every line in order (topology.cpp)
  auto ops_of = [&](int a, int c) {
    for (int k = 0; k < m; ++k) {
      if (ht.lyr[k] == 0.0 && ht.lyi[k] == 0.0) continue;
      const int i = ht.lfrom[k], j = ht.lto[k];
      if (i == a && j == c) p.pz_ops.push_back(2 * k + 1);
      if (j == a && i == c) p.pz_ops.push_back(2 * k + 1);
      if (a == c && i == a) p.pz_ops.push_back(2 * k);
      if (a == c && j == a) p.pz_ops.push_back(2 * k);
    }
  };
  p.pz_ops_ptr.assign((size_t)2 * nsl + 1, 0);
  p.pz_ops.clear();
  for (int list = 0; list < 2 * nsl; ++list) {
    p.pz_ops_ptr[list] = (int32_t)p.pz_ops.size();
    const int s = list % nsl;
    if (s < ht.n && p.pz_has[s]) { if (list < nsl) ops_of(s, ht.fbs_parent[s]); else if (newton) ops_of(s, s); }
  }
  p.pz_ops_ptr[2 * nsl] = (int32_t)p.pz_ops.size();
  return "";
}

std::string gs_check_line_impedances(const gs_topology& topo, int batch, const double* r_inst, const double* x_inst, const uint8_t* mask) {
  if (!r_inst || !x_inst) return "line impedances: r and x go together";
  char msg[256];
  for (int b = 0; b < batch; ++b) {
    if (mask && !mask[b]) continue;
    for (int k = 0; k < topo.m; ++k) {
      const double r = r_inst[(size_t)b * topo.m + k], x = x_inst[(size_t)b * topo.m + k];
      if (!std::isfinite(r) || !std::isfinite(x)) snprintf(msg, sizeof msg, "line impedances: instance %d line %d is not finite", b, k);
      else if (!(r >= 0.0)) snprintf(msg, sizeof msg, "line impedances: instance %d line %d has r < 0", b, k);
      else if (!(std::hypot(topo.r[k], topo.x[k]) > 1e-12)) {
        if (r == topo.r[k] && x == topo.x[k]) continue;
        snprintf(msg, sizeof msg, "line impedances: instance %d line %d: a line of zero nominal impedance keeps its nominal r, x", b, k);
      } else if (!(std::hypot(r, x) > 1e-12)) snprintf(msg, sizeof msg, "line impedances: instance %d line %d has zero impedance", b, k);
      else continue;
      return msg;
    }
  }
  return "";
}

// ---- per-instance load powers: every second-generation step member takes them (nothing of its tables depends on the loads; the
// flat start of the Newton-Raphson members does not either, so their flat-start table / W product stays)
std::string plan_load_params(const gs_topology& topo, const gs_config& cfg, const HostTopology& ht, GsPlan& p) {
  if (!p.second_gen()) {
    std::string why = !p.flow2_why.empty() ? p.flow2_why : !p.mesh_why.empty() ? p.mesh_why
                    : cfg.solver_kind == GS_SOLVER_FBS && cfg.fbs_warm_start ? "warm start"
                    : cfg.solver_kind == GS_SOLVER_NR && cfg.jacobian_mode != GS_JACOBIAN_EXACT ? "as-coded Jacobian"
                    : std::string("the step runs on ") + kSolveName[(int)p.solve];
    return "per-instance load powers need a second-generation step member: " + why;
  }
  p.pl_tan.resize((size_t)topo.n_loads);
  for (int l = 0; l < topo.n_loads; ++l) p.pl_tan[l] = std::tan(std::acos(topo.load_pf[l]));      // topology.cpp: load_q = base * this
  return "";
}

std::string gs_check_load_powers(int n_loads, int batch, const double* base_inst, const uint8_t* mask) {
  if (n_loads <= 0) return "load powers: the feeder has no loads";
  if (!base_inst) return "load powers: base is NULL";
  char msg[256];
  for (int b = 0; b < batch; ++b) {
    if (mask && !mask[b]) continue;
    for (int l = 0; l < n_loads; ++l) {
      const double v = base_inst[(size_t)b * n_loads + l];
      if (!std::isfinite(v)) snprintf(msg, sizeof msg, "load powers: instance %d load %d is not finite", b, l);
      else if (!(v >= 0.0)) snprintf(msg, sizeof msg, "load powers: instance %d load %d is negative", b, l);
      else continue;
      return msg;
    }
  }
  return "";
}

std::string gs_plan(const gs_topology& topo, const gs_config& cfg, const HostTopology& ht, int batch, int cus, GsPlan& p) {
  p.B = batch; p.Bp = (batch + 63) / 64 * 64; p.groups = p.Bp / 64;
  int W = cfg.waves_per_group;
  if (const char* e = getenv("GS_WAVES")) W = atoi(e);
  const bool auto_w = W <= 0;
  if (W <= 0) { W = 1; while (W < 16 && p.groups * W * 2 <= 2048) W *= 2; }
  p.W = std::min(W, GS_MAX_WAVES);
  std::string why = plan_solve(cfg, ht, auto_w, p);
  if (!why.empty()) return why;
  // the epilogue's cross-wave partials need 48 KB; the observation pack stages two or three 64-column tiles behind them
  p.dyn_lds = std::max<size_t>(49152 + 2 * 64 * 65 * sizeof(double), p.dyn_lds);
  p.n = ht.n; p.m = ht.m; p.n_loads = topo.n_loads; p.n_gens = topo.n_gens; p.n_bats = topo.n_bats;
  p.obs_dim = 2 * p.n + 2 * p.m + 1 + 2 * p.n_loads + p.n_gens + 2 * p.n_bats;     // grid_env.py:307-314
  p.action_dim = p.n_bats + p.n_gens;                                               // grid_env.py:351
  p.state_dim = 12 + 2 * p.n_bats + p.n_gens + 2 * p.n + 2 * p.m;
  plan_rows(ht, p);
  plan_work_lists(ht, p);
  plan_second_gen(topo, cfg, ht, auto_w, p);
  p.pz = topo.line_r_inst != nullptr;
  p.nr_flat = p.f2().newton() && !getenv("GS_NR_NO_FLAT") && !p.pz;
  if (p.pz && (why = plan_line_params(topo, cfg, ht, p)).empty() == false) { p.err_code = GS_E_TOPOLOGY; return why; }
  p.pl = topo.load_base_inst != nullptr;
  if (p.pl && (why = plan_load_params(topo, cfg, ht, p)).empty() == false) { p.err_code = GS_E_TOPOLOGY; return why; }
  if (ht.has_lu) plan_lu_schedule(ht, p);
  if (p.solve == SolveMember::nr_dense_mfma && !(why = plan_dense(cfg, ht, cus, p)).empty()) return why;
#if defined(GS_BUILD_EXPERIMENTS)
  if (p.solve == SolveMember::nr_sparse_lds && !(why = plan_sparse_lds(cfg, ht, cus, p)).empty()) return why;
#endif
  // a step as two half-grid launches on two streams: only where each half still gives every CU a workgroup
  p.lean = p.second_gen() && !getenv("GS_EAGER_ROWS");
  p.split_ok = p.second_gen() && 2 * (size_t)p.F2.lds_bytes <= 160 * 1024 && !getenv("GS_NO_SPLIT") && p.groups * (64 / p.f2().iw) >= 512 &&
               p.groups >= 2;
  p.SC.tolerance = cfg.tolerance; p.SC.alpha = cfg.acceleration_factor;
  p.SC.max_iterations = cfg.max_iterations; p.SC.jacobian_exact = (cfg.jacobian_mode == GS_JACOBIAN_EXACT);
  GsEnvCfg& E = p.EC;
  E.timestep = cfg.timestep; E.v_min = cfg.v_min; E.v_max = cfg.v_max; E.f_min = cfg.f_min; E.f_max = cfg.f_max;
  E.safety_penalty = cfg.safety_penalty; E.H = cfg.inertia_H; E.D = cfg.damping_D; E.f0 = cfg.f_nominal;
  E.power_base = cfg.power_base; E.inv_power_base = 1.0 / cfg.power_base; E.episode_length = cfg.episode_length; E.stochastic_loads = cfg.stochastic_loads;
  E.fbs_warm_start = cfg.fbs_warm_start; E.weather_variation = cfg.weather_variation;
  // sum(load.active_power) in list order, starting from 0 like python's sum() (grid_env.py:744)
  p.total_load = 0.0;
  for (int l = 0; l < p.n_loads; ++l) p.total_load += topo.load_base[l];
  return plan_maps(ht, p);
}

void gs_plan_format(const GsPlan& p, const HostTopology& ht, char* buf, int buflen) {
  const bool f2 = p.second_gen(), dense = p.solve == SolveMember::nr_dense_mfma;
  snprintf(buf, buflen,
           "{\"kernel\": \"%s\", \"n\": %d, \"m\": %d, \"nnz\": %d, \"forest\": %s, \"levels\": %d, \"max_level_width\": %d, "
           "\"lu_slots\": %d, \"lu_orig\": %d, \"lu_pairs\": %lld, \"waves_per_group\": %d, \"groups\": %d, "
           "\"rows_per_group\": %d, \"slab_bytes\": %zu, \"obs_dim\": %d, \"action_dim\": %d, "
           "\"instances_per_workgroup\": %d, \"workgroups\": %d, \"step_lds_bytes\": %zu, \"step_launches\": %d, \"solve_kernel\": \"%s\", \"flow2\": \"%s\", "
           "\"mesh2\": \"%s\", \"mesh_levels\": %d, \"mesh_rows\": %d, \"mesh_message_units\": %d, \"mesh_messages\": %d, \"mesh_accumulators\": %d, "
           "\"dense_form\": \"%s\", \"dense_workgroups\": %d, \"dense_lds_bytes\": %zu, \"per_instance_z\": %d, \"nr_flat_start_table\": %d, "
           "\"per_instance_loads\": %d}",
           f2 ? p.f2().name : kSolveName[(int)p.solve], p.n, p.m, ht.nnz, ht.is_forest ? "true" : "false", ht.n_levels,
           ht.max_level_width, ht.lu_n_slots, ht.lu_n_orig, (long long)ht.lu_n_pairs, f2 ? p.f2().nw : p.W, p.groups,
           p.R.total, (size_t)p.groups * p.R.total * GS_LANES * sizeof(double), p.obs_dim, p.action_dim,
           f2 ? p.f2().iw : 64, f2 ? (64 / p.f2().iw) * p.groups : p.groups, f2 ? (size_t)p.F2.lds_bytes : p.dyn_lds + 24576, p.split_ok ? 2 : 1,
           kSolveName[(int)p.solve], f2 ? "on" : (p.flow2_why.empty() ? "n/a" : p.flow2_why.c_str()),
           p.step == StepMember::nr_mesh2 ? "on" : (p.mesh_why.empty() ? "n/a" : p.mesh_why.c_str()), p.mesh_levels, p.mesh_rows, p.mesh_units,
           p.mesh_messages, p.mesh_accs, dense ? (p.dense_blockrow ? "block_row" : "panel") : "n/a", dense ? p.dense_grid : 0, dense ? p.dense_lds : (size_t)0,
           p.pz ? 1 : 0, p.nr_flat ? 1 : 0, p.pl ? 1 : 0);
}
