// kernels_costs.hip -- the constraint signals of observation rows (include/gridstep.h, "constraint costs"):
// gs_k_costs, one kernel for the rows of a rollout, its terminal list and a plain matrix (GsCostArgs, gs_internal.h).
//
// A bandwidth kernel: per row it reads the contiguous prefix of 2 n + 2 m + 1 doubles and writes nine numbers.  A row is owned by a
// group of L = 8 .. 64 lanes of one wavefront (the host picks L from the prefix length, gs_cost_lanes: a 51-column prefix on 64 lanes
// would idle three quarters of them), lane = column, so every load instruction of a group is one run of L consecutive doubles --
// 8-byte loads, since a row with an odd obs_dim is only 8-byte aligned.  A lane issues the GS_COST_LOADS loads of a pass for
// GS_COST_ROWS rows before it looks at any of them (4 KiB a wavefront); the workgroup is one wavefront and a compute unit holds
// twenty at this register count, so tens of KiB are in flight.  (Eight loads a pass for the 64-lane form took 170 registers, two
// wavefronts a SIMD: more in flight per wavefront, less per compute unit.)
// Which family a column belongs to depends on the column alone: even columns below 2 n are |V|, odd columns from 2 n on are the
// loadings, and L is even, so a lane sees voltages or loadings, never both.  The extremes and counts are reduced across the group
// with DPP (quad permutes, the two row mirrors) and the gfx950 lane swaps above 16 lanes: no LDS.  v_min_f64 / v_max_f64 drop a NaN
// operand, so `x != x` of a channel's own inputs rides along as a flag and overwrites that channel's margin at the end.
// Every result is a minimum, a maximum, a count or one rounded subtraction of those (x -> x - lo and x -> hi - x are monotonic under
// rounding, so the minimum of the differences is the difference at the extreme): the bits do not depend on L or on the launch.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/gridstep.h"
#include "gs_internal.h"
#include "kernels.h"

namespace {

template <int CTRL> __device__ __forceinline__ int gc_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }
template <int CTRL> __device__ __forceinline__ double gc_dpp(double v) {
  const uint2 u = __builtin_bit_cast(uint2, v);
  return __builtin_bit_cast(double, make_uint2((unsigned)gc_dpp<CTRL>((int)u.x), (unsigned)gc_dpp<CTRL>((int)u.y)));
}
// (x of the even 16-lane row of this lane's row pair, x of the odd one) and (x of lane i mod 32, x of lane 32 + i mod 32): the
// forms of kernels_flow2.hip (f2_rows16, f2_halves32)
struct GcTwoI { int a, b; };
struct GcTwoD { double a, b; };
__device__ __forceinline__ GcTwoI gc_rows16(int x) { const auto r = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false); return GcTwoI{(int)r[0], (int)r[1]}; }
__device__ __forceinline__ GcTwoI gc_halves32(int x) { const auto r = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false); return GcTwoI{(int)r[0], (int)r[1]}; }
__device__ __forceinline__ GcTwoD gc_rows16(double x) {
  const uint2 u = __builtin_bit_cast(uint2, x);
  const auto lo = __builtin_amdgcn_permlane16_swap(u.x, u.x, false, false), hi = __builtin_amdgcn_permlane16_swap(u.y, u.y, false, false);
  return GcTwoD{__builtin_bit_cast(double, make_uint2(lo[0], hi[0])), __builtin_bit_cast(double, make_uint2(lo[1], hi[1]))};
}
__device__ __forceinline__ GcTwoD gc_halves32(double x) {
  const uint2 u = __builtin_bit_cast(uint2, x);
  const auto lo = __builtin_amdgcn_permlane32_swap(u.x, u.x, false, false), hi = __builtin_amdgcn_permlane32_swap(u.y, u.y, false, false);
  return GcTwoD{__builtin_bit_cast(double, make_uint2(lo[0], hi[0])), __builtin_bit_cast(double, make_uint2(lo[1], hi[1]))};
}

struct GcMin { __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); } };
struct GcMax { __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); } };
struct GcAdd { __device__ __forceinline__ int operator()(int a, int b) const { return a + b; } };

// op over the L lanes of this lane's group, the result in every one of them: neighbours (quad_perm [1,0,3,2]), pairs ([2,3,0,1]),
// the other quad of the eight (row_half_mirror), the other eight of the sixteen (row_mirror), then the swaps
template <int L, class X, class Op> __device__ __forceinline__ X gc_all(X v, Op op) {
  v = op(v, gc_dpp<0xB1>(v));
  v = op(v, gc_dpp<0x4E>(v));
  v = op(v, gc_dpp<0x141>(v));
  if constexpr (L >= 16) v = op(v, gc_dpp<0x140>(v));
  if constexpr (L >= 32) { const auto t = gc_rows16(v); v = op(t.a, t.b); }
  if constexpr (L >= 64) { const auto t = gc_halves32(v); v = op(t.a, t.b); }
  return v;
}

__device__ __forceinline__ double gc_cost(int kind, double margin, int count) {
  if (kind == GS_COSTKIND_COUNT) return (double)count;
  if (kind == GS_COSTKIND_INDICATOR) return margin < 0.0 ? 1.0 : 0.0;
  return margin < 0.0 ? -margin : 0.0;
}

template <int L> __device__ __forceinline__ void gc_rows(const GsCostArgs& A) {
#pragma clang fp contract(off)
  constexpr int CH = GS_COST_LOADS;
  constexpr int R = GS_COST_ROWS, RW = R * (64 / L);         // rows of a group, of the wavefront, per pass over the grid
  const int lane = threadIdx.x & 63, g = lane / L, l = lane % L;
  const long long rows = A.rows_dev ? (long long)min(*A.rows_dev, A.rows) : (long long)A.rows;
  const int n2 = 2 * A.n, W = n2 + 2 * A.m;                  // the frequency's column
  const size_t D = (size_t)A.D;
  const double inf = __builtin_huge_val();
  int viol[GS_COST_CHANNELS] = {0, 0, 0};
  for (long long r0 = (long long)blockIdx.x * RW; r0 < rows; r0 += (long long)gridDim.x * RW) {
    const double* row[R];
    double f[R], vmin[R], vmax[R], lmax[R];
    int cv[R], ct[R], nan[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      row[r] = A.obs + (size_t)min(r0 + g * R + r, rows - 1) * D;      // (a row past the end: the last one again, never written)
      vmin[r] = inf; vmax[r] = -inf; lmax[r] = 0.0; cv[r] = 0; ct[r] = 0; nan[r] = 0;
      f[r] = row[r][W];                    // (the same address in every lane of the group: one request)
    }
    for (int c0 = 0; c0 < W; c0 += CH * L) {
      double x[R][CH];
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int c = min(c0 + j * L + l, W - 1);
#pragma unroll
        for (int r = 0; r < R; ++r) x[r][j] = row[r][c];
      }
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int c = c0 + j * L + l;
        const bool is_v = c < n2 && !(c & 1), is_l = c >= n2 && c < W && (c & 1);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double v = x[r][j], a = fabs(v);
          vmin[r] = fmin(vmin[r], is_v ? v : inf);
          vmax[r] = fmax(vmax[r], is_v ? v : -inf);
          lmax[r] = fmax(lmax[r], is_l ? a : 0.0);
          cv[r] += (is_v && (v < A.vlo || v > A.vhi)) ? 1 : 0;
          ct[r] += (is_l && a > A.lim) ? 1 : 0;
          nan[r] |= (v != v) ? (is_v ? 1 : (is_l ? 256 : 0)) : 0;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      vmin[r] = gc_all<L>(vmin[r], GcMin{}); vmax[r] = gc_all<L>(vmax[r], GcMax{}); lmax[r] = gc_all<L>(lmax[r], GcMax{});
      cv[r] = gc_all<L>(cv[r], GcAdd{}); ct[r] = gc_all<L>(ct[r], GcAdd{}); nan[r] = gc_all<L>(nan[r], GcAdd{});
    }
    // lane r of the group files row r
    double fr = f[0], vmn = vmin[0], vmx = vmax[0], lmx = lmax[0];
    int cvr = cv[0], ctr = ct[0], nanr = nan[0];
#pragma unroll
    for (int r = 1; r < R; ++r)
      if (l == r) { fr = f[r]; vmn = vmin[r]; vmx = vmax[r]; lmx = lmax[r]; cvr = cv[r]; ctr = ct[r]; nanr = nan[r]; }
    const long long k = r0 + g * R + l;
    if (l < R && k < rows && !(A.skip && A.skip[k])) {
      long long entry = k;
      bool ok = true;
      if (A.scatter_idx) {
        const int t = A.scatter_idx[2 * k], b = A.scatter_idx[2 * k + 1];
        ok = (unsigned)t < (unsigned)A.scatter_T && (unsigned)b < (unsigned)A.scatter_B;
        entry = (long long)t * A.scatter_B + b;
      }
      if (ok) {
        const double qnan = __builtin_nan("");
        double mg[GS_COST_CHANNELS];
        mg[GS_COST_VOLTAGE] = (nanr & 0xff) ? qnan : fmin(vmn - A.vlo, A.vhi - vmx);
        mg[GS_COST_FREQUENCY] = fr != fr ? qnan : fmin(fr - A.flo, A.fhi - fr);
        mg[GS_COST_THERMAL] = (nanr >> 8) ? qnan : A.lim - lmx;
        const int cn[GS_COST_CHANNELS] = {cvr, (fr < A.flo || fr > A.fhi) ? 1 : 0, ctr};
#pragma unroll
        for (int c = 0; c < GS_COST_CHANNELS; ++c) {
          const long long at = c * A.chan_stride + entry * A.row_stride;
          if (A.margins) A.margins[at] = mg[c];
          if (A.counts) A.counts[at] = cn[c];
          if (A.costs) A.costs[at] = gc_cost(A.kind[c], mg[c], cn[c]);
          viol[c] += mg[c] < 0.0 ? 1 : 0;
        }
      }
    }
  }
  // the workgroup is this wavefront: its sum, then one integer atomic per channel
  if (A.n_violating) {
#pragma unroll
    for (int c = 0; c < GS_COST_CHANNELS; ++c) {
      const int s = gc_all<64>(viol[c], GcAdd{});
      if (lane == 0 && s) atomicAdd(A.n_violating + c, (unsigned long long)s);
    }
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64)
gs_k_costs(GsCostArgs A) {
  if (A.lanes == 8) gc_rows<8>(A);
  else if (A.lanes == 16) gc_rows<16>(A);
  else if (A.lanes == 32) gc_rows<32>(A);
  else gc_rows<64>(A);
}
