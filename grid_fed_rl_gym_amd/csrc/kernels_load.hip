// kernels_load.hip -- a recorded dataset becomes the handle's rollout (include/gridstep.h "a recorded dataset as the handle's
// rollout"): gs_k_load_widen, the one exact widening of a float32 source, and gs_k_load_next_f64 / _f32, which
// file a staged chunk of next_observations (GsLoadNextArgs, rollout_load.h).
//
// Bandwidth kernels.  gs_k_load_next: a row is owned by a group of L = 8 .. 64 lanes of one wavefront (gs_load_lanes: a 71-column
// row on 64 lanes would idle half of them in its second pass), lane = column, so every load and store of a group is one run of L
// consecutive elements -- 8-byte accesses in float64, since a row with an odd obs_dim is only 8-byte aligned.  What happens to a row
// depends on the row alone (its map entry, its t), so a group never diverges inside a row.  A finished row is stored at its place in
// the terminal list; a live row is compared with the slot the load wrote before, word by word as integers: a NaN equals the same
// NaN.  The group's verdict is an OR across its lanes (DPP-free: L is a run-time value here, the shuffles are five at most and the
// kernel waits for memory); one lane then counts the row and lowers the first offending index.  Integer atomics only.
#include <hip/hip_runtime.h>

#include "gs_internal.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ double gl_widen(double x) { return x; }
__device__ __forceinline__ double gl_widen(float x) { return (double)x; }

template <class SRC> __device__ __forceinline__ void gl_next(const GsLoadNextArgs& G) {
  const int L = G.lanes, lane = threadIdx.x & 63, g = lane / L, l = lane % L, per_wave = 64 / L;
  const int wave = (int)(threadIdx.x >> 6), waves = (int)(blockDim.x >> 6);
  const size_t D = (size_t)G.D;
  const SRC* const src = (const SRC*)G.src;
  const long long last0 = G.n - G.B;      // the first transition of step T - 1
  for (long long i0 = ((long long)blockIdx.x * waves + wave) * per_wave; i0 < G.rows; i0 += (long long)gridDim.x * waves * per_wave) {
    const long long i = i0 + g;
    const bool there = i < G.rows;
    const long long j = G.row0 + (there ? i : 0);
    const int k = there ? G.map[i] : -1;
    const SRC* const row = src + (size_t)(there ? i : 0) * D;
    double* const slot = G.obs_seq + ((size_t)j + (size_t)G.B) * D;       // obs_seq[t + 1][b]
    const bool is_slot = j >= last0 && !G.have_final;                      // the row IS slot T
    const bool done = k >= 0 && k < G.term_cap;
    double* const term = done ? G.term_obs + (size_t)k * D : nullptr;
    const bool compare = there && k < 0 && !is_slot;
    int bad = 0;
    if (there) {
#pragma unroll 4
      for (int c = l; c < G.D; c += L) {
        const double x = gl_widen(row[c]);
        if (term) term[c] = x;
        if (is_slot) slot[c] = x;
        if (compare) bad |= __builtin_bit_cast(unsigned long long, x) != __builtin_bit_cast(unsigned long long, slot[c]) ? 1 : 0;
      }
    }
    // (every lane of the wavefront is here: rows past the end carry bad = 0)
    for (int w = 1; w < L; w *= 2) bad |= __shfl_xor(bad, w, 64);
    if (bad && l == 0) {
      atomicAdd(G.verdict, 1);
      atomicMin(G.verdict + 1, (int)j);
    }
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256)
gs_k_load_widen(const float* __restrict__ src, double* __restrict__ dst, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] = (double)src[i];
}

extern "C" __global__ void __launch_bounds__(64 * GS_LOAD_WAVES) gs_k_load_next_f64(GsLoadNextArgs G) { gl_next<double>(G); }
extern "C" __global__ void __launch_bounds__(64 * GS_LOAD_WAVES) gs_k_load_next_f32(GsLoadNextArgs G) { gl_next<float>(G); }
