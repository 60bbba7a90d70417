// kernels_window.hip -- the device side of gs_rollout_continue (include/gridstep.h "a sliding window over consecutive rollouts";
// DESIGN.md section 30; argument blocks: rollout_window.h):
//   gs_k_window_shift       the kept steps of up to five arrays to the front (or into larger buffers), a streaming copy
//   gs_k_window_terms       the terminal list's kept entries, compacted in their order and renumbered (one workgroup)
//   gs_k_window_term_rows   their terminal observation rows, into another buffer
#include <hip/hip_runtime.h>

#include "rollout_window.h"

template <typename X>
static __device__ __forceinline__ void win_copy(const char* __restrict__ src, char* __restrict__ dst, long long bytes) {
  const X* __restrict__ s = (const X*)src;
  X* __restrict__ d = (X*)dst;
  const long long n = bytes / (long long)sizeof(X), stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) d[i] = s[i];
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_window_shift(GsWindowShiftArgs G) {
  GsWindowSeg s = G.seg[0];                  // (selected, not indexed: the argument block stays in scalar registers)
#pragma unroll
  for (int a = 1; a < GS_WIN_ARRAYS; ++a)
    if ((int)blockIdx.y == a) s = G.seg[a];
  if (s.bytes <= 0) return;
  const unsigned long long fit = (unsigned long long)(uintptr_t)s.src | (unsigned long long)(uintptr_t)s.dst | (unsigned long long)s.bytes;
  if ((fit & 15ull) == 0) win_copy<uint4>(s.src, s.dst, s.bytes);
  else if ((fit & 7ull) == 0) win_copy<unsigned long long>(s.src, s.dst, s.bytes);
  else win_copy<unsigned char>(s.src, s.dst, s.bytes);
}

extern "C" __global__ void __launch_bounds__(GS_WIN_TERM_THREADS)
gs_k_window_terms(GsWindowTermsArgs G) {
  constexpr int WAVES = GS_WIN_TERM_THREADS / 64;
  __shared__ int wsum[WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int count = G.count[0];
  const int n = min(max(count, 0), G.cap_in);
  int running = 0;                           // (the same in every thread)
  for (int base = 0; base < n; base += GS_WIN_TERM_THREADS) {
    const int k = base + tid;
    int t = -1, b = 0;
    if (k < n) { t = G.idx_in[2 * k]; b = G.idx_in[2 * k + 1]; }
    const bool kept = k < n && t >= G.drop;
    const unsigned long long ballot = __ballot(kept);
    const int before = __popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(ballot);
    __syncthreads();
    int off = running, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      if (w < wave) off += wsum[w];
      total += wsum[w];
    }
    if (k < n) {
      int p = -1;
      if (kept) {
        p = off + before;
        G.idx_out[2 * p] = t - G.drop; G.idx_out[2 * p + 1] = b;
      }
      G.pos[k] = p;
    }
    running += total;
    __syncthreads();                         // (wsum is rewritten by the next chunk)
  }
  __syncthreads();                           // (every thread has read the old count)
  if (tid == 0) { G.n_old[0] = n; G.count[0] = running + (count - n); }
}

extern "C" __global__ void __launch_bounds__(256)
gs_k_window_term_rows(GsWindowTermRowsArgs G) {
  const long long total = (long long)G.n_old[0] * G.D, stride = (long long)gridDim.x * blockDim.x;
  for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += stride) {
    const long long k = x / G.D;
    const int p = G.pos[k];
    if (p >= 0) G.obs_out[(long long)p * G.D + (x - k * G.D)] = G.obs_in[x];
  }
}
