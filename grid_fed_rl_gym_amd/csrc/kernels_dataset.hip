// kernels_dataset.hip -- the device-resident GridDataset (include/gridstep.h "gs_dataset_*"): per-column
// statistics of the last rollout, the transition -> terminal-row map, and the minibatch gather.  Nothing here reads or writes the
// slab: the kernels see the rollout's buffers (read only) and the dataset's own.
//
// Statistics: three row-major matrices over the same N = T * B rows (obs_seq[0 .. T-1] [N][obs_dim], actions [N][A], rewards [N][1])
// go through one pair of kernels; their columns are filed side by side, Ct = obs_dim + A + 1 in all.
//   gs_k_ds_chunk_stats  one wave per (64-lane column panel, chunk of GS_DS_ROWS_PER_CHUNK rows).  A lane owns one column pair
//                        (16-byte loads; one column with 8-byte loads where the matrix has an odd width) and keeps the SHIFTED sums
//                        S1 = sum (x - k), S2 = sum (x - k)^2, k = the chunk's first row of the column: a subtraction, an addition and
//                        a fused multiply-add per element, no division in the loop.  It files (offset, M2) with
//                        offset = (k - K) + S1 / n, K = row 0 of the whole matrix, and M2 = S2 - S1^2 / n floored at 0; the chunk's
//                        mean is K + offset.  Keeping the tree's means relative to K leaves ONE rounding at the magnitude of the data
//                        (the last addition of K, gs_k_ds_merge), every other one scales with the column's spread.
//   gs_k_ds_merge        Chan's pairwise update over the chunks in a FIXED binary tree: one launch folds aligned groups of 16 nodes
//                        (four levels of the tree, in registers), in place; a node's row count follows from its position, so it is
//                        not stored.  The launch that leaves one node writes mean = K + offset and std = sqrt(M2 / N).
// No atomics, no dependence on which workgroup runs when: the same rollout gives the same bits.  A column whose values are all equal
// has x - k = 0 in every chunk and k - K = 0, so its offset and M2 are exact zeros through every merge: mean = the value, std = 0.
#include <hip/hip_runtime.h>
#include <math.h>

#include "gs_internal.h"
#include "env_device.h"
#include "kernels.h"

namespace {

// one column pair (W = 2, 16-byte loads) or one column (W = 1) of one chunk
template <int W>
__device__ __forceinline__ void ds_chunk_column(const double* __restrict__ x, int C, int c, long long row0, int n, double* __restrict__ part_row) {
  typedef double V __attribute__((ext_vector_type(W)));
  const double* p = x + (size_t)row0 * C + c;
  const V K = *(const V*)(x + c);
  const V k = *(const V*)p;
  V s1 = 0.0, s2 = 0.0;
  int r = 0;
  for (; r + 8 <= n; r += 8) {            // eight rows in flight per lane
    V v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = *(const V*)(p + (size_t)j * C);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const V d = v[j] - k;
      s1 += d;
      for (int w = 0; w < W; ++w) s2[w] = fma(d[w], d[w], s2[w]);
    }
    p += (size_t)8 * C;
  }
  for (; r < n; ++r, p += C) {
    const V d = *(const V*)p - k;
    s1 += d;
    for (int w = 0; w < W; ++w) s2[w] = fma(d[w], d[w], s2[w]);
  }
  const double dn = (double)n;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const double q = s1[w] / dn;
    part_row[2 * (c + w)] = (k[w] - K[w]) + q;
    part_row[2 * (c + w) + 1] = fmax(fma(-s1[w], q, s2[w]), 0.0);
  }
}

struct DsNode { double off, m2; long long n; };

// Chan et al.: b joins a (a covers the rows in front of b's); a node without rows leaves the other as it is
__device__ __forceinline__ DsNode ds_join(const DsNode& a, const DsNode& b) {
  if (b.n == 0) return a;
  if (a.n == 0) return b;
  DsNode o;
  o.n = a.n + b.n;
  const double na = (double)a.n, nb = (double)b.n, nn = (double)o.n;
  const double delta = b.off - a.off;
  o.off = a.off + delta * (nb / nn);
  o.m2 = (a.m2 + b.m2) + (delta * delta) * (na * nb / nn);
  return o;
}

}  // namespace

extern "C" {

// grid: (sum of the matrices' panels) * ceil(chunks / 4) workgroups of 4 waves; wave w of a workgroup takes chunk 4 * group + w
__global__ void __launch_bounds__(256)
gs_k_ds_chunk_stats(GsDsStatArgs A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int panels = A.m[0].panels + A.m[1].panels + A.m[2].panels;
  int panel = (int)(blockIdx.x % (unsigned)panels);
  const long long chunk = (long long)(blockIdx.x / (unsigned)panels) * 4 + wave;
  if (chunk >= A.chunks) return;
  int mi = 0;
  if (panel >= A.m[0].panels) { panel -= A.m[0].panels; mi = 1; }
  if (mi == 1 && panel >= A.m[1].panels) { panel -= A.m[1].panels; mi = 2; }
  const GsDsMatrix M = A.m[mi];
  const long long row0 = chunk * GS_DS_ROWS_PER_CHUNK;
  const int n = (int)(A.N - row0 < GS_DS_ROWS_PER_CHUNK ? A.N - row0 : GS_DS_ROWS_PER_CHUNK);
  double* part_row = A.part + ((size_t)chunk * A.Ct + M.col0) * 2;
  if (M.C & 1) {
    const int c = panel * 64 + lane;
    if (c < M.C) ds_chunk_column<1>(M.x, M.C, c, row0, n, part_row);
  } else {
    const int c = (panel * 64 + lane) * 2;
    if (c < M.C) ds_chunk_column<2>(M.x, M.C, c, row0, n, part_row);
  }
}

// One launch of the merge tree: the nodes are the entries part[i * stride] (i < ceil(chunks / stride)), node i covering the chunks
// [i * stride, (i + 1) * stride); thread (g, c) folds nodes 16 g .. 16 g + 15 of column c into node 16 g.  fin_mean != NULL (the
// launch with one group): also mean[c] = first[c] + offset and std[c] = sqrt(M2 / N).
__global__ void __launch_bounds__(256)
gs_k_ds_merge(double* __restrict__ part, long long chunks, int Ct, long long stride, long long N,
              const GsDsMatrix m0, const GsDsMatrix m1, const GsDsMatrix m2, double* __restrict__ fin_mean, double* __restrict__ fin_std) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long g = gid / Ct;
  const int c = (int)(gid - g * Ct);
  const long long first = g * 16 * stride;
  if (first >= chunks) return;
  DsNode v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const long long i = first + j * stride;             // first chunk of the node
    long long lo = i * GS_DS_ROWS_PER_CHUNK, hi = (i + stride) * GS_DS_ROWS_PER_CHUNK;
    if (hi > N) hi = N;
    v[j].n = i < chunks && hi > lo ? hi - lo : 0;
    v[j].off = 0.0; v[j].m2 = 0.0;
    if (v[j].n) {
      const double2 e = *(const double2*)(part + ((size_t)i * Ct + c) * 2);
      v[j].off = e.x; v[j].m2 = e.y;
    }
  }
#pragma unroll
  for (int s = 1; s < 16; s *= 2)
#pragma unroll
    for (int j = 0; j < 16; j += 2 * s) v[j] = ds_join(v[j], v[j + s]);
  *(double2*)(part + ((size_t)first * Ct + c) * 2) = make_double2(v[0].off, v[0].m2);
  if (fin_mean) {
    const GsDsMatrix& M = c >= m2.col0 ? m2 : (c >= m1.col0 ? m1 : m0);
    fin_mean[c] = M.x[c - M.col0] + v[0].off;
    fin_std[c] = sqrt(v[0].m2 / (double)N);
  }
}

// ---- the transition -> terminal-row map -------------------------------------------------------------------------------------
__global__ void gs_k_ds_map_fill(int32_t* __restrict__ map, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) map[i] = -1;
}

// entry k of the rollout's terminal list (t, b) -> map[t * B + b] = k; the list's length is read where the rollout left it
__global__ void gs_k_ds_map_scatter(int32_t* __restrict__ map, const int32_t* __restrict__ term_count, const int32_t* __restrict__ term_idx,
                                    int term_cap, int T, int B) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int cnt = *term_count < term_cap ? *term_count : term_cap;
  if (k >= cnt) return;
  const int t = term_idx[2 * k], b = term_idx[2 * k + 1];
  if (t >= 0 && t < T && b >= 0 && b < B) map[(size_t)t * B + b] = k;
}

// ---- sample indices drawn on the device ---------------------------------------------------------------------------------------
// sample i of call `draw` = word i & 3 of Philox(counter (i >> 2, draw lo, draw hi, 'SMPL'), key seed), idx = (word * N) >> 32
__global__ void gs_k_ds_draw(int32_t* __restrict__ idx, int n, long long N, uint64_t seed, uint64_t draw) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (4 * q >= n) return;
  const U4 r = philox((uint32_t)q, (uint32_t)draw, (uint32_t)(draw >> 32), 0x534D504Cu, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t w[4] = {r.a, r.b, r.c, r.d};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * q + k < n) idx[4 * q + k] = (int32_t)(((uint64_t)w[k] * (uint64_t)N) >> 32);
}

}  // extern "C"

// ---- the gather ------------------------------------------------------------------------------------------------------------------
namespace {

template <typename O> struct DsOut2;
template <> struct DsOut2<double> { typedef double2 type; };
template <> struct DsOut2<float> { typedef float2 type; };

// exactly (x - mean) / (std + 1e-6) in float64 (IEEE subtraction, addition and division), rounded once where O is float
template <typename O>
__device__ __forceinline__ O ds_norm(double x, double mean, double std, int normalize) {
  return (O)(normalize ? (x - mean) / (std + 1e-6) : x);
}

// One wave per sample, GS_DS_GATHER_ROWS samples per workgroup; lanes along the columns.  The observation and the next observation
// of a sample are produced in the same pass (they share the statistics a lane holds).
template <typename O>
__device__ __forceinline__ void ds_gather(const GsDsGatherArgs& G) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * GS_DS_GATHER_ROWS + (threadIdx.x >> 6);
  if (i >= G.n) return;
  const long long j = G.idx[i];
  if (j < 0 || j >= G.N) return;                       // (refused on the host / cannot be drawn)
  const int D = G.D, A = G.A;
  const int k = G.map[j];
  const double* src = G.obs_seq + (size_t)j * D;
  const double* nxt = (k >= 0 && k < G.term_cap) ? G.term_obs + (size_t)k * D : G.obs_seq + ((size_t)j + G.B) * D;
  O* o_obs = (O*)G.out_obs + (size_t)i * D;
  O* o_nxt = (O*)G.out_next + (size_t)i * D;
  const double* mean = G.stats; const double* std = G.stats + G.Cs;
  if (G.vec2) {
    typedef typename DsOut2<O>::type O2;
    for (int c = lane * 2; c < D; c += 128) {
      const double2 x = *(const double2*)(src + c), y = *(const double2*)(nxt + c);
      const double2 m = *(const double2*)(mean + c), s = *(const double2*)(std + c);
      O2 a, b;
      a.x = ds_norm<O>(x.x, m.x, s.x, G.normalize); a.y = ds_norm<O>(x.y, m.y, s.y, G.normalize);
      b.x = ds_norm<O>(y.x, m.x, s.x, G.normalize); b.y = ds_norm<O>(y.y, m.y, s.y, G.normalize);
      *(O2*)(o_obs + c) = a;
      *(O2*)(o_nxt + c) = b;
    }
  } else {
    for (int c = lane; c < D; c += 64) {
      const double m = mean[c], s = std[c];
      o_obs[c] = ds_norm<O>(src[c], m, s, G.normalize);
      o_nxt[c] = ds_norm<O>(nxt[c], m, s, G.normalize);
    }
  }
  for (int c = lane; c < A; c += 64)
    ((O*)G.out_act)[(size_t)i * A + c] = ds_norm<O>(G.act[(size_t)j * A + c], mean[D + c], std[D + c], G.normalize);
  if (lane == 0) {
    ((O*)G.out_rew)[i] = ds_norm<O>(G.rew[j], mean[D + A], std[D + A], G.normalize);
    ((O*)G.out_term)[i] = (G.done[j] & 3) ? (O)1 : (O)0;
  }
}

}  // namespace

extern "C" {

__global__ void __launch_bounds__(64 * GS_DS_GATHER_ROWS)
gs_k_ds_gather_f64(GsDsGatherArgs G) { ds_gather<double>(G); }

__global__ void __launch_bounds__(64 * GS_DS_GATHER_ROWS)
gs_k_ds_gather_f32(GsDsGatherArgs G) { ds_gather<float>(G); }

}  // extern "C"
