// kernels_policy.hip -- the MLP policy of gs_rollout(GS_POLICY_MLP) / gs_policy_mlp_eval: every layer of the reference's actor
// (algorithms/base.py:157-177 `_build_mlp`; head: algorithms/offline.py:69-76, 114-136) in ONE launch, float64 on the matrix cores.
//
// Mapping.  A workgroup of four wavefronts owns GS_POL_ROWS = 32 instances (B = 8192: 256 workgroups, one per compute unit).  A
// layer is  out[32][N] = in[32][K] W^T + b  as v_mfma_f64_16x16x4_f64 products (operand maps: A[row = lane & 15][k = lane >> 4],
// B[k = lane >> 4][col = lane & 15], C/D[row = (lane >> 4) + 4 reg][col = lane & 15]):
//   - the A operand is the layer's input: the observation rows straight from global memory for the first layer (one 16-byte load
//     per lane gives the operands of two k-steps: k = 8 kb + 2 (lane >> 4) + j, j = 0, 1 -- any assignment of k to steps is a valid
//     product as long as both operands use it), the activations in LDS for the others (32 rows x 264 doubles = 66 KB);
//   - the B operand is the weight matrix, packed by the host in exactly that order (policy.h: [column tile][k block][lane][2]), so a
//     wavefront's load of one tile and block is 1 KB contiguous; the matrices stream from L2 (684 x 256 doubles = 1.4 MB);
//   - wavefront w takes column tiles w, w + 4, w + 8, w + 12 for both row tiles: 8 accumulators of 4 doubles, and per k block
//     2 input + 4 weight loads feed 16 products.  The operands of the next two k blocks are loaded before the products of the
//     current two are issued (one wavefront per SIMD: nothing else hides the load latency).
// Between layers all four wavefronts meet at a barrier, add the bias, apply the activation and write their columns to LDS; padded
// columns come out as act(0) = 0 (zero weights and bias), which is what the next layer's padded k range expects.  The head reads
// the last layer's rows from LDS, one thread per (instance, action); for a sampling policy with P.logp set it also files the
// action's log-probability term in LDS, and one thread per instance adds them in action order (policy_head.h).
#include <hip/hip_runtime.h>
#include <math.h>

#include "env_device.h"
#include "policy.h"
#include "policy_head.h"

typedef double gp_v4 __attribute__((ext_vector_type(4)));
typedef double gp_v2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int GP_RT = GS_POL_ROWS / 16;      // row tiles per workgroup
constexpr int GP_CT = 4;                     // column tiles per wavefront (16 tiles of a 256-wide layer over four wavefronts)
static_assert(GP_CT * GS_POL_WAVES * 16 >= GS_POL_MAX_WIDTH, "every column tile of the widest layer has a wavefront");

// the input operands of k blocks kb, kb + 1 for this lane: rows 16 rt + (lane & 15), k = 8 kb + 2 (lane >> 4) + {0, 1}
template <bool EVEN>
struct GpSrcObs {      // observation rows in global memory; row clamped to the batch, columns beyond D read as zero
  const double* row[GP_RT]; int D;
  __device__ __forceinline__ gp_v2 get(int rt, int k) const {
    if (EVEN) {        // D even: k even, so k < D means k + 1 < D, and the address is 16-byte aligned
      const gp_v2 v = *(const gp_v2*)(row[rt] + min(k, D - 2));
      return k < D ? v : gp_v2{0.0, 0.0};
    }
    const double a = row[rt][min(k, D - 1)], b = row[rt][min(k + 1, D - 1)];
    return gp_v2{k < D ? a : 0.0, k + 1 < D ? b : 0.0};
  }
};
struct GpSrcLds {      // activations of the previous layer
  const double* row[GP_RT];
  __device__ __forceinline__ gp_v2 get(int rt, int k) const { return *(const gp_v2*)(row[rt] + k); }
};

struct GpFrag { gp_v2 x[2][GP_RT], w[2][GP_CT]; };       // [k block of the pair][tile]

// FULL: the layer has all sixteen column tiles, so every wavefront has its four (no predicates in the loop)
template <bool FULL, class Src>
__device__ __forceinline__ void gp_load(GpFrag& f, const Src& src, const double* __restrict__ wl, int kb_total, int kb, int nt, int wave, int lane) {
  const int kq = 2 * (lane >> 4);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int rt = 0; rt < GP_RT; ++rt) f.x[s][rt] = src.get(rt, 8 * (kb + s) + kq);
#pragma unroll
    for (int c = 0; c < GP_CT; ++c) {
      const int tile = wave + GS_POL_WAVES * c;
      if (FULL || tile < nt) f.w[s][c] = *(const gp_v2*)(wl + (((size_t)tile * kb_total + kb + s) * 64 + lane) * 2);
    }
  }
}

// acc[rt][c] = in[rows of tile rt][:] W[columns of tile wave + 4 c][:]^T
template <bool FULL, class Src>
__device__ __forceinline__ void gp_layer(gp_v4 (&acc)[GP_RT][GP_CT], const Src& src, const GsPolicyLayer& L, int wave, int lane) {
#pragma unroll
  for (int rt = 0; rt < GP_RT; ++rt)
#pragma unroll
    for (int c = 0; c < GP_CT; ++c) acc[rt][c] = gp_v4{0.0, 0.0, 0.0, 0.0};
  if (!FULL && wave >= L.nt) return;         // (a narrow layer: this wavefront has no column tile)
  GpFrag cur, nxt;
  gp_load<FULL>(cur, src, L.w, L.kb, 0, L.nt, wave, lane);
  for (int kb = 0; kb < L.kb; kb += 2) {
    if (kb + 2 < L.kb) gp_load<FULL>(nxt, src, L.w, L.kb, kb + 2, L.nt, wave, lane);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < GP_CT; ++c) {
          if (!FULL && wave + GS_POL_WAVES * c >= L.nt) continue;
#pragma unroll
          for (int rt = 0; rt < GP_RT; ++rt)
            acc[rt][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.x[s][rt][j], cur.w[s][c][j], acc[rt][c], 0, 0, 0);
        }
    cur = nxt;
  }
}

__device__ __forceinline__ double gp_activation(double x, int kind) {
  if (kind == GS_ACT_RELU) return x > 0.0 ? x : 0.0;
  if (kind == GS_ACT_TANH) return tanh(x);
  return x > 0.0 ? x : expm1(x);             // elu, alpha = 1
}

// component `comp` of the four normals of one Philox call (env_device.h's rng_normal_component), tag 'PNOI'
__device__ __forceinline__ double gp_noise(uint64_t seed, uint64_t instance, uint32_t t, uint32_t quad, int comp) {
  const U4 r = philox((uint32_t)instance, t, quad, 0x504E4F49u, (uint32_t)seed, (uint32_t)(seed >> 32));
  return rng_normal_component(r, comp);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64 * GS_POL_WAVES)
gs_k_policy_mlp(GsPolicyArgs P) {
  extern __shared__ __attribute__((aligned(16))) double gp_lds[];         // [GS_POL_ROWS][GS_POL_LDS_STRIDE]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * GS_POL_ROWS;
  gp_v4 acc[GP_RT][GP_CT];
  for (int l = 0; l < P.n_layers; ++l) {
    const GsPolicyLayer L = P.L[l];
    const bool full = L.nt == GP_CT * GS_POL_WAVES;
    if (l == 0 && !(P.D & 1)) {
      GpSrcObs<true> src;
      src.D = P.D;
#pragma unroll
      for (int rt = 0; rt < GP_RT; ++rt) src.row[rt] = P.obs + (size_t)min(row0 + 16 * rt + (lane & 15), P.B - 1) * P.D;
      if (full) gp_layer<true>(acc, src, L, wave, lane);
      else gp_layer<false>(acc, src, L, wave, lane);
    } else if (l == 0) {
      GpSrcObs<false> src;
      src.D = P.D;
#pragma unroll
      for (int rt = 0; rt < GP_RT; ++rt) src.row[rt] = P.obs + (size_t)min(row0 + 16 * rt + (lane & 15), P.B - 1) * P.D;
      gp_layer<false>(acc, src, L, wave, lane);
    } else {
      GpSrcLds src;
#pragma unroll
      for (int rt = 0; rt < GP_RT; ++rt) src.row[rt] = gp_lds + (16 * rt + (lane & 15)) * GS_POL_LDS_STRIDE;
      if (full) gp_layer<true>(acc, src, L, wave, lane);
      else gp_layer<false>(acc, src, L, wave, lane);
    }
    __syncthreads();                         // every wavefront has read the previous activations
    const bool last = l == P.n_layers - 1;
#pragma unroll
    for (int c = 0; c < GP_CT; ++c) {
      const int tile = wave + GS_POL_WAVES * c;
      if (tile >= L.nt) continue;
      const int col = 16 * tile + (lane & 15);
      const double bias = L.b[col];
#pragma unroll
      for (int rt = 0; rt < GP_RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double v = acc[rt][c][r] + bias;
          gp_lds[(16 * rt + (lane >> 4) + 4 * r) * GS_POL_LDS_STRIDE + col] = last ? v : gp_activation(v, P.activation);
        }
    }
    __syncthreads();
  }
  // head: a = tanh(mean) or tanh(mean + exp(clamp(log_std, -20, 2)) eps); with P.logp the sampled action's log-probability term
  // as well, into LDS: columns 2 A .. 3 A - 1 of the row where the tile has them, behind the tile otherwise (P.logp_behind)
  const bool sample = P.head == GS_HEAD_GAUSSIAN_TANH && P.stochastic;
  double* const terms = P.logp_behind ? gp_lds + GS_POL_ROWS * GS_POL_LDS_STRIDE : gp_lds + 2 * P.A;
  const int tstride = P.logp_behind ? P.A : GS_POL_LDS_STRIDE;
  for (int idx = threadIdx.x; idx < GS_POL_ROWS * P.A; idx += blockDim.x) {
    const int r = idx / P.A, a = idx - r * P.A, b = row0 + r;
    if (b >= P.B) break;
    double x = gp_lds[r * GS_POL_LDS_STRIDE + a];
    if (sample) {
      const double ls = fmin(fmax(gp_lds[r * GS_POL_LDS_STRIDE + P.A + a], -20.0), 2.0);
      const double eps = gp_noise(P.seed, (uint64_t)(P.first_instance + b), (uint32_t)P.t, (uint32_t)(a >> 2), a & 3);
      x += exp(ls) * eps;
      const double act = tanh(x);
      P.act[(size_t)b * P.A + a] = act;
      if (P.logp) terms[r * tstride + a] = gs_logp_term(eps, ls, act);
    } else {
      P.act[(size_t)b * P.A + a] = tanh(x);
    }
  }
  if (sample && P.logp) gs_logp_rows<GS_POL_ROWS>(terms, tstride, P.A, row0, P.B, P.logp);
}
