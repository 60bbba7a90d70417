// kernels_fed.hip -- one federated round over the learners of K handles (fed.h; include/gridstep.h "the federation"; DESIGN.md
// section 20):
//   gs_k_fed_gram     per entry (i, k) and per 1024 parameters: the float64 sum of d_i[j] d_k[j], d = p - g
//   gs_k_fed_sum      ONE workgroup per entry over the workgroups' sums; for a round also norm_k, c_k and a_k
//   gs_k_fed_apply    one thread per parameter: g' from g and the participants' updates (and the noise), stored into g and into every
//                     client's master parameters, forward image and transposed image; Adam's moments zeroed on request
// All arithmetic is float64 on the float32 values, nothing is contracted, and there are no floating-point atomics: every sum has an
// order fixed by P and the list of participants.
#include <hip/hip_runtime.h>
#include <math.h>

#include "block_reduce.h"
#include "env_device.h"
#include "fed.h"

namespace {

// component `comp` of the four normals of one Philox call (env_device.h's rng_normal_component), tag 'FEDN'
__device__ __forceinline__ double gf_noise(uint64_t seed, uint32_t quad, uint32_t round, uint32_t net, int comp) {
  const U4 r = philox(quad, round, net, 0x4645444Eu, (uint32_t)seed, (uint32_t)(seed >> 32));
  return rng_normal_component(r, comp);
}

}  // namespace

// ---- the updates' products, 1024 parameters a workgroup ----------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(GS_FED_RED_THREADS)
gs_k_fed_gram(GsFedGramArgs A) {
#pragma clang fp contract(off)
  __shared__ double lds[GS_FED_RED_THREADS / 64];
  const int e = blockIdx.y;
  const int qi = A.pairs ? A.pairs[2 * e] : e, qk = A.pairs ? A.pairs[2 * e + 1] : e;
  const float* __restrict__ pi = A.clients[A.part[qi]].params;
  const float* __restrict__ pk = A.clients[A.part[qk]].params;
  const int base = blockIdx.x * GS_FED_BLOCK;
  double ss = 0.0;
  for (int r = 0; r < GS_FED_RED_PER_THREAD; ++r) {
    const int j = base + r * GS_FED_RED_THREADS + (int)threadIdx.x;
    if (j >= A.P) break;
    const double g = (double)A.g[j];
    const double di = (double)pi[j] - g, dk = (double)pk[j] - g;
    ss = ss + di * dk;
  }
  ss = gs_block_sum(ss, lds);
  if (threadIdx.x == 0) A.blocksum[(size_t)e * A.blocks + blockIdx.x] = ss;
}

// ---- one entry's sum over the workgroups; a round's coefficients -------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(GS_FED_SUM_THREADS)
gs_k_fed_sum(GsFedSumArgs A) {
#pragma clang fp contract(off)
  __shared__ double lds[GS_FED_SUM_THREADS / 64];
  const int e = blockIdx.x;
  const double* __restrict__ src = A.blocksum + (size_t)e * A.blocks;
  double s = 0.0;
  for (int k = threadIdx.x; k < A.blocks; k += GS_FED_SUM_THREADS) s = s + src[k];
  s = gs_block_sum(s, lds);
  if (threadIdx.x) return;
  A.out[e] = s;
  if (!A.coef) return;
  const double norm = sqrt(s);
  double c = 1.0;
  if (A.clip_norm > 0.0) {
    c = A.clip_norm / (norm + 1e-6);
    c = c < 1.0 ? c : 1.0;
  }
  A.stats[e] = norm;
  A.stats[GS_FED_MAX_CLIENTS + e] = c;
  A.stats[2 * GS_FED_MAX_CLIENTS + e] = A.u[e] * c;
}

// ---- the new global parameters, into g and into every client ------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(GS_FED_APPLY_THREADS)
gs_k_fed_apply(GsFedApplyArgs A) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.S.P) return;
  float w = A.g[j];
  if (A.n > 0) {
    const double g = (double)w;
    double s = 0.0;
    for (int k = 0; k < A.n; ++k) {
      const double d = (double)A.clients[A.part[k]].params[j] - g;
      s = s + A.stats[2 * GS_FED_MAX_CLIENTS + k] * d;
    }
    double x = g + s;
    if (A.noise_std > 0.0) x = x + A.noise_std * gf_noise(A.seed, (uint32_t)j >> 2, A.round, (uint32_t)A.net, j & 3);
    w = (float)x;
    A.g[j] = w;
  }
  int l = 0;
  while (l + 1 < A.S.n_layers && j >= A.S.p_off[l + 1]) ++l;
  const int n_out = A.S.dims[l + 1], n_in = A.S.dims[l], local = j - A.S.p_off[l];
  const bool bias = local >= n_out * n_in;
  const int o = bias ? local - n_out * n_in : local / n_in, k = bias ? 0 : local - o * n_in;
  const size_t slot = bias ? (size_t)o : gs_pol32_slot(o, k, A.S.kb[l]);
  const size_t slot_t = !bias && l ? gs_pol32_slot(k, o, A.S.kbt[l]) : 0;      // (W^T: the output index is k, the k axis runs over o)
  for (int c = 0; c < A.n_clients; ++c) {
    const GsFedClient& C = A.clients[c];
    C.params[j] = w;
    if (A.reset_moments) { C.m[j] = 0.0f; C.v[j] = 0.0f; }
    if (bias) { C.b[l][slot] = w; continue; }
    C.w[l][slot] = w;
    if (l) C.t[l][slot_t] = w;
  }
}
