// kernels_train.hip -- one PPO / critic update on a minibatch (train.h; include/gridstep.h "the learner"):
//   gs_k_train_forward    the layers of mlp_f32.h on the float32 minibatch, 32 rows a workgroup; every layer's output saved
//   gs_k_train_head       per sample, float64 on the float32 pre-head values: log-probability, ratio, clip flag, loss terms, and
//                         dL / d(pre-head) rounded once to float32
//   gs_k_train_bwd_data   delta_l = (delta_{l+1} W_{l+1}) * act'(y_l), the same product loop over the packed image of W^T
//   gs_k_train_grad       dW_l = delta_l^T a_{l-1}, db_l = column sums, one partial per segment of GS_TR_SEG rows
//   gs_k_train_reduce     the partials added in ascending segment order; the squares of the result summed in float64 per workgroup
//   gs_k_train_stats      ONE workgroup: the loss statistics and the gradient norm, in section 17's fixed order
//   gs_k_train_adam       Adam on the master parameters; the same thread refreshes the forward and the transposed image
// Every product of the three matrix kernels runs on v_mfma_f32_16x16x4_f32.  No floating-point atomics: every sum has an order fixed
// by the network's shape and n.
#include <hip/hip_runtime.h>
#include <math.h>

#include "block_reduce.h"
#include "bootstrap.h"
#include "mlp_f32.h"
#include "train.h"

namespace {

constexpr int GT_RT = GS_TR_ROWS / 16;
constexpr int GT_SPLIT = 4;                 // accumulator sets of the forward pass (the epilogue adds four)

// columns [16 kb0, 16 kb1) of rows row0 .. row0 + GS_TR_ROWS - 1 (clamped to n) of the float32 matrix src (row stride `ld`, columns
// beyond `cols` read as 0) into `tile`; wavefront w takes rows w, w + 4, ..., a lane one column
__device__ __forceinline__ void gt_stage(const float* __restrict__ src, int ld, int cols, int n, int stride, float* tile, int row0, int kb0, int kb1,
                                         int wave, int lane) {
  const int width = 16 * (kb1 - kb0);
  for (int r = wave; r < GS_TR_ROWS; r += GS_POL_WAVES) {
    const float* s = src + (size_t)min(row0 + r, n - 1) * ld;
    for (int c = lane; c < width; c += 64) {
      const int k = 16 * kb0 + c;
      tile[r * stride + c] = k < cols ? s[k] : 0.0f;
    }
  }
}

// act'(x) from the saved output y = act(x)
__device__ __forceinline__ float gt_act_grad(float y, int kind) {
  if (kind == GS_ACT_RELU) return y > 0.0f ? 1.0f : 0.0f;
  if (kind == GS_ACT_TANH) return 1.0f - y * y;
  return y > 0.0f ? 1.0f : y + 1.0f;         // elu, alpha = 1: exp(x) = y + 1
}

}  // namespace

// ---- forward -------------------------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(64 * GS_POL_WAVES)
gs_k_train_forward(GsTrainFwdArgs P) {
  extern __shared__ __attribute__((aligned(16))) float gt_lds[];
  float* const act_lds = gt_lds;                                           // [GS_TR_ROWS][GS_POL32_ACT_STRIDE]
  float* const obs_lds = gt_lds + GS_TR_ROWS * GS_POL32_ACT_STRIDE;        // [GS_TR_ROWS][P.obs_stride]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * GS_TR_ROWS;
  if (row0 >= P.n) return;
  const int last = P.N.n_layers - 1;
  // GT_SPLIT accumulator sets, each over a quarter of the k blocks (of every panel), added pairwise at the end: a sum over 684
  // inputs is four chains of 43 k-steps instead of one of 172, which is what a blocked host matrix product's error is measured by
  gq_v4 acc[GT_SPLIT][GT_RT][GQ_CT];
#pragma unroll 1
  for (int l = 0; l <= last; ++l) {
    const GsPolicyLayerF32 L = P.N.L[l];
    const bool full = L.nt == GQ_CT * GS_POL_WAVES;
#pragma unroll
    for (int s = 0; s < GT_SPLIT; ++s)
#pragma unroll
      for (int rt = 0; rt < GT_RT; ++rt)
#pragma unroll
        for (int c = 0; c < GQ_CT; ++c) acc[s][rt][c] = gq_v4{0.0f, 0.0f, 0.0f, 0.0f};
    const int stride = l == 0 ? P.obs_stride : GS_POL32_ACT_STRIDE;
    const float* const src = l == 0 ? obs_lds : act_lds;
    const int panel = l == 0 ? P.panel_kb : L.kb;
    for (int kb0 = 0; kb0 < L.kb; kb0 += panel) {
      const int kb1 = min(kb0 + panel, L.kb);
      if (l == 0) {
        if (kb0) __syncthreads();            // every wavefront has read the previous panel
        gt_stage(P.obs, P.D, P.D, P.n, P.obs_stride, obs_lds, row0, kb0, kb1, wave, lane);
        __syncthreads();
      }
#pragma unroll
      for (int s = 0; s < GT_SPLIT; ++s) {
        const int k0 = kb0 + (kb1 - kb0) * s / GT_SPLIT, k1 = kb0 + (kb1 - kb0) * (s + 1) / GT_SPLIT;
        if (k1 <= k0) continue;
        const float* in[GT_RT];               // this lane's operand of block k0 (gq_layer counts its LDS offsets from its first block)
#pragma unroll
        for (int rt = 0; rt < GT_RT; ++rt) in[rt] = src + (16 * rt + (lane & 15)) * stride + 4 * (lane >> 4) + 16 * (k0 - kb0);
        if (full) gq_layer<GT_RT, true>(acc[s], in, L, k0, k1, wave, lane);
        else gq_layer<GT_RT, false>(acc[s], in, L, k0, k1, wave, lane);
      }
    }
    __syncthreads();                         // every wavefront has read the previous activations
    float* const saved = P.acts + P.N.col_off[l];
#pragma unroll
    for (int c = 0; c < GQ_CT; ++c) {
      const int tile = wave + GS_POL_WAVES * c;
      if (tile >= L.nt) continue;
      const int col = 16 * tile + (lane & 15);
      const float bias = L.b[col];
#pragma unroll
      for (int rt = 0; rt < GT_RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * rt + 4 * (lane >> 4) + r;
          float v = ((acc[0][rt][c][r] + acc[1][rt][c][r]) + (acc[2][rt][c][r] + acc[3][rt][c][r])) + bias;
          if (l < last) {
            v = gq_activation(v, P.N.activation);
            act_lds[row * GS_POL32_ACT_STRIDE + col] = v;
          }
          if (row0 + row < P.n) saved[(size_t)(row0 + row) * P.N.row_stride + col] = v;
        }
    }
    __syncthreads();
  }
}

// ---- the head: loss terms and dL / d(pre-head) ---------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(64)
gs_k_train_head(GsTrainHeadArgs H) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H.n) return;
  const float* pre = H.pre + (size_t)i * H.row_stride;
  float* g = H.ghead + (size_t)i * H.row_stride;
  const double inv_n = 1.0 / (double)H.n;
  if (H.A == 0) {                            // a critic: L = mean (v - ret)^2
    const double d = (double)pre[0] - (double)H.ret[i];
    H.term0[i] = d * d;
    g[0] = (float)((2.0 * d) * inv_n);
    for (int k = 1; k < H.width16; ++k) g[k] = 0.0f;
    return;
  }
  const int A = H.A;
  const long long j = gb_row(H.idx[i], H.N);
  const double* act = H.act + (size_t)j * A;
  const double lp_old = H.logp[j], adv = (double)H.adv[i];
  const double lim = 1.0 - 1e-7;
  double lp = 0.0, ent = 0.0;
  for (int k = 0; k < A; ++k) {
    const double mean = (double)pre[k], lsr = (double)pre[A + k];
    const double ls = fmin(fmax(lsr, -20.0), 2.0);
    const double a = act[k];
    const double x = atanh(fmin(fmax(a, -lim), lim));
    const double e = (x - mean) * exp(-ls);
    const double term = (((-0.5 * e) * e - ls) - 0.91893853320467274178) - log((1.0 - a * a) + 1e-6);
    lp = k ? lp + term : term;
    const double h = ls + 1.4189385332046727418;      // 0.5 log(2 pi e)
    ent = k ? ent + h : h;
  }
  const double r = exp(lp - lp_old);
  const double lo = 1.0 - H.clip, hi = 1.0 + H.clip;
  const double rc = fmin(fmax(r, lo), hi);
  const bool clipped = (adv > 0.0 && r > hi) || (adv < 0.0 && r < lo);
  H.lp_new[i] = lp; H.ratio[i] = r; H.clipped[i] = clipped ? 1 : 0;
  H.term0[i] = fmin(r * adv, rc * adv);
  H.term1[i] = ent;
  const double dlp = clipped ? 0.0 : -((r * adv) * inv_n);
  const double dent = -(H.ent_coef * inv_n);
  for (int k = 0; k < A; ++k) {
    const double mean = (double)pre[k], lsr = (double)pre[A + k];
    const bool inside = lsr >= -20.0 && lsr <= 2.0;
    const double ls = fmin(fmax(lsr, -20.0), 2.0);
    const double x = atanh(fmin(fmax(act[k], -lim), lim));
    const double inv = exp(-ls);
    const double e = (x - mean) * inv;
    g[k] = (float)(dlp * (e * inv));
    g[A + k] = inside ? (float)(dlp * (e * e - 1.0) + dent) : 0.0f;
  }
  for (int k = 2 * A; k < H.width16; ++k) g[k] = 0.0f;
}

// ---- backward, data ------------------------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(64 * GS_POL_WAVES)
gs_k_train_bwd_data(GsTrainBwdArgs P) {
  __shared__ __attribute__((aligned(16))) float d_lds[GS_TR_ROWS * GS_POL32_ACT_STRIDE];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * GS_TR_ROWS;
  if (row0 >= P.n) return;
  const int last = P.N.n_layers - 1, rs = P.N.row_stride;
  gt_stage(P.deltas + P.N.col_off[last], rs, 16 * P.N.L[last].nt, P.n, GS_POL32_ACT_STRIDE, d_lds, row0, 0, P.N.L[last].nt, wave, lane);
  __syncthreads();
  const float* in[GT_RT];
#pragma unroll
  for (int rt = 0; rt < GT_RT; ++rt) in[rt] = d_lds + (16 * rt + (lane & 15)) * GS_POL32_ACT_STRIDE + 4 * (lane >> 4);
  gq_v4 acc[GT_RT][GQ_CT];
  for (int l = last - 1; l >= 0; --l) {
    const GsPolicyLayerF32 T = P.N.T[l + 1];       // kb: the column tiles of layer l + 1; nt: those of layer l
    const bool full = T.nt == GQ_CT * GS_POL_WAVES;
#pragma unroll
    for (int rt = 0; rt < GT_RT; ++rt)
#pragma unroll
      for (int c = 0; c < GQ_CT; ++c) acc[rt][c] = gq_v4{0.0f, 0.0f, 0.0f, 0.0f};
    if (full) gq_layer<GT_RT, true>(acc, in, T, 0, T.kb, wave, lane);
    else gq_layer<GT_RT, false>(acc, in, T, 0, T.kb, wave, lane);
    __syncthreads();                         // every wavefront has read delta_{l+1}
    const float* const y = P.acts + P.N.col_off[l];
    float* const out = P.deltas + P.N.col_off[l];
#pragma unroll
    for (int c = 0; c < GQ_CT; ++c) {
      const int tile = wave + GS_POL_WAVES * c;
      if (tile >= T.nt) continue;
      const int col = 16 * tile + (lane & 15);
#pragma unroll
      for (int rt = 0; rt < GT_RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * rt + 4 * (lane >> 4) + r;
          const size_t at = (size_t)min(row0 + row, P.n - 1) * rs + col;
          const float d = acc[rt][c][r] * gt_act_grad(y[at], P.N.activation);
          d_lds[row * GS_POL32_ACT_STRIDE + col] = d;
          if (row0 + row < P.n) out[at] = d;
        }
    }
    __syncthreads();
  }
}

// ---- backward, weights ---------------------------------------------------------------------------------------------------------------
// One wavefront per (layer, 32 outputs, 64 inputs, segment): the rows of the segment are the k axis, four a k-step.  Operand A of a
// k-step is delta[row + (lane >> 4)][out tile's column lane & 15], operand B the input activation at the same row; lane (i, q) of an
// accumulator then holds dW[16 tile_o + 4 q + r][16 tile_i + i].  Consecutive k-steps go to GS_TR_CHAINS accumulator sets in turn
// (k-step t to set t mod 4), added as (c0 + c1) + (c2 + c3) at the end: a segment's sum is four chains of at most sixteen k-steps.
// db: every lane adds its delta operands per chain (rows = q mod 4), the chains are added the same way, then the four q as
// (q0 + q1) + (q2 + q3).
extern "C" __global__ void __launch_bounds__(64)
gs_k_train_grad(GsTrainGradArgs P) {
#pragma clang fp contract(off)
  constexpr int WO = GS_TR_WT_OUT, WI = GS_TR_WT, CH = GS_TR_CHAINS;
  const int lane = threadIdx.x, q = lane >> 4, i = lane & 15;
  int l = 0;
  while (l + 1 < P.N.n_layers && (int)blockIdx.x >= P.blk0[l + 1]) ++l;
  const int local = blockIdx.x - P.blk0[l];
  const int bo = local / P.in_blocks[l], bi = local - bo * P.in_blocks[l], seg = blockIdx.y;
  const int n_out = P.N.dims[l + 1], n_in = P.N.dims[l], nt_out = P.N.L[l].nt, rs = P.N.row_stride;
  const float* const dA = P.deltas + P.N.col_off[l];
  const float* const aB = l == 0 ? P.obs : P.acts + P.N.col_off[l - 1];
  const int ldb = l == 0 ? P.D : rs;
  const int bcols = l == 0 ? P.D : 16 * P.N.L[l - 1].nt;
  const int r_begin = seg * GS_TR_SEG, r_end = min(P.n, r_begin + GS_TR_SEG);
  int ocol[WO], icol[WI];
  bool ook[WO], iok[WI];
#pragma unroll
  for (int a = 0; a < WO; ++a) { ocol[a] = 16 * (WO * bo + a) + i; ook[a] = WO * bo + a < nt_out; }
#pragma unroll
  for (int b = 0; b < WI; ++b) { icol[b] = 16 * (WI * bi + b) + i; iok[b] = icol[b] < bcols; }
  gq_v4 acc[CH][WO][WI];
  float dbias[CH][WO];
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int a = 0; a < WO; ++a) {
      dbias[c][a] = 0.0f;
#pragma unroll
      for (int b = 0; b < WI; ++b) acc[c][a][b] = gq_v4{0.0f, 0.0f, 0.0f, 0.0f};
    }
  for (int r0 = r_begin; r0 < r_end; r0 += 4 * CH) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int r = r0 + 4 * c;
      const bool ok = r + q < r_end;         // (a k-step past the segment's end adds zeros)
      const size_t row = ok ? r + q : r_begin;
      float av[WO], bv[WI];
#pragma unroll
      for (int a = 0; a < WO; ++a) av[a] = ok && ook[a] ? dA[row * rs + ocol[a]] : 0.0f;
#pragma unroll
      for (int b = 0; b < WI; ++b) bv[b] = ok && iok[b] ? aB[row * ldb + icol[b]] : 0.0f;
#pragma unroll
      for (int a = 0; a < WO; ++a) {
        dbias[c][a] += av[a];
#pragma unroll
        for (int b = 0; b < WI; ++b) acc[c][a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[c][a][b], 0, 0, 0);
      }
    }
  }
  float* const part = P.partial + (size_t)seg * P.N.P + P.N.p_off[l];
#pragma unroll
  for (int a = 0; a < WO; ++a) {
#pragma unroll
    for (int b = 0; b < WI; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = 16 * (WO * bo + a) + 4 * q + r;
        const float v = (acc[0][a][b][r] + acc[1][a][b][r]) + (acc[2][a][b][r] + acc[3][a][b][r]);
        if (o < n_out && icol[b] < n_in) part[(size_t)o * n_in + icol[b]] = v;
      }
    if (bi == 0) {
      const float d = (dbias[0][a] + dbias[1][a]) + (dbias[2][a] + dbias[3][a]);
      float s = d + __shfl_xor(d, 16);
      s = s + __shfl_xor(s, 32);
      if (q == 0 && ocol[a] < n_out) part[(size_t)n_out * n_in + ocol[a]] = s;
    }
  }
}

// ---- the partials in ascending segment order; the squares of the result per workgroup ------------------------------------------------
extern "C" __global__ void __launch_bounds__(GS_TR_RED_THREADS)
gs_k_train_reduce(GsTrainReduceArgs A) {
#pragma clang fp contract(off)
  __shared__ double lds[GS_TR_RED_THREADS / 64];
  const int base = blockIdx.x * (GS_TR_RED_THREADS * GS_TR_RED_PER_THREAD);
  double ss = 0.0;
  for (int k = 0; k < GS_TR_RED_PER_THREAD; ++k) {
    const int p = base + k * GS_TR_RED_THREADS + (int)threadIdx.x;
    if (p >= A.P) break;
    float g = A.partial[p];
    for (int s = 1; s < A.segments; ++s) g = g + A.partial[(size_t)s * A.P + p];
    A.grad[p] = g;
    ss = ss + (double)g * (double)g;
  }
  ss = gs_block_sum(ss, lds);
  if (threadIdx.x == 0) A.blocksum[blockIdx.x] = ss;
}

// ---- statistics of the step: ONE workgroup, thread i over entries i, i + 1024, ..., then the tree of gs_block_sum --------------------
extern "C" __global__ void __launch_bounds__(GS_TR_STAT_THREADS)
gs_k_train_stats(GsTrainStatArgs S) {
#pragma clang fp contract(off)
  __shared__ double lds[GS_TR_STAT_THREADS / 64];
  __shared__ long long lds_i[GS_TR_STAT_THREADS / 64];
  const int tid = threadIdx.x;
  const double nan = __builtin_nan("");
  double t0 = 0.0, t1 = 0.0, kl = 0.0, gs = 0.0;
  long long nc = 0;
  for (int k = tid; k < S.n; k += GS_TR_STAT_THREADS) {
    t0 = t0 + S.term0[k];
    if (S.policy) {
      t1 = t1 + S.term1[k];
      const long long j = gb_row(S.idx[k], S.N);
      kl = kl + (S.logp[j] - S.lp_new[k]);
      nc += S.clipped[k];
    }
  }
  for (int k = tid; k < S.blocks; k += GS_TR_STAT_THREADS) gs = gs + S.blocksum[k];
  t0 = gs_block_sum(t0, lds);
  gs = gs_block_sum(gs, lds);
  if (S.policy) { t1 = gs_block_sum(t1, lds); kl = gs_block_sum(kl, lds); nc = gs_block_sum(nc, lds_i); }
  if (tid) return;
  const double n = (double)S.n;
  double* o = S.stats;
  if (S.policy) {
    const double surr = t0 / n, ent = t1 / n;
    o[GS_TR_STAT_LOSS] = -surr - S.ent_coef * ent;
    o[GS_TR_STAT_SURR] = surr; o[GS_TR_STAT_ENT] = ent; o[GS_TR_STAT_KL] = kl / n; o[GS_TR_STAT_CLIPFRAC] = (double)nc / n;
    o[GS_TR_STAT_VLOSS] = nan;
  } else {
    const double vl = t0 / n;
    o[GS_TR_STAT_LOSS] = vl; o[GS_TR_STAT_VLOSS] = vl;
    o[GS_TR_STAT_SURR] = nan; o[GS_TR_STAT_ENT] = nan; o[GS_TR_STAT_KL] = nan; o[GS_TR_STAT_CLIPFRAC] = nan;
  }
  o[GS_TR_STAT_GNORM] = sqrt(gs);
}

// ---- Adam, and the images the rollout, critic and learner kernels read ---------------------------------------------------------------
// Every operation is one correctly rounded float32 operation, in the order include/gridstep.h states; nothing is contracted.
extern "C" __global__ void __launch_bounds__(256)
gs_k_train_adam(GsTrainAdamArgs A) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= A.N.P) return;
  int l = 0;
  while (l + 1 < A.N.n_layers && p >= A.N.p_off[l + 1]) ++l;
  float g = A.grad[p];
  if (A.max_grad_norm > 0.0) {
    double sc = A.max_grad_norm / (A.stats[GS_TR_STAT_GNORM] + 1e-6);
    sc = sc < 1.0 ? sc : 1.0;
    g = g * (float)sc;
  }
  float w = A.params[p];
  if (A.wd != 0.0f) g = g + A.wd * w;
  const float m = A.b1 * A.m[p] + A.omb1 * g;
  const float v = A.b2 * A.v[p] + (A.omb2 * g) * g;
  const float denom = sqrtf(v) / A.bc2s + A.eps;      // (sqrtf and / are correctly rounded: the compiler's default for HIP)
  w = w - A.step * (m / denom);
  A.params[p] = w; A.m[p] = m; A.v[p] = v;
  const int n_out = A.N.dims[l + 1], n_in = A.N.dims[l], local = p - A.N.p_off[l];
  const GsPolicyLayerF32 L = A.N.L[l];
  if (local >= n_out * n_in) {
    const_cast<float*>(L.b)[local - n_out * n_in] = w;
    return;
  }
  const int o = local / n_in, k = local - o * n_in;
  // (policy.h's gs_pol32_slot(o, k, L.kb) and gs_pol32_slot(k, o, T.kb), written out: through the function the registers are allocated differently)
  const_cast<float*>(L.w)[(((size_t)(o >> 4) * L.kb + (k >> 4)) * 64 + ((k & 15) >> 2) * 16 + (o & 15)) * 4 + (k & 3)] = w;
  if (l) {                                   // W^T: the output index is k, the k axis runs over o
    const GsPolicyLayerF32 T = A.N.T[l];
    const_cast<float*>(T.w)[(((size_t)(k >> 4) * T.kb + (o >> 4)) * 64 + ((o & 15) >> 2) * 16 + (k & 15)) * 4 + (o & 3)] = w;
  }
}
