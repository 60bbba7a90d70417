// kernels_anchor.hip -- parameter anchors (anchor.h; include/gridstep.h "parameter anchors"):
//   gs_k_train_anchor        g += mu (w - a), g += lambda (A (w - c)) on the reduced gradient, in gs_k_train_reduce's grid and order; the
//                            squares of the new gradient per workgroup, and three more sums for gs_learner_anchor_stats
//   gs_k_train_grad_sq       gs_k_train_grad on squared operands: sum_i ((float)n delta_i)^2 (a_i)^2, the per-sample Fisher diagonal of
//                            a dense layer, one partial per segment
//   gs_k_fisher_accumulate   the partials in ascending segment order (float32), widened and added to the task's pending sum
//   gs_k_fisher_commit       F = max(pending / samples, min_importance) merged into the consolidated importance and centre
// No floating-point atomics: every sum has an order fixed by the network's shape and n.
#include <hip/hip_runtime.h>
#include <math.h>

#include "anchor.h"
#include "block_reduce.h"
#include "mlp_f32.h"
#include "train.h"

// ---- the terms on the reduced gradient ---------------------------------------------------------------------------------------------------
// Every operation is one correctly rounded float32 operation, in the order include/gridstep.h states; nothing is contracted.
extern "C" __global__ void __launch_bounds__(GS_TR_RED_THREADS)
gs_k_train_anchor(GsAnchorArgs A) {
#pragma clang fp contract(off)
  __shared__ double lds[GS_TR_RED_THREADS / 64];
  const int base = blockIdx.x * (GS_TR_RED_THREADS * GS_TR_RED_PER_THREAD);
  const bool with_prox = A.mu != 0.0f, with_ewc = A.lambda != 0.0f;
  double ss = 0.0, sl = 0.0, sp = 0.0, se = 0.0;
  for (int k = 0; k < GS_TR_RED_PER_THREAD; ++k) {
    const int p = base + k * GS_TR_RED_THREADS + (int)threadIdx.x;
    if (p >= A.P) break;
    float g = A.grad[p];
    const float w = A.params[p];
    sl = sl + (double)g * (double)g;
    if (with_prox) {
      const float d = w - A.prox[p];
      g = g + A.mu * d;
      sp = sp + (double)d * (double)d;
    }
    if (with_ewc) {
      const float imp = A.importance[p];
      const float d = w - A.centre[p];
      g = g + A.lambda * (imp * d);
      se = se + (double)imp * ((double)d * (double)d);
    }
    A.grad[p] = g;
    ss = ss + (double)g * (double)g;
  }
  ss = gs_block_sum(ss, lds);
  sl = gs_block_sum(sl, lds);
  sp = gs_block_sum(sp, lds);
  se = gs_block_sum(se, lds);
  if (threadIdx.x == 0) {
    A.blocksum[blockIdx.x] = ss; A.sum_loss[blockIdx.x] = sl; A.sum_prox[blockIdx.x] = sp; A.sum_ewc[blockIdx.x] = se;
  }
}

// ---- the Fisher diagonal of the dense layers ---------------------------------------------------------------------------------------------
// gs_k_train_grad's geometry (kernels_train.hip): one wavefront per (layer, 32 outputs, 64 inputs, segment), the rows of the segment the
// k axis, four a k-step, consecutive k-steps to GS_TR_CHAINS accumulator sets in turn, joined as (c0 + c1) + (c2 + c3); the bias's
// lanes joined as (q0 + q1) + (q2 + q3).  The operands are squared in registers after the load: A = ((float)n delta)^2, B = a^2.
extern "C" __global__ void __launch_bounds__(64)
gs_k_train_grad_sq(GsTrainGradArgs P) {
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
  const float nf = (float)P.n;
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
      for (int a = 0; a < WO; ++a) {
        const float d = ok && ook[a] ? dA[row * rs + ocol[a]] : 0.0f;
        const float t = nf * d;
        av[a] = t * t;
      }
#pragma unroll
      for (int b = 0; b < WI; ++b) {
        const float x = ok && iok[b] ? aB[row * ldb + icol[b]] : 0.0f;
        bv[b] = x * x;
      }
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

// ---- the partials into the task's pending sum --------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
gs_k_fisher_accumulate(GsFisherAccArgs A) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= A.P) return;
  float f = A.partial[p];
  for (int s = 1; s < A.segments; ++s) f = f + A.partial[(size_t)s * A.P + p];
  A.pending[p] = A.pending[p] + (double)f;
}

// ---- the end of a task: the merge into the consolidated importance and centre ------------------------------------------------------------
// float64 on the float32 values, every operation rounded, nothing contracted; each result rounded once to float32
extern "C" __global__ void __launch_bounds__(256)
gs_k_fisher_commit(GsFisherCommitArgs C) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= C.P) return;
  const float f32 = (float)(C.pending[p] / C.samples);
  const double F = (double)fmaxf(f32, C.min_importance);
  const double w = (double)C.params[p];
  if (C.first) {
    C.importance[p] = (float)F; C.centre[p] = (float)w;
    return;
  }
  const double dA = C.decay * (double)C.importance[p];
  const double An = dA + F;
  const double cn = An != 0.0 ? (dA * (double)C.centre[p] + F * w) / An : w;
  C.importance[p] = (float)An; C.centre[p] = (float)cn;
}
