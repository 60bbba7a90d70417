// train.h -- the learner of gs_learner_* (include/gridstep.h "the learner"): tile shapes and argument blocks of
// the kernels of kernels_train.hip, shared with abi_learner.hip, which fills every block and queues every launch in one place each
// (its queue_* helpers; the reduction's workgroup count is gs_tr_red_blocks below).
//
// A network of L layers with widths dims[0 .. L] has P = sum_l dims[l + 1] (dims[l] + 1) parameters, flat in torch order: W_0
// row-major [out][in], b_0, W_1, b_1, ...  Gradients, Adam's m and v, and every partial gradient share that order.
// Per-sample scratch: `acts` and `deltas` hold, for layer l, an [n][16 nt_l] float32 matrix at column offset col_off[l] of a row
// of `row_stride` floats (nt_l = the layer's column tiles): acts = the hidden post-activations and, for the last layer, the
// pre-head values; deltas = dL / d(pre-activation of layer l), the head gradient for the last layer.  Columns beyond a layer's
// width hold zeros in both (zero weights and biases give act(0) = 0; the transposed image's padding gives delta 0).
#pragma once
#include <stdint.h>

#include "policy.h"

// rows of a workgroup of the forward and the backward-data kernel (two 16-row tiles, the policy kernel's shape: at a minibatch of
// 4096 that is 128 workgroups; the value kernel's 64 rows would leave three quarters of the compute units idle)
constexpr int GS_TR_ROWS = 32;
// rows of one partial weight gradient: a compile-time constant, so that the gradient's bits depend on n alone
constexpr int GS_TR_SEG = 256;
constexpr int gs_tr_segments(int n) { return (n + GS_TR_SEG - 1) / GS_TR_SEG; }
// a wavefront of the weight-gradient kernel owns GS_TR_WT_OUT x GS_TR_WT 16 x 16 tiles of dW (32 outputs x 64 inputs), each summed
// in GS_TR_CHAINS accumulator sets that take the k-steps in turn
constexpr int GS_TR_WT_OUT = 2, GS_TR_WT = 4, GS_TR_CHAINS = 4;
constexpr int GS_TR_RED_THREADS = 256, GS_TR_RED_PER_THREAD = 4;      // the segment reduction: 1024 parameters per workgroup
// ... so P parameters take this many workgroups: the launch of gs_k_train_reduce, the length of its `blocksum`, what the statistics add up
constexpr int gs_tr_red_blocks(int P) { return (P + GS_TR_RED_THREADS * GS_TR_RED_PER_THREAD - 1) / (GS_TR_RED_THREADS * GS_TR_RED_PER_THREAD); }
constexpr int GS_TR_STAT_THREADS = 1024;
// LDS of the forward kernel: the activation tile and the observation tile, staged in the value kernel's panels (policy.h)
inline int gs_tr_lds_bytes(int kb0) { return GS_TR_ROWS * (gs_val_obs_stride(kb0) + GS_POL32_ACT_STRIDE) * 4; }
constexpr int GS_TR_LDS_MAX = GS_TR_ROWS * (16 * GS_VAL_PANEL_KB + 4 + GS_POL32_ACT_STRIDE) * 4;

enum { GS_TR_STAT_LOSS = 0, GS_TR_STAT_SURR, GS_TR_STAT_ENT, GS_TR_STAT_KL, GS_TR_STAT_CLIPFRAC, GS_TR_STAT_VLOSS, GS_TR_STAT_GNORM, GS_TR_STAT_COUNT };

struct GsTrainNet {
  int32_t n_layers, activation, row_stride, P;
  int32_t dims[GS_POLICY_MAX_LAYERS + 1];
  int32_t col_off[GS_POLICY_MAX_LAYERS];      // of layer l's block in a row of acts / deltas
  int32_t p_off[GS_POLICY_MAX_LAYERS];        // of W_l in the flat parameter order (b_l follows W_l)
  int32_t reserved;
  GsPolicyLayerF32 L[GS_POLICY_MAX_LAYERS];   // the forward image (what the rollout and critic kernels read)
  GsPolicyLayerF32 T[GS_POLICY_MAX_LAYERS];   // l >= 1: the packed image of W_l^T (kb = nt of L[l], nt = kb of L[l]); b unused
};

struct GsTrainFwdArgs {
  GsTrainNet N;
  const float* obs;      // [n][D], already normalised
  float* acts;           // [n][row_stride]
  int32_t n, D, obs_stride, panel_kb;
};

struct GsTrainHeadArgs {
  const float* pre;      // acts + col_off[last]: [n] rows of row_stride floats
  float* ghead;          // deltas + col_off[last]
  int32_t n, row_stride, width16, A;      // width16: 16 nt of the last layer; A: action_dim, 0 for a critic
  // the policy
  const int32_t* idx;    // [n] transition of every sample
  const double* act;     // [N][A] the rollout's actions
  const double* logp;    // [N] the rollout's log-probabilities
  const float* adv;      // [n]
  long long N;
  double clip, ent_coef;
  // a critic
  const float* ret;      // [n]
  // per sample
  double* lp_new; double* ratio; int32_t* clipped;      // policy only
  double* term0;         // policy: min(r A, clip(r) A); critic: (v - ret)^2
  double* term1;         // policy: sum_k (ls_k + 0.5 log(2 pi e))
};

struct GsTrainBwdArgs {
  GsTrainNet N;
  const float* acts; float* deltas;
  int32_t n, reserved;
};

struct GsTrainGradArgs {
  GsTrainNet N;
  const float* obs; const float* acts; const float* deltas;
  float* partial;        // [segments][P]
  int32_t n, D;
  int32_t blk0[GS_POLICY_MAX_LAYERS + 1];     // the first workgroup of layer l along blockIdx.x
  int32_t in_blocks[GS_POLICY_MAX_LAYERS];    // 64-input blocks of layer l (its workgroups: 32-output blocks x in blocks)
};

struct GsTrainReduceArgs {
  const float* partial; float* grad; double* blocksum;
  int32_t P, segments;
};

struct GsTrainStatArgs {
  const double* term0; const double* term1; const double* lp_new; const double* logp; const int32_t* idx; const int32_t* clipped;
  const double* blocksum; double* stats;
  long long N;
  int32_t n, blocks, policy, reserved;
  double ent_coef;
};

// ---- the heads of kernels_train_offline.hip (include/gridstep.h "the learner's loss") ----
// gs_k_train_head_awr: GsTrainHeadArgs' policy part without the rollout's log-probabilities and the clip
struct GsTrainAwrHeadArgs {
  const float* pre; float* ghead;        // as GsTrainHeadArgs
  int32_t n, row_stride, width16, A;
  const int32_t* idx; const double* act; const float* adv;
  long long N;
  double temperature, weight_max, ent_coef;
  double* lp_new; double* weight; int32_t* capped;
  double* term0;         // w_i lp
  double* term1;         // sum_k (ls_k + 0.5 log(2 pi e))
};

// gs_k_train_head_expectile: a critic's head, term0 = q_i (v - ret)^2
struct GsTrainExpectileArgs {
  const float* pre; float* ghead; const float* ret; double* term0;
  int32_t n, row_stride, width16, reserved;
  double tau;
};

// gs_k_train_stats_awr: GsTrainStatArgs for a policy whose rollout may hold no log-probabilities (logp NULL: approx_kl NaN)
struct GsTrainAwrStatArgs {
  const double* term0; const double* term1; const double* lp_new; const double* logp; const int32_t* idx; const int32_t* capped;
  const double* blocksum; double* stats;
  long long N;
  int32_t n, blocks;
  double ent_coef;
};

struct GsTrainAdamArgs {
  GsTrainNet N;
  float* params; const float* grad; float* m; float* v;
  const double* stats;   // GS_TR_STAT_GNORM is read for the clip
  double max_grad_norm;  // 0: off
  float wd, b1, omb1, b2, omb2, bc2s, eps, step;      // the host's float64 scalars rounded once
};
