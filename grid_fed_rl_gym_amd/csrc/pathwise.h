// pathwise.h -- the pathwise actor step of gs_learner_step_pathwise (include/gridstep.h "the pathwise actor step"; DESIGN.md section
// 23): the argument blocks of the kernels of kernels_pathwise.hip, shared with abi_learner.hip.  The layers of a step -- the policy's
// and the twins' -- run on the kernels of kernels_train.hip (train.h), unchanged.
#pragma once
#include <stdint.h>

constexpr uint32_t GS_PW_NOISE_TAG = 0x50574E4Fu;      // 'PWNO'
// gs_k_pw_input_grad: GS_PW_JT rows of W0's action columns are staged in LDS at a time (A <= 128: at most 32 KB)
constexpr int GS_PW_JT = 64, GS_PW_MAX_A = 128, GS_PW_THREADS = 256;

// gs_k_pw_sample: one thread per sample, float64 on the policy's float32 pre-head values (mean_k | log_std_k)
struct GsPwSampleArgs {
  const float* pre;           // the policy's acts + col_off[last]: [n] rows of row_stride floats
  double* actions;            // [n][A] a_k = tanh(mean_k + std_k eps_k)
  double* noise;              // [n][A] eps_k
  double* logp;               // [n]
  float* sa;                  // [n][D + A] the twins' input rows: the action columns (float)a_k are written here
  int32_t n, row_stride, A, D, stochastic, reserved;
  uint32_t draw, tag;         // tag: the noise counter's fourth word; 0 means GS_PW_NOISE_TAG (the conservative critic step passes its own)
  uint64_t seed;
};

// gs_k_pw_rows: one thread per element, sa[i][c] = obs[i][c] for c < D
struct GsPwRowsArgs {
  const float* obs;           // [n][D] the minibatch's normalised observations
  float* sa;                  // [n][DA]
  int32_t n, D, DA, reserved;
};

// gs_k_pw_seed: one thread per sample, the head gradient of q: 1.0f in column 0 of the twin's last layer's delta, 0 up to width16
struct GsPwSeedArgs {
  float* ghead;               // the Q scratch's deltas + col_off[last]
  int32_t n, row_stride, width16, reserved;
};

// gs_k_pw_input_grad: one thread per (sample, action): dqda[i][k] = sum_j delta0[i][j] W0[j][D + k], j ascending from 0 in ONE float32
// chain (every product and every sum rounded); threads with k = 0 also widen the twin's value q[i] = acts[i][col_off[last]]
struct GsPwInputGradArgs {
  const float* delta0;        // the Q scratch's deltas + col_off[0]
  const float* qpre;          // the Q scratch's acts + col_off[last]
  const float* W0;            // the Q learner's master parameters + p_off[0]: [H0][D + A] row-major
  float* dqda;                // [n][A]
  double* q;                  // [n]
  int32_t n, row_stride, H0, D, A, reserved;
};

// gs_k_pw_head: one thread per sample
struct GsPwHeadArgs {
  const float* pre;           // as GsPwSampleArgs
  float* ghead;               // the policy's deltas + col_off[last]
  const double* actions; const double* noise; const double* logp;
  const double* q[2];         // [n] each; NULL: that twin is not installed
  const float* dqda[2];       // [n][A] each
  const int32_t* idx;         // [n] transition of every sample; read when bc_coef != 0 only
  const double* act;          // [N][A] the rollout's stored actions
  long long N;
  int32_t n, row_stride, width16, A;
  double alpha, bc_coef;
  int32_t* which; double* qmin; double* bc; double* terms;      // [n] each
};

// gs_k_pw_stats: GsTrainAwrStatArgs' shape
struct GsPwStatArgs {
  const double* terms; const double* qmin; const double* logp;
  const double* blocksum; double* stats;
  int32_t n, blocks;
};
