// conservative.h -- the conservative critic step of gs_learner_step_conservative (include/gridstep.h "the conservative critic step";
// DESIGN.md section 26): the argument blocks of the kernels of kernels_conservative.hip, shared with abi_learner.hip.  The layers of
// a step -- the policy's forward pass and the twin's passes over 3 n rows -- run on the kernels of kernels_train.hip (train.h), the
// data block and the targets are gs_k_q_gather's (q.h) and the policy block's actions gs_k_pw_sample's (pathwise.h), all unchanged.
#pragma once
#include <stdint.h>

constexpr uint32_t GS_CQL_UNIFORM_TAG = 0x43514C55u;      // 'CQLU'
constexpr uint32_t GS_CQL_NOISE_TAG = 0x43514C4Eu;        // 'CQLN': gs_k_pw_sample's noise under this step
// n minibatch rows make 3 n rows of a twin's passes, which take at most 2^24 like every learner's
constexpr int GS_CQL_MAX_N = (1 << 24) / 3;
// the logsumexp drops what lies this far below the maximum (exp(-700) is still a normal float64: no subnormal enters a sum)
constexpr double GS_CQL_EXP_FLOOR = -700.0;

// gs_k_cql_rows: one thread per element (i, c) of [n][D + A].  c < D: the observation obs[i][c] into the uniform and the policy
// block (rows n + i and 2 n + i; the data block is gs_k_q_gather's); c >= D: the uniform action of column k = c - D into
// random[i][k] (float64) and, rounded once, into row n + i.  The policy block's action columns are gs_k_pw_sample's.
struct GsCqlRowsArgs {
  const float* obs;           // [n][D] the minibatch's normalised observations
  float* sa;                  // [3 n][D + A] the twin's input rows
  double* random;             // [n][A]
  int32_t n, D, A;
  uint32_t draw;
  uint64_t seed;
};

// gs_k_cql_lse: ONE workgroup of GS_TR_STAT_THREADS over the twin's 3 n values
struct GsCqlLseArgs {
  const float* qpre;          // the twin's acts + col_off[last]: [3 n] rows of row_stride floats, column 0
  double* scalars;            // [4] m, S, lse, qbar
  int32_t n, row_stride;
};

// gs_k_cql_head: one thread per row j of [0, 3 n)
struct GsCqlHeadArgs {
  const float* qpre;          // as GsCqlLseArgs
  float* ghead;               // the twin's deltas + col_off[last]
  const float* y;             // [n] the regression targets
  const double* scalars;      // [4] of gs_k_cql_lse
  double* q;                  // [3 n] the values, widened
  double* weights;            // [3 n] p_j
  double* terms;              // [n] (q_i - y_i)^2
  int32_t n, row_stride, width16, reserved;
  double cw;
};

// gs_k_cql_stats: GsPwStatArgs' shape
struct GsCqlStatArgs {
  const double* terms; const double* scalars;
  const double* blocksum; double* stats;
  int32_t n, blocks;
  double cw;
};
