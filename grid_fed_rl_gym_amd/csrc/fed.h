// fed.h -- the federation of gs_fed_* (include/gridstep.h "the federation"): shapes and argument blocks of the
// kernels of kernels_fed.hip, shared with abi_fed.hip.
//
// Parameters are flat float32 in torch order, as the learner's (train.h).  The images a round rewrites are the learner's: the forward
// image of layer l ([nt][kb][64 lanes][4], policy.h) and, for l >= 1, the image of W_l^T.  gs_k_fed_apply finds a parameter's slots
// with policy.h's gs_pol32_slot; gs_k_train_adam (kernels_train.hip) is the other writer of these images.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gridstep.h"
#include "policy.h"

// the reductions: 1024 parameters a workgroup (four per thread), then one workgroup of 1024 threads over the workgroups' sums
constexpr int GS_FED_RED_THREADS = 256, GS_FED_RED_PER_THREAD = 4, GS_FED_BLOCK = GS_FED_RED_THREADS * GS_FED_RED_PER_THREAD;
constexpr int GS_FED_SUM_THREADS = 1024;
constexpr int GS_FED_APPLY_THREADS = 256;
constexpr int GS_FED_MAX_PAIRS = GS_FED_MAX_CLIENTS * (GS_FED_MAX_CLIENTS + 1) / 2;

// what a round reads and writes of one client, rebuilt from the handle's learner on every call
struct GsFedClient {
  float* params; float* m; float* v;
  float* w[GS_POLICY_MAX_LAYERS];      // the forward image's weights ...
  float* b[GS_POLICY_MAX_LAYERS];      // ... and biases
  float* t[GS_POLICY_MAX_LAYERS];      // l >= 1: the transposed image's weights
  void* reserved;
};
static_assert(sizeof(GsFedClient) == 128, "GsFedClient: sixteen pointers");

// the shape every client shares
struct GsFedShape {
  int32_t n_layers, P;
  int32_t dims[GS_POLICY_MAX_LAYERS + 1];
  int32_t p_off[GS_POLICY_MAX_LAYERS];
  int32_t kb[GS_POLICY_MAX_LAYERS];       // k blocks of the forward image
  int32_t kbt[GS_POLICY_MAX_LAYERS];      // k blocks of the transposed image
  int32_t reserved;
};

// gs_k_fed_gram, grid (blocks, entries): entry e is the pair (pi[e], pk[e]) of POSITIONS in `part`
struct GsFedGramArgs {
  const GsFedClient* clients; const float* g;
  double* blocksum;                       // [entries][blocks]
  int32_t P, blocks;
  uint8_t part[GS_FED_MAX_CLIENTS];       // the participants
  const uint8_t* pairs;                   // [entries][2] positions; NULL: entry e is (e, e)
};

// gs_k_fed_sum, grid (entries): out[e] = the sum of blocksum[e][0 .. blocks); with `coef` also the round's coefficients of entry e
struct GsFedSumArgs {
  const double* blocksum; double* out;
  int32_t blocks, coef;
  double clip_norm;
  double u[GS_FED_MAX_CLIENTS];           // server_lr w_k / W
  double* stats;                          // [3][GS_FED_MAX_CLIENTS]: norm, c, a
};

// gs_k_fed_apply, one thread per parameter.  n = 0: the broadcast of g as it is
struct GsFedApplyArgs {
  GsFedShape S;
  const GsFedClient* clients; float* g;
  const double* stats;                    // a_k at stats[2 * GS_FED_MAX_CLIENTS + k]
  int32_t n_clients, n;
  uint8_t part[GS_FED_MAX_CLIENTS];
  double noise_std;
  uint64_t seed;
  uint32_t round; int32_t net;
  int32_t reset_moments, reserved;
};

extern "C" {
__global__ void gs_k_fed_gram(GsFedGramArgs A);
__global__ void gs_k_fed_sum(GsFedSumArgs A);
__global__ void gs_k_fed_apply(GsFedApplyArgs A);
}
