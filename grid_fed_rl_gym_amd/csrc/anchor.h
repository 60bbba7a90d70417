// anchor.h -- parameter anchors of gs_learner_anchor_* / gs_learner_fisher_* (include/gridstep.h "parameter anchors"; DESIGN.md
// section 31): argument blocks of the kernels of kernels_anchor.hip, shared with abi_anchor.hip, which fills every block and queues
// every launch.  All arrays are flat over the learner's P parameters in torch order (train.h).
#pragma once
#include <stdint.h>

#include "train.h"

// gs_k_train_anchor: the grid and per-thread order of gs_k_train_reduce (gs_tr_red_blocks(P) workgroups of GS_TR_RED_THREADS
// threads, GS_TR_RED_PER_THREAD parameters a thread).  A term whose coefficient is 0 is not evaluated and its arrays may be NULL;
// its per-workgroup sum is written as 0.
struct GsAnchorArgs {
  float* grad;             // [P] in: the reduced gradient of the loss; out: with the terms
  const float* params;     // [P] the master parameters w
  const float* prox;       // [P] a
  const float* importance; // [P] A
  const float* centre;     // [P] c
  double* blocksum;        // [blocks] OVERWRITTEN: the sums of the new g^2 (what the statistics kernels add up)
  double* sum_loss;        // [blocks] sum g_loss^2
  double* sum_prox;        // [blocks] sum (w - a)^2
  double* sum_ewc;         // [blocks] sum A (w - c)^2
  int32_t P, reserved;
  float mu, lambda;        // the host's doubles rounded once
};

// gs_k_train_grad_sq takes gs_k_train_grad's GsTrainGradArgs (train.h) and is launched on its grid.

// gs_k_fisher_accumulate: one thread per parameter
struct GsFisherAccArgs {
  const float* partial;    // [segments][P]
  double* pending;         // [P]
  int32_t P, segments;
};

// gs_k_fisher_commit: one thread per parameter
struct GsFisherCommitArgs {
  const double* pending;   // [P]
  const float* params;     // [P] w
  float* importance;       // [P] A
  float* centre;           // [P] c
  double samples, decay;
  float min_importance;
  int32_t first;           // the slot is empty: A = F, c = w
  int32_t P, reserved;
};
