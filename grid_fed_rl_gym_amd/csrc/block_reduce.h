// block_reduce.h -- the one workgroup reduction of the learning kernels (kernels_train, kernels_train_offline, kernels_pathwise,
// kernels_fed, kernels_batches, kernels_episodes).  Kernels whose results are compared bit for bit sum through this function, so
// "the same order" is this order.
#pragma once
#include <hip/hip_runtime.h>

struct GsSum { template <typename X> __device__ X operator()(X a, X b) const { return a + b; } };
struct GsMin { __device__ double operator()(double a, double b) const { return fmin(a, b); } };
struct GsMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

// The reduction of one value per thread over the workgroup, in a fixed order: a butterfly over the wavefront's 64 lanes (partners
// at 32, 16, 8, 4, 2, 1 lanes), the W wavefronts' results through lds[W], a second butterfly over those (partners at W / 2, ..., 1):
// a balanced binary tree over the threads' values, of depth 10 for 1024 threads.  IEEE addition, fmin and fmax commute, so both
// partners of a butterfly step hold the same bits and every thread returns the same value.  Every thread of the workgroup calls it;
// consecutive calls may share `lds` (the first barrier).  WAVES: the number of wavefronts W, a power of two up to 64 -- 0 reads it
// from blockDim.x, which must then be 64 W.  Nothing is contracted.
template <int WAVES = 0, typename X, typename Op = GsSum>
__device__ __forceinline__ X gs_block_reduce(X v, X* lds, Op op = Op()) {
#pragma clang fp contract(off)
  static_assert(WAVES >= 0 && WAVES <= 64 && (WAVES & (WAVES - 1)) == 0, "the second butterfly runs over a power of two of lanes");
  const int W = WAVES ? WAVES : blockDim.x >> 6;
  for (int off = 32; off > 0; off >>= 1) v = op(v, (X)__shfl_xor(v, off));
  __syncthreads();                           // (the reduction before this one has been read)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  v = lds[threadIdx.x & (W - 1)];
  for (int off = W / 2; off > 0; off >>= 1) v = op(v, (X)__shfl_xor(v, off));
  return v;
}

template <int WAVES = 0, typename X>
__device__ __forceinline__ X gs_block_sum(X v, X* lds) { return gs_block_reduce<WAVES>(v, lds, GsSum()); }
