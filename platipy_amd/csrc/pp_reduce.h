// platipy_amd/csrc/pp_reduce.h -- the block-wide LDS reduction tree, written once, and the two reductions built on it
// that several features share: min / max of a range (float or double) and its single-block fold over block partials.
// (pp_block_sum3 of pp_internal.h, the demons kernels' sum, stays where it is.)
#pragma once

#include "pp_internal.h"

namespace {

// Slots t < NT of the caller's own LDS arrays hold one value per thread; merge(a, b) folds slot b into slot a.  Slot t + s
// is folded into slot t for s = NT / 2 ... 1, a fixed order, so sums are bit-identical from run to run.  Every thread of
// the block calls it, right after writing its slot (the first barrier is in here); the result is in slot 0, visible to all.
// `t` is the caller's linear thread index (a 2-D block passes threadIdx.y * blockDim.x + threadIdx.x).
template <int NT, typename Merge>
__device__ __forceinline__ void pp_block_tree(int t, Merge&& merge) {
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s) merge(t, t + s);
    __syncthreads();
  }
}

// min / max as the range reductions take them: fminf / fmaxf and fmin / fmax (a NaN operand loses), and the value an empty
// thread or block contributes.
template <typename T>
struct pp_range;
template <>
struct pp_range<float> {
  static __device__ __forceinline__ float lo0() { return FLT_MAX; }
  static __device__ __forceinline__ float hi0() { return -FLT_MAX; }
  static __device__ __forceinline__ float lower(float a, float b) { return fminf(a, b); }
  static __device__ __forceinline__ float upper(float a, float b) { return fmaxf(a, b); }
};
template <>
struct pp_range<double> {
  static __device__ __forceinline__ double lo0() { return INFINITY; }
  static __device__ __forceinline__ double hi0() { return -INFINITY; }
  static __device__ __forceinline__ double lower(double a, double b) { return fmin(a, b); }
  static __device__ __forceinline__ double upper(double a, double b) { return fmax(a, b); }
};

// The tail of a range kernel (1-D block of NT threads): the threads' (lo, hi) folded by the tree, pair[0] = min and
// pair[1] = max stored by thread 0.
template <int NT, typename T>
__device__ __forceinline__ void pp_block_range_store(T lo, T hi, T* __restrict__ pair) {
  __shared__ T smin[NT], smax[NT];
  const int t = threadIdx.x;
  smin[t] = lo;
  smax[t] = hi;
  pp_block_tree<NT>(t, [&](int a, int b) {
    smin[a] = pp_range<T>::lower(smin[a], smin[b]);
    smax[a] = pp_range<T>::upper(smax[a], smax[b]);
  });
  if (t == 0) {
    pair[0] = smin[0];
    pair[1] = smax[0];
  }
}

// One block: partials[2 b] = min and partials[2 b + 1] = max of block b < nb  ->  result[0] = min, result[1] = max.
// Thread t folds blocks t, t + NT, ... in that order, then the tree.
template <int NT, typename T>
__global__ void __launch_bounds__(NT) k_range_fold(const T* __restrict__ partials, int nb, T* __restrict__ result) {
  T lo = pp_range<T>::lo0(), hi = pp_range<T>::hi0();
  for (int b = threadIdx.x; b < nb; b += NT) {
    lo = pp_range<T>::lower(lo, partials[2 * b]);
    hi = pp_range<T>::upper(hi, partials[2 * b + 1]);
  }
  pp_block_range_store<NT>(lo, hi, result);
}

}  // namespace
