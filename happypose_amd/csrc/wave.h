// Wavefront reductions (gfx950: 64 lanes): xor butterflies over offsets 32, 16, ... 1.  Both partners of every exchange apply the
// same commutative operation to the same two values, so EVERY lane ends with the same bits, and the order of the floating-point
// additions is fixed: sums that must repeat bit for bit (the losses, the pose errors) rely on exactly this tree.
//   wave_sum   int, float, double and the other integer types __shfl_xor takes
//   wave_min / wave_max   int (min / max), float (fminf / fmaxf), double (fmin / fmax)
// Block-level reductions stay with their kernels (their LDS layouts and wavefront counts differ) and call these.  So do the
// (value, index) arg-min / arg-max butterflies of multiview.hip, teaser.hip and det_eval.hip: they differ in direction, value type
// and payload, and one signature would not serve them.  head_train.hip keeps a reduction of its own in the OTHER order (offsets
// 1 .. 32): the trained weights depend on that rounding order.  icp.hip keeps its butterfly written out (the same order as
// wave_sum): through the helper the compiler allocates icp_accumulate_kernel's 29 accumulators differently.
//
// Single additions, min and max only.  Shared headers are compiled OUTSIDE the `#pragma clang fp contract(off)` of the files that
// include them, so nothing with a contractible floating-point expression (a bare a * b + c) may be added here.
#pragma once

#include "common.h"

namespace hp {

constexpr int kWave = 64;

namespace wave_detail {
__device__ __forceinline__ int min2(int a, int b) { return min(a, b); }
__device__ __forceinline__ int max2(int a, int b) { return max(a, b); }
__device__ __forceinline__ float min2(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float max2(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double min2(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ double max2(double a, double b) { return fmax(a, b); }
}  // namespace wave_detail

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

template <class T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = wave_detail::min2(v, __shfl_xor(v, off, kWave));
  return v;
}

template <class T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = wave_detail::max2(v, __shfl_xor(v, off, kWave));
  return v;
}

}  // namespace hp
