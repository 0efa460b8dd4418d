// Rigid transforms in float32 as the upper 3 x 4 of a row-major 4 x 4 (bottom row 0 0 0 1), shared by the evaluation kernels
// (pose_errors.hip, multiview.hip).  Every product is an explicit fmaf chain in the order written below, and results that are
// compared bit for bit depend on that nesting: change it nowhere.  The training kernels (pose_losses, batch_data, train_hyp) and
// geometry.hip do NOT use this type: their double-precision, order-pinned arithmetic is different on purpose.
//
// Explicit fmaf calls and copies only.  Shared headers are compiled OUTSIDE the `#pragma clang fp contract(off)` of the files that
// include them, so nothing with a contractible floating-point expression (a bare a * b + c) may be added here.
#pragma once

#include "common.h"

namespace hp {

struct T34 {
  float m[12];
};

__device__ inline T34 load_T(const float* __restrict__ p) {
  T34 t;
#pragma unroll
  for (int i = 0; i < 12; ++i) t.m[i] = p[i];
  return t;
}

__device__ inline void store_T(float* __restrict__ out, const T34& t) {
#pragma unroll
  for (int i = 0; i < 12; ++i) out[i] = t.m[i];
  out[12] = 0.f;
  out[13] = 0.f;
  out[14] = 0.f;
  out[15] = 1.f;
}

__device__ inline T34 mul(const T34& a, const T34& b) {
  T34 c;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float s = j == 3 ? a.m[4 * i + 3] : 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) s = fmaf(a.m[4 * i + k], b.m[4 * k + j], s);
      c.m[4 * i + j] = s;
    }
  }
  return c;
}

// invert_transform_matrices (TB/lib3d/transform_ops.py:59-67): R^T, -R^T t
__device__ inline T34 inverse(const T34& a) {
  T34 c;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c.m[4 * i + k] = a.m[4 * k + i];
      s = fmaf(-a.m[4 * k + i], a.m[4 * k + 3], s);
    }
    c.m[4 * i + 3] = s;
  }
  return c;
}

__device__ inline void apply(const T34& t, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = fmaf(t.m[0], x, fmaf(t.m[1], y, fmaf(t.m[2], z, t.m[3])));
  oy = fmaf(t.m[4], x, fmaf(t.m[5], y, fmaf(t.m[6], z, t.m[7])));
  oz = fmaf(t.m[8], x, fmaf(t.m[9], y, fmaf(t.m[10], z, t.m[11])));
}

// P = K @ T[:3] (CP/lib3d/camera_geometry.py:15)
__device__ inline T34 camera_matrix(const float* __restrict__ K, const T34& t) {
  T34 c;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) s = fmaf(K[3 * i + k], t.m[4 * k + j], s);
      c.m[4 * i + j] = s;
    }
  }
  return c;
}

}  // namespace hp
