// The look-at views of make_TCO_multiview (TB/lib3d/multiview.py:28-92, 166-251; closed form derived in SURVEY.md A.9), shared by
// geometry.hip (the "TCO+front_{1,3,5}views" of the refinement loop) and train_hyp.hip (the "sphere_26views" candidates of the
// coarse classifier's training step): the look-at in double, and the fp32 tail invert_transform_matrices(TC0_CV) @ TCO.
//
// Unlike philox.h / rigid.h this header holds contractible floating-point expressions.  Every function therefore opens with its
// own `#pragma clang fp contract(off)`: each product and sum rounds once, in the order written, whatever the including file's
// pragma state is at the point of inclusion.  geometry.hip's results are pinned bit for bit to this arithmetic: change it nowhere.
#pragma once

#include "common.h"

namespace hp {

// Below this length of (forward x up hint), both unit vectors, the hint does not define a right vector: see look_at_cv.
constexpr double kLookAtDegenerate = 1e-9;

// look-at pose (camera -> cam0, OpenCV axes) in double, as the reference's numpy/Panda path: forward f = (tgt - pos) / |tgt - pos|
// exactly, right = f x up / |f x up| with camera 0's up (0, -1, 0) as the hint, up' = right x f; columns right, -up', f.
// fallback_right == nullptr (geometry.hip): no test, a forward along the hint gives a NaN pose as it always did.
// fallback_right != nullptr: where |f x up| < kLookAtDegenerate, right = fallback_right (a unit vector orthogonal to f is the
// caller's business; train_hyp.hip passes the right axis of the re-aimed camera 0).
__device__ __forceinline__ void look_at_cv(const double* pos, const double* tgt, double* M /*[12]*/, const double* fallback_right = nullptr) {
#pragma clang fp contract(off)
  double f[3] = {tgt[0] - pos[0], tgt[1] - pos[1], tgt[2] - pos[2]};
  double nf = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  f[0] /= nf; f[1] /= nf; f[2] /= nf;
  const double up[3] = {0.0, -1.0, 0.0};
  double r[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
  double nr = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  if (fallback_right && nr < kLookAtDegenerate) {
    r[0] = fallback_right[0]; r[1] = fallback_right[1]; r[2] = fallback_right[2];
  } else {
    r[0] /= nr; r[1] /= nr; r[2] /= nr;
  }
  double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
  // columns: right, -up', forward ; translation pos
  M[0] = r[0]; M[1] = -u[0]; M[2] = f[0]; M[3] = pos[0];
  M[4] = r[1]; M[5] = -u[1]; M[6] = f[1]; M[7] = pos[1];
  M[8] = r[2]; M[9] = -u[2]; M[10] = f[2]; M[11] = pos[2];
}

// TC0_CV of the view at `off` (units of |tcr|, in the Panda frame of camera 0 re-aimed at tcr: x = right (cv x), y = forward
// (cv z), z = up (-cv y)) looking at tcr.  `degenerate_rule`: the fallback of look_at_cv with the re-aimed camera's right axis.
// |tcr| == 0 (what a non-finite pose is turned into by the callers): the identity view.
__device__ __forceinline__ void look_at_view(const double* tcr, int ox, int oy, int oz, bool degenerate_rule, double* M /*[12]*/) {
#pragma clang fp contract(off)
  double radius = sqrt(tcr[0] * tcr[0] + tcr[1] * tcr[1] + tcr[2] * tcr[2]);
  M[0] = 1; M[1] = 0; M[2] = 0; M[3] = 0; M[4] = 0; M[5] = 1; M[6] = 0; M[7] = 0; M[8] = 0; M[9] = 0; M[10] = 1; M[11] = 0;
  if (radius > 0.0) {
    double zero[3] = {0, 0, 0};
    double base[12];
    look_at_cv(zero, tcr, base);
    double pos[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[c] = radius * (ox * base[4 * c + 0] + oy * base[4 * c + 2] - oz * base[4 * c + 1]);
    if (degenerate_rule) {
      const double right[3] = {base[0], base[4], base[8]};
      look_at_cv(pos, tcr, M, right);
    } else {
      look_at_cv(pos, tcr, M);
    }
  }
}

// TCV_O = invert_transform_matrices(TC0_CV) @ TCO (TB/lib3d/transform_ops.py:59-67) in fp32 from the double look-at pose M rounded
// to fp32; the bottom row of T is copied.
__device__ __forceinline__ void view_from_cam0(const double* M /*[12]*/, const float* T /*[16]*/, float* TV /*[16]*/) {
#pragma clang fp contract(off)
  float Mf[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) Mf[k] = (float)M[k];
  float Ri[9] = {Mf[0], Mf[4], Mf[8], Mf[1], Mf[5], Mf[9], Mf[2], Mf[6], Mf[10]};
  float ti[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) ti[r] = -(Ri[3 * r] * Mf[3] + Ri[3 * r + 1] * Mf[7] + Ri[3 * r + 2] * Mf[11]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float acc = Ri[3 * r] * T[c] + Ri[3 * r + 1] * T[4 + c] + Ri[3 * r + 2] * T[8 + c];
      TV[4 * r + c] = acc + ti[r] * T[12 + c];
    }
  }
  TV[12] = T[12]; TV[13] = T[13]; TV[14] = T[14]; TV[15] = T[15];
}

}  // namespace hp
