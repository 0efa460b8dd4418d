// The losses the pose networks are trained and validated on (loss_CO_symmetric, compute_ADD_L1_loss, the two disentangled
// refiner losses and the rendered-views-logits loss), value and gradient: entry points, definitions and the reference lines they
// replace are in include/happypose_amd.h.
//
// Three kernels, each instantiated for one term (the symmetric loss) and for three (orientation, xy, z of a refiner loss):
//   terms_kernel     a workgroup is one (row, chunk of HP_POSE_LOSS_SYM_CHUNK symmetries).  Thread 0 builds the row's predicted poses
//                    (in double, from the float32 inputs) and hands them to the others through LDS; the chunk's T_gt,s lie in LDS too
//                    and are read by same-address (broadcast) 16-byte reads.  Lanes walk the row's points: every point is read
//                    once and transformed once per predicted pose, T_gt,s p_j is formed once per (s, j) and compared with all of
//                    them.  Per (s, term) the mean |difference| goes to the workspace [B][S][terms]: nothing of size B x S x N exists.
//   finish_kernel    one thread per row: first strict minimum over s per term (the lowest index on an exact tie), the sum of the
//                    terms, the chosen ids, and the gathered TCO_assign.
//   backward_kernel  a workgroup is one row: for the chosen symmetry of each term the twelve sums of sign(d) (p | 1), then
//                    thread 0 applies the analytic chain (Gram-Schmidt of the 6-D rotation, the image-space translation) and the
//                    row's upstream gradient.
// bce_logits_kernel (the coarse classifier's rendered-views-logits loss, value and gradient) is elementwise and described at its
// definition.
// The points are transformed in float32 (the arithmetic whose rounding the tests' sign-flip allowance describes); every SUM is
// accumulated in double, per lane in point order, then over the wavefront by xor butterflies, then over the four wavefronts in
// LDS in wavefront order.  No atomics: a row's outputs are a function of the row alone and the same bits in every run.
#include "common.h"
#include "wave.h"

namespace hp {
namespace {

#pragma clang fp contract(off)  // the prologue is compiled into two kernels: both must give the predicted poses the same bits

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kSymChunk = HP_POSE_LOSS_SYM_CHUNK;
constexpr int kSums = 12;  // sums of the backward pass, for one term and for three (see backward_kernel)

struct LossArgs {
  const float* gt;      // [B][S][16], entry 0 of a row is the ground truth
  const float* pred;    // [B][16]: the symmetric loss; nullptr in the refiner losses
  const float* T_in;    // [B][16]
  const float* out9;    // [B][9]
  const float* K;       // [B][9]
  const float* tCR;     // [B][3] or nullptr (CosyPose's form)
  const float* points;  // [B][N][3]
  int S, N;
};

// what the gradient needs of the prologue beyond the poses
struct Chain {
  double Rin[9];
  double x[3], z[3], yr[3], nx, nz;  // compute_rotation_matrix_from_ortho6d: x = xr / nx, z = (x cross yr) / nz, y = z cross x
  double dxy[2], dz;                 // d t_x / d out[6], d t_y / d out[7], d t_z / d out[8]
};

__device__ inline void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The three predicted poses of a refiner loss, upper 3 x 4 each (P[0] orientation, P[1] xy, P[2] z).
// tCR != nullptr: loss_refiner_CO_disentangled_reference_point (TB/lib3d/cosypose_ops.py:82-156) over
// pose_update_with_reference_point (:34-62); its vxvy_gt reaches none of the three (the orientation term keeps the update's
// rotation only, the z term its t_z = dR_gt (t_in - tCR) + vz tCR_z only), so it is not formed.
// tCR == nullptr: loss_refiner_CO_disentangled (CP/lib3d/cosypose_ops.py:62-101).
__device__ inline void refiner_poses(const LossArgs& a, int64_t b, float P[3][12], Chain& c) {
  const float* G = a.gt + 16 * b * a.S;
  const float* Ti = a.T_in + 16 * b;
  const float* o = a.out9 + 9 * b;
  const float* K = a.K + 9 * b;
  double Rg[9], tg[3], ti[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Rg[3 * r + k] = G[4 * r + k];
      c.Rin[3 * r + k] = Ti[4 * r + k];
    }
    tg[r] = G[4 * r + 3];
    ti[r] = Ti[4 * r + 3];
  }
  // TB/lib3d/rotations.py:22-36, no epsilon: a degenerate 6-D part makes the row NaN
  const double xr[3] = {o[0], o[1], o[2]};
  c.yr[0] = o[3], c.yr[1] = o[4], c.yr[2] = o[5];
  c.nx = sqrt(dot3(xr, xr));
#pragma unroll
  for (int k = 0; k < 3; ++k) c.x[k] = xr[k] / c.nx;
  double zu[3], y[3];
  cross3(c.x, c.yr, zu);
  c.nz = sqrt(dot3(zu, zu));
#pragma unroll
  for (int k = 0; k < 3; ++k) c.z[k] = zu[k] / c.nz;
  cross3(c.z, c.x, y);
  const double dR[9] = {c.x[0], y[0], c.z[0], c.x[1], y[1], c.z[1], c.x[2], y[2], c.z[2]};
  const double fxy[2] = {K[0], K[4]};
  double txy[2], tz;
  if (a.tCR) {
    const double tr[3] = {a.tCR[3 * b], a.tCR[3 * b + 1], a.tCR[3 * b + 2]};
    const double e[3] = {ti[0] - tr[0], ti[1] - tr[1], ti[2] - tr[2]};
    double q[3];  // dR_gt (t_in - tCR), dR_gt = R_gt R_in^T
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      q[r] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double d = Rg[3 * r] * c.Rin[3 * k] + Rg[3 * r + 1] * c.Rin[3 * k + 1] + Rg[3 * r + 2] * c.Rin[3 * k + 2];
        q[r] += d * e[k];
      }
    }
    const double vz_gt = (tg[2] - q[2]) / tr[2];
    const double ztgt = vz_gt * tr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      txy[i] = q[i] + (o[6 + i] / fxy[i] + tr[i] / tr[2]) * ztgt;
      c.dxy[i] = ztgt / fxy[i];
    }
    tz = q[2] + o[8] * tr[2];
    c.dz = tr[2];
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      txy[i] = (o[6 + i] / fxy[i] + ti[i] / ti[2]) * tg[2];
      c.dxy[i] = tg[2] / fxy[i];
    }
    tz = o[8] * ti[2];
    c.dz = ti[2];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      P[0][4 * r + k] = (float)(dR[3 * r] * c.Rin[k] + dR[3 * r + 1] * c.Rin[3 + k] + dR[3 * r + 2] * c.Rin[6 + k]);
      P[1][4 * r + k] = P[2][4 * r + k] = (float)Rg[3 * r + k];
    }
    P[0][4 * r + 3] = (float)tg[r];
    P[1][4 * r + 3] = (float)(r < 2 ? txy[r] : tg[2]);
    P[2][4 * r + 3] = (float)(r < 2 ? tg[r] : tz);
  }
}

template <int NT>
__device__ inline void predicted_poses(const LossArgs& a, int64_t b, float P[NT][12], Chain& c) {
  if constexpr (NT == 1) {
#pragma unroll
    for (int k = 0; k < 12; ++k) P[0][k] = a.pred[16 * b + k];
  } else {
    refiner_poses(a, b, P, c);
  }
}

__device__ inline void apply(const float* t, float x, float y, float z, float* o) {
  o[0] = fmaf(t[0], x, fmaf(t[1], y, fmaf(t[2], z, t[3])));
  o[1] = fmaf(t[4], x, fmaf(t[5], y, fmaf(t[6], z, t[7])));
  o[2] = fmaf(t[8], x, fmaf(t[9], y, fmaf(t[10], z, t[11])));
}

template <int NT>
__global__ void __launch_bounds__(kThreads) terms_kernel(LossArgs a, float* __restrict__ term_loss) {
  __shared__ float s_pred[NT][12];
  __shared__ float4 s_gt[kSymChunk][3];
  __shared__ double s_red[kWaves][kSymChunk * NT];
  const int64_t b = blockIdx.x;
  const int s0 = blockIdx.y * kSymChunk, tid = threadIdx.x;
  const int ns = min(kSymChunk, a.S - s0);  // >= 1: the grid holds ceil(S / chunk) chunks
  if (tid == 0) {  // one evaluation per workgroup: every lane compares against the same poses by construction
    float P[NT][12];
    Chain c;
    predicted_poses<NT>(a, b, P, c);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int k = 0; k < 12; ++k) s_pred[t][k] = P[t][k];
  }
  if (tid < 12 * ns) ((float*)s_gt)[tid] = a.gt[16 * (b * a.S + s0 + tid / 12) + tid % 12];
  __syncthreads();
  float P[NT][12];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int k = 0; k < 12; ++k) P[t][k] = s_pred[t][k];
  double acc[kSymChunk][NT];
#pragma unroll
  for (int s = 0; s < kSymChunk; ++s)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[s][t] = 0.0;
  const float* pts = a.points + 3 * b * a.N;
  for (int j = tid; j < a.N; j += kThreads) {
    const float x = pts[3 * (int64_t)j], y = pts[3 * (int64_t)j + 1], z = pts[3 * (int64_t)j + 2];
    float q[NT][3];
#pragma unroll
    for (int t = 0; t < NT; ++t) apply(P[t], x, y, z, q[t]);
#pragma unroll
    for (int s = 0; s < kSymChunk; ++s) {
      if (s < ns) {  // uniform over the workgroup
        const float4 r0 = s_gt[s][0], r1 = s_gt[s][1], r2 = s_gt[s][2];
        const float g[3] = {fmaf(r0.x, x, fmaf(r0.y, y, fmaf(r0.z, z, r0.w))), fmaf(r1.x, x, fmaf(r1.y, y, fmaf(r1.z, z, r1.w))),
                            fmaf(r2.x, x, fmaf(r2.y, y, fmaf(r2.z, z, r2.w)))};
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[s][t] += ((double)fabsf(q[t][0] - g[0]) + (double)fabsf(q[t][1] - g[1])) + (double)fabsf(q[t][2] - g[2]);
      }
    }
  }
  const int wave = tid / kWave;
#pragma unroll
  for (int s = 0; s < kSymChunk; ++s)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const double v = wave_sum(acc[s][t]);
      if (tid % kWave == 0) s_red[wave][s * NT + t] = v;
    }
  __syncthreads();
  if (tid < ns * NT) {
    double v = s_red[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += s_red[w][tid];  // wavefront order
    term_loss[(b * a.S + s0) * NT + tid] = (float)(v / (3.0 * (double)a.N));
  }
}

// A term loss that is not finite (a non-finite input anywhere in the row's points, poses or update; a degenerate 6-D part)
// makes the whole row NaN with ids -1, whichever term or symmetry it came from.
template <int NT>
__global__ void __launch_bounds__(kWave) finish_kernel(int B, int S, const float* __restrict__ term_loss, const float* __restrict__ gt,
                                                       float* __restrict__ loss, float* __restrict__ parts, int32_t* __restrict__ ids,
                                                       float* __restrict__ assign) {
  const int64_t b = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (b >= B) return;
  float best[NT];
  int id[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) best[t] = INFINITY, id[t] = -1;
  bool bad = false;
  for (int s = 0; s < S; ++s) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float v = term_loss[(b * S + s) * NT + t];
      bad |= !isfinite(v);
      if (v < best[t]) best[t] = v, id[t] = s;  // ascending s, strict <: the lowest index on an exact tie
    }
  }
  float total = best[0];
#pragma unroll
  for (int t = 1; t < NT; ++t) total += best[t];  // loss_orn + loss_xy + loss_z, left to right
  loss[b] = bad ? NAN : total;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (parts) parts[b * NT + t] = bad ? NAN : best[t];
    ids[b * NT + t] = bad ? -1 : id[t];
  }
  if (assign) {
    const float* src = gt + 16 * (b * S + (bad ? 0 : id[0]));
#pragma unroll
    for (int k = 0; k < 16; ++k) assign[16 * b + k] = bad ? NAN : src[k];
  }
}

__device__ inline float sign_of(float d) { return (float)((d > 0.f) - (d < 0.f)); }  // sign(0) = 0

// The sums, all over j and divided by 3N afterwards, with d = T_pred p_j - T_gt,s p_j for the term's own pose and chosen s:
//   one term     g[4a + c] = sum sign(d_a) (p_c | 1): the gradient with respect to the upper 3 x 4 of TCO_pred
//   three terms  g[3a + c] = sum sign(d_a) p_c of the orientation term (its translation is the ground truth's: no gradient),
//                g[9], g[10] = sum sign(d_x), sum sign(d_y) of the xy term, g[11] = sum sign(d_z) of the z term -- the only
//                entries of those two poses that depend on the outputs
template <int NT>
__global__ void __launch_bounds__(kThreads) backward_kernel(LossArgs a, const int32_t* __restrict__ ids, const float* __restrict__ grad_loss,
                                                            float* __restrict__ grad, float* __restrict__ grad_parts) {
  constexpr int kOut = NT == 1 ? 16 : 9;
  __shared__ float s_pred[NT][12];
  __shared__ float s_gt[NT][12];
  __shared__ Chain s_chain;
  __shared__ double s_red[kWaves][kSums];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  int id[NT];
  bool bad = false;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    id[t] = ids[b * NT + t];
    bad |= (unsigned)id[t] >= (unsigned)a.S;  // -1: the forward pass answered the row with NaN
  }
  if (bad) {  // uniform over the workgroup
    if (tid < kOut) grad[kOut * b + tid] = NAN;
    if (grad_parts && tid < 27) grad_parts[27 * b + tid] = NAN;
    return;
  }
  if (tid == 0) {
    float P[NT][12];
    predicted_poses<NT>(a, b, P, s_chain);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int k = 0; k < 12; ++k) s_pred[t][k] = P[t][k];
  }
  if (tid < 12 * NT) s_gt[tid / 12][tid % 12] = a.gt[16 * (b * a.S + id[tid / 12]) + tid % 12];
  __syncthreads();
  float P[NT][12], T[NT][12];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int k = 0; k < 12; ++k) P[t][k] = s_pred[t][k], T[t][k] = s_gt[t][k];
  double g[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) g[k] = 0.0;
  const float* pts = a.points + 3 * b * a.N;
  for (int j = tid; j < a.N; j += kThreads) {
    const float p[3] = {pts[3 * (int64_t)j], pts[3 * (int64_t)j + 1], pts[3 * (int64_t)j + 2]};
    float sg[NT][3];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float q[3], h[3];
      apply(P[t], p[0], p[1], p[2], q);  // the forward pass's arithmetic: the same differences, the same signs
      apply(T[t], p[0], p[1], p[2], h);
#pragma unroll
      for (int c = 0; c < 3; ++c) sg[t][c] = sign_of(q[c] - h[c]);
    }
    if constexpr (NT == 1) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) g[4 * r + c] += (double)sg[0][r] * (double)p[c];
        g[4 * r + 3] += (double)sg[0][r];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) g[3 * r + c] += (double)sg[0][r] * (double)p[c];
      g[9] += (double)sg[1][0];
      g[10] += (double)sg[1][1];
      g[11] += (double)sg[2][2];
    }
  }
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    const double v = wave_sum(g[k]);
    if (tid % kWave == 0) s_red[tid / kWave][k] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  const double n3 = 3.0 * (double)a.N, up = grad_loss[b];
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    double v = s_red[0][k];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += s_red[w][k];  // wavefront order
    g[k] = v / n3;
  }
  if constexpr (NT == 1) {
#pragma unroll
    for (int k = 0; k < 12; ++k) grad[16 * b + k] = (float)(up * g[k]);
#pragma unroll
    for (int k = 12; k < 16; ++k) grad[16 * b + k] = 0.f;
  } else {
    const Chain& c = s_chain;
    // R_pred = dR R_in with dR = [x y z] as columns: dL/dx, dL/dy, dL/dz are the columns of G R_in^T
    double gx[3], gy[3], gz[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      gx[r] = g[3 * r] * c.Rin[0] + g[3 * r + 1] * c.Rin[1] + g[3 * r + 2] * c.Rin[2];
      gy[r] = g[3 * r] * c.Rin[3] + g[3 * r + 1] * c.Rin[4] + g[3 * r + 2] * c.Rin[5];
      gz[r] = g[3 * r] * c.Rin[6] + g[3 * r + 1] * c.Rin[7] + g[3 * r + 2] * c.Rin[8];
    }
    double u[3], v[3], gzu[3], gxr[3], gyr[3];
    cross3(c.x, gy, u);  // y = z cross x
    cross3(gy, c.z, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) gz[k] += u[k], gx[k] += v[k];
    const double zg = dot3(c.z, gz);  // z = zu / |zu|
#pragma unroll
    for (int k = 0; k < 3; ++k) gzu[k] = (gz[k] - c.z[k] * zg) / c.nz;
    cross3(c.yr, gzu, u);  // zu = x cross yr
    cross3(gzu, c.x, gyr);
#pragma unroll
    for (int k = 0; k < 3; ++k) gx[k] += u[k];
    const double xg = dot3(c.x, gx);  // x = xr / |xr|
#pragma unroll
    for (int k = 0; k < 3; ++k) gxr[k] = (gx[k] - c.x[k] * xg) / c.nx;
    const double d[9] = {gxr[0], gxr[1], gxr[2], gyr[0], gyr[1], gyr[2], g[9] * c.dxy[0], g[10] * c.dxy[1], g[11] * c.dz};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      grad[9 * b + k] = (float)(up * d[k]);
      if (grad_parts) {  // the same numbers split by term: orientation 0..5, xy 6..7, z 8
        const int term = k < 6 ? 0 : k < 8 ? 1 : 2;
#pragma unroll
        for (int t = 0; t < 3; ++t) grad_parts[27 * b + 9 * t + k] = t == term ? (float)(up * d[k]) : 0.f;
      }
    }
  }
}

int check_sizes(const char* what, int n_sym, int n_pts) {
  HP_REQUIRE(n_sym >= 1 && n_pts >= 1, std::string(what) + ": n_sym and n_pts must be positive");
  HP_REQUIRE((n_sym + kSymChunk - 1) / kSymChunk <= 65535, std::string(what) + ": more than 65535 chunks of symmetries");
  return HP_OK;
}

template <int NT>
int forward(const char* what, int b, const LossArgs& a, float* d_loss, float* d_parts, int32_t* d_ids, float* d_assign, void* d_workspace,
            int64_t workspace_bytes, void* stream) {
  HP_REQUIRE(d_workspace && workspace_bytes >= hp_pose_loss_workspace_bytes(b, a.S),
             std::string(what) + ": workspace smaller than hp_pose_loss_workspace_bytes(b, n_sym)");
  hipStream_t st = (hipStream_t)stream;
  float* tl = (float*)d_workspace;
  hipLaunchKernelGGL(terms_kernel<NT>, dim3(b, (a.S + kSymChunk - 1) / kSymChunk), dim3(kThreads), 0, st, a, tl);
  if (int rc = check_launch(what)) return rc;
  hipLaunchKernelGGL(finish_kernel<NT>, dim3((b + kWave - 1) / kWave), dim3(kWave), 0, st, b, a.S, (const float*)tl, a.gt, d_loss, d_parts,
                     d_ids, d_assign);
  return check_launch(what);
}

// BCEWithLogitsLoss(reduction="none") of x = logit / temperature against y, the rendered-views-logits loss of the coarse
// classifier: a thread is one element.  Everything is formed in double from the float32 inputs and rounded once.
// forward: max(x, 0) - x y + log1p(exp(-|x|)); exp(-|x|) <= 1 cannot overflow, and beyond |x| ~ 37 the last term no longer
// reaches the float32 result (the saturated branch).  backward: (sigmoid(x) - y) / temperature times the upstream gradient, with
// sigmoid(x) = 1 / (1 + e) for x >= 0 and e / (1 + e) for x < 0, e = exp(-|x|).
template <bool kBackward>
__global__ void __launch_bounds__(kThreads) bce_logits_kernel(int64_t n, const float* __restrict__ logits, const float* __restrict__ y,
                                                              double temperature, const float* __restrict__ grad_loss,
                                                              float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double x = (double)logits[i] / temperature, t = (double)y[i];
  const double e = exp(-fabs(x));
  if (kBackward) {
    const double s = x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
    out[i] = (float)(((s - t) / temperature) * (double)grad_loss[i]);
  } else {
    out[i] = (float)(((x > 0.0 ? x : 0.0) - x * t) + log1p(e));
  }
}

}  // namespace
}  // namespace hp

using namespace hp;

extern "C" int hp_loss_bce_logits(int64_t n, const float* d_logits, const float* d_targets, float temperature, float* d_loss,
                                  void* stream) {
  HP_REQUIRE(n >= 0, "hp_loss_bce_logits: negative count");
  HP_REQUIRE(temperature > 0.f && std::isfinite(temperature), "hp_loss_bce_logits: the temperature must be positive and finite");
  if (n == 0) return HP_OK;
  HP_REQUIRE(d_logits && d_targets && d_loss, "hp_loss_bce_logits: null pointer");
  const int64_t n_blocks = (n + kThreads - 1) / kThreads;
  HP_REQUIRE(n_blocks <= 0x7fffffff, "hp_loss_bce_logits: too many elements");
  hipLaunchKernelGGL(bce_logits_kernel<false>, dim3((unsigned)n_blocks), dim3(kThreads), 0, (hipStream_t)stream, n, d_logits, d_targets,
                     (double)temperature, (const float*)nullptr, d_loss);
  return check_launch("hp_loss_bce_logits");
}

extern "C" int hp_loss_bce_logits_backward(int64_t n, const float* d_logits, const float* d_targets, float temperature,
                                           const float* d_grad_loss, float* d_grad_logits, void* stream) {
  HP_REQUIRE(n >= 0, "hp_loss_bce_logits_backward: negative count");
  HP_REQUIRE(temperature > 0.f && std::isfinite(temperature), "hp_loss_bce_logits_backward: the temperature must be positive and finite");
  if (n == 0) return HP_OK;
  HP_REQUIRE(d_logits && d_targets && d_grad_loss && d_grad_logits, "hp_loss_bce_logits_backward: null pointer");
  const int64_t n_blocks = (n + kThreads - 1) / kThreads;
  HP_REQUIRE(n_blocks <= 0x7fffffff, "hp_loss_bce_logits_backward: too many elements");
  hipLaunchKernelGGL(bce_logits_kernel<true>, dim3((unsigned)n_blocks), dim3(kThreads), 0, (hipStream_t)stream, n, d_logits, d_targets,
                     (double)temperature, d_grad_loss, d_grad_logits);
  return check_launch("hp_loss_bce_logits_backward");
}

extern "C" int64_t hp_pose_loss_workspace_bytes(int b, int n_sym) {
  if (b < 0 || n_sym < 1) return -1;
  return (int64_t)b * n_sym * 3 * (int64_t)sizeof(float);
}

extern "C" int hp_loss_co_symmetric(int b, int n_sym, int n_pts, const float* d_TCO_possible_gt, const float* d_TCO_pred,
                                    const float* d_points, float* d_loss, int32_t* d_sym_id, float* d_TCO_assign, void* d_workspace,
                                    int64_t workspace_bytes, void* stream) {
  HP_REQUIRE(b >= 0, "hp_loss_co_symmetric: negative batch");
  if (b == 0) return HP_OK;
  if (int rc = check_sizes("hp_loss_co_symmetric", n_sym, n_pts)) return rc;
  HP_REQUIRE(d_TCO_possible_gt && d_TCO_pred && d_points && d_loss && d_sym_id, "hp_loss_co_symmetric: null pointer");
  const LossArgs a{d_TCO_possible_gt, d_TCO_pred, nullptr, nullptr, nullptr, nullptr, d_points, n_sym, n_pts};
  return forward<1>("hp_loss_co_symmetric", b, a, d_loss, nullptr, d_sym_id, d_TCO_assign, d_workspace, workspace_bytes, stream);
}

extern "C" int hp_loss_co_symmetric_backward(int b, int n_sym, int n_pts, const float* d_TCO_possible_gt, const float* d_TCO_pred,
                                             const float* d_points, const int32_t* d_sym_id, const float* d_grad_loss,
                                             float* d_grad_TCO_pred, void* stream) {
  HP_REQUIRE(b >= 0, "hp_loss_co_symmetric_backward: negative batch");
  if (b == 0) return HP_OK;
  if (int rc = check_sizes("hp_loss_co_symmetric_backward", n_sym, n_pts)) return rc;
  HP_REQUIRE(d_TCO_possible_gt && d_TCO_pred && d_points && d_sym_id && d_grad_loss && d_grad_TCO_pred,
             "hp_loss_co_symmetric_backward: null pointer");
  const LossArgs a{d_TCO_possible_gt, d_TCO_pred, nullptr, nullptr, nullptr, nullptr, d_points, n_sym, n_pts};
  hipLaunchKernelGGL(backward_kernel<1>, dim3(b), dim3(kThreads), 0, (hipStream_t)stream, a, d_sym_id, d_grad_loss, d_grad_TCO_pred,
                     (float*)nullptr);
  return check_launch("hp_loss_co_symmetric_backward");
}

extern "C" int hp_loss_refiner_disentangled(int b, int n_sym, int n_pts, const float* d_TCO_possible_gt, const float* d_TCO_input,
                                            const float* d_refiner_outputs, const float* d_K_crop, const float* d_points,
                                            const float* d_tCR, float* d_loss, float* d_loss_parts, int32_t* d_sym_ids,
                                            void* d_workspace, int64_t workspace_bytes, void* stream) {
  HP_REQUIRE(b >= 0, "hp_loss_refiner_disentangled: negative batch");
  if (b == 0) return HP_OK;
  if (int rc = check_sizes("hp_loss_refiner_disentangled", n_sym, n_pts)) return rc;
  HP_REQUIRE(d_TCO_possible_gt && d_TCO_input && d_refiner_outputs && d_K_crop && d_points && d_loss && d_loss_parts && d_sym_ids,
             "hp_loss_refiner_disentangled: null pointer");
  const LossArgs a{d_TCO_possible_gt, nullptr, d_TCO_input, d_refiner_outputs, d_K_crop, d_tCR, d_points, n_sym, n_pts};
  return forward<3>("hp_loss_refiner_disentangled", b, a, d_loss, d_loss_parts, d_sym_ids, nullptr, d_workspace, workspace_bytes, stream);
}

extern "C" int hp_loss_refiner_disentangled_backward(int b, int n_sym, int n_pts, const float* d_TCO_possible_gt,
                                                     const float* d_TCO_input, const float* d_refiner_outputs, const float* d_K_crop,
                                                     const float* d_points, const float* d_tCR, const int32_t* d_sym_ids,
                                                     const float* d_grad_loss, float* d_grad_outputs, float* d_grad_parts,
                                                     void* stream) {
  HP_REQUIRE(b >= 0, "hp_loss_refiner_disentangled_backward: negative batch");
  if (b == 0) return HP_OK;
  if (int rc = check_sizes("hp_loss_refiner_disentangled_backward", n_sym, n_pts)) return rc;
  HP_REQUIRE(d_TCO_possible_gt && d_TCO_input && d_refiner_outputs && d_K_crop && d_points && d_sym_ids && d_grad_loss && d_grad_outputs,
             "hp_loss_refiner_disentangled_backward: null pointer");
  const LossArgs a{d_TCO_possible_gt, nullptr, d_TCO_input, d_refiner_outputs, d_K_crop, d_tCR, d_points, n_sym, n_pts};
  hipLaunchKernelGGL(backward_kernel<3>, dim3(b), dim3(kThreads), 0, (hipStream_t)stream, a, d_sym_ids, d_grad_loss, d_grad_outputs,
                     d_grad_parts);
  return check_launch("hp_loss_refiner_disentangled_backward");
}
