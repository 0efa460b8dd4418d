// Multi-view scene reconstruction (CosyPose's "consistent multi-view" half): the device kernels of the RANSAC candidate matching
// and the host-side seed / inlier bookkeeping.  Entry points and the reference lines they replace: include/happypose_amd.h.
//
// The matching kernels give ONE WAVEFRONT to a row (a seed / a tentative match) and spread the candidate symmetries over its 64 lanes;
// every lane walks the object's points in table order, so a row's result is a function of its inputs alone (no atomics, no
// cross-wave reduction): launch geometry cannot change a bit.  Nothing of size rows x symmetries is ever written to memory.
#include <algorithm>
#include <limits>
#include <map>
#include <numeric>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "common.h"
#include "rigid.h"
#include "wave.h"

namespace hp {
namespace {

constexpr int kRowsPerBlock = 4;  // 256 threads
// Shaped for the tables the matching uses: 8 box-corner points per object (aabb=True) and up to 64 - 128 symmetries.  A lane walks
// all points (and, in the seed kernel, all symmetries of the second object) serially, and only min(n_sym, 64) lanes of a wavefront
// have work: meshes of thousands of points or objects without symmetry use the machine poorly.  Not measured beyond the defaults.

// (value, index) arg-min over the wavefront, lowest index on a tie; every lane ends with the winner
__device__ inline void wave_argmin(float& v, int& idx) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    float ov = __shfl_xor(v, off, kWave);
    int oi = __shfl_xor(idx, off, kWave);
    if (ov < v || (ov == v && oi < idx)) {
      v = ov;
      idx = oi;
    }
  }
}

// symmetric_distance_batched_fast of ONE pair (CP/lib3d/symmetric_distances.py:36-55), by one lane: over the symmetries s of the
// object, the s with the smallest MEAN OF SQUARED point distances between (T1 S_s) p and T2 p (first strict minimum); the value
// is the MEAN OF THE ROOTS for that s.
__device__ inline float symmetric_distance_lane(const T34& T1, const T34& T2, const float* __restrict__ sym, int n_sym,
                                                const float* __restrict__ pts, int n_pts) {
  float best_sq = INFINITY, best = NAN;
  const float inv_n = 1.f / (float)n_pts;
  for (int s = 0; s < n_sym; ++s) {
    const T34 M = mul(T1, load_T(sym + 16 * s));
    float sum_sq = 0.f, sum_rt = 0.f;
    for (int p = 0; p < n_pts; ++p) {
      const float x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
      float ax, ay, az, bx, by, bz;
      apply(M, x, y, z, ax, ay, az);
      apply(T2, x, y, z, bx, by, bz);
      const float dx = ax - bx, dy = ay - by, dz = az - bz;
      const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
      sum_sq += d2;
      sum_rt += sqrtf(d2);
    }
    const float mean_sq = sum_sq * inv_n;
    if (mean_sq < best_sq) {
      best_sq = mean_sq;
      best = sum_rt * inv_n;
    }
  }
  return best;
}

__global__ void __launch_bounds__(kWave* kRowsPerBlock)
    estimate_camera_poses_kernel(int n_seeds, const int32_t* __restrict__ m1c1, const int32_t* __restrict__ m1c2,
                                 const int32_t* __restrict__ m2c1, const int32_t* __restrict__ m2c2,
                                 const float* __restrict__ poses, const int32_t* __restrict__ cand_obj, int n_cand,
                                 const float* __restrict__ points, const float* __restrict__ symmetries,
                                 const int32_t* __restrict__ n_sym, int n_obj, int n_pts, int s_max, float* __restrict__ TC1C2) {
  const int lane = threadIdx.x % kWave;
  const int seed = blockIdx.x * kRowsPerBlock + threadIdx.x / kWave;
  if (seed >= n_seeds) return;  // whole wavefront
  float* out = TC1C2 + 16 * (int64_t)seed;
  const int a = m1c1[seed], b = m1c2[seed], g = m2c1[seed], d = m2c2[seed];
  bool ok = (unsigned)a < (unsigned)n_cand && (unsigned)b < (unsigned)n_cand && (unsigned)g < (unsigned)n_cand &&
            (unsigned)d < (unsigned)n_cand;
  int oa = 0, og = 0, ns_a = 0, ns_g = 0;
  if (ok) {
    oa = cand_obj[a];
    og = cand_obj[g];
    ok = (unsigned)oa < (unsigned)n_obj && (unsigned)og < (unsigned)n_obj;
  }
  if (ok) {
    ns_a = n_sym[oa];
    ns_g = n_sym[og];
    ok = ns_a >= 1 && ns_a <= s_max && ns_g >= 1 && ns_g <= s_max;
  }
  if (!ok) {  // an index outside its table answers NaN, it never reads outside the table
    if (lane < 16) out[lane] = NAN;
    return;
  }
  const T34 TC1Oa = load_T(poses + 16 * (int64_t)a);
  const T34 TObC2 = inverse(load_T(poses + 16 * (int64_t)b));
  const T34 TC1Og = load_T(poses + 16 * (int64_t)g);
  const T34 TC2Od = load_T(poses + 16 * (int64_t)d);
  const float* sym_a = symmetries + 16 * (int64_t)oa * s_max;
  const float* sym_g = symmetries + 16 * (int64_t)og * s_max;
  const float* pts_g = points + 3 * (int64_t)og * n_pts;
  // a lane starts from its first symmetry at +inf, so a distance that is NaN never wins and the winner is always inside the table
  float best = INFINITY;
  int best_s = lane < ns_a ? lane : 0x7fffffff;
  for (int s = lane; s < ns_a; s += kWave) {  // ascending per lane: a strict < keeps the lowest index
    // (TC1Oa @ S @ TObC2) @ TC2Od, the reference's association (ransac.py:43)
    const T34 T2 = mul(mul(mul(TC1Oa, load_T(sym_a + 16 * s)), TObC2), TC2Od);
    const float v = symmetric_distance_lane(TC1Og, T2, sym_g, ns_g, pts_g, n_pts);
    if (v < best) {
      best = v;
      best_s = s;
    }
  }
  wave_argmin(best, best_s);
  if (lane == 0) store_T(out, mul(mul(TC1Oa, load_T(sym_a + 16 * best_s)), TObC2));
}

// Seed-indexed rows of the matching (hp_mv_score_seed_matches): every seed of a view pair lists ALL tentative matches of that pair,
// so the rows of seed n are row_off[n] .. row_off[n + 1] and row r of them is match pair_off[n] + (r - row_off[n]) of the pair
// tables -- nothing per row is uploaded.  row_off == nullptr: explicit (hypothesis_id, cand1, cand2) columns.
struct SeedRows {
  const int32_t* row_off;   // [n_hyp + 1], ascending, row_off[0] == 0, row_off[n_hyp] == n_rows
  const int32_t* pair_off;  // [n_hyp]
  const int32_t* pair_cand1;
  const int32_t* pair_cand2;
  int n_pair_matches;
};

template <int MODE>
__global__ void __launch_bounds__(kWave* kRowsPerBlock)
    score_matches_kernel(SeedRows sr, int n_rows, const int32_t* __restrict__ hyp_id, const int32_t* __restrict__ cand1,
                         const int32_t* __restrict__ cand2, const float* __restrict__ TC1C2, int n_hyp,
                         const float* __restrict__ poses1, const int32_t* __restrict__ obj1, int n_cand1,
                         const float* __restrict__ poses2, int n_cand2, const float* __restrict__ K,
                         const float* __restrict__ points, const float* __restrict__ symmetries,
                         const int32_t* __restrict__ n_sym, int n_obj, int n_pts, int s_max, float* __restrict__ dists,
                         int32_t* __restrict__ sym_ids) {
  const int lane = threadIdx.x % kWave;
  const int row = blockIdx.x * kRowsPerBlock + threadIdx.x / kWave;
  if (row >= n_rows) return;
  int h = -1, c1 = -1, c2 = -1;
  if (sr.row_off) {
    int lo = 0, hi = n_hyp;  // the last seed whose first row is <= row; indices stay inside [0, n_hyp]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (sr.row_off[mid] <= row) lo = mid; else hi = mid;
    }
    if (n_hyp > 0 && sr.row_off[lo] <= row && row < sr.row_off[lo + 1]) {
      const int64_t m = (int64_t)sr.pair_off[lo] + (row - sr.row_off[lo]);
      if (m >= 0 && m < sr.n_pair_matches) {
        h = lo;
        c1 = sr.pair_cand1[m];
        c2 = sr.pair_cand2[m];
      }
    }
  } else {
    h = hyp_id[row];
    c1 = cand1[row];
    c2 = cand2[row];
  }
  bool ok = (unsigned)h < (unsigned)n_hyp && (unsigned)c1 < (unsigned)n_cand1 && (unsigned)c2 < (unsigned)n_cand2;
  int o = 0, ns = 0;
  if (ok) {
    o = obj1[c1];
    ok = (unsigned)o < (unsigned)n_obj;
  }
  if (ok) {
    ns = n_sym[o];
    ok = ns >= 1 && ns <= s_max;
  }
  if (!ok) {
    if (lane == 0) {
      dists[row] = NAN;
      if (sym_ids) sym_ids[row] = -1;
    }
    return;
  }
  const T34 T1 = load_T(poses1 + 16 * (int64_t)c1);
  T34 T2 = mul(load_T(TC1C2 + 16 * (int64_t)h), load_T(poses2 + 16 * (int64_t)c2));
  const float* Kh = K + 9 * (int64_t)h;  // MODE 1 only
  if (MODE == 1) T2 = camera_matrix(Kh, T2);
  const float* sym = symmetries + 16 * (int64_t)o * s_max;
  const float* pts = points + 3 * (int64_t)o * n_pts;
  const float inv_n = 1.f / (float)n_pts;
  float best_key = INFINITY, best_val = NAN;
  int best_s = lane < ns ? lane : 0x7fffffff;
  for (int s = lane; s < ns; s += kWave) {
    T34 M = mul(T1, load_T(sym + 16 * s));
    if (MODE == 1) M = camera_matrix(Kh, M);
    float key_sum = 0.f, val_sum = 0.f;
    for (int p = 0; p < n_pts; ++p) {
      const float x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
      float ax, ay, az, bx, by, bz;
      apply(M, x, y, z, ax, ay, az);
      apply(T2, x, y, z, bx, by, bz);
      if (MODE == 0) {
        const float dx = ax - bx, dy = ay - by, dz = az - bz;
        const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
        key_sum += d2;
        val_sum += sqrtf(d2);
      } else {  // project_points: suv / suv[2], then the L2 pixel distance (symmetric_distances.py:92-100)
        const float du = ax / az - bx / bz, dv = ay / az - by / bz;
        key_sum += sqrtf(fmaf(du, du, dv * dv));
      }
    }
    const float key = key_sum * inv_n;
    const float val = MODE == 0 ? val_sum * inv_n : key;
    if (key < best_key) {
      best_key = key;
      best_val = val;
      best_s = s;
    }
  }
  float key = best_key;
  int win = best_s;
  wave_argmin(key, win);
  const int owner = win % kWave;  // symmetry s was evaluated by lane s % 64
  const float val = __shfl(best_val, owner, kWave);
  if (lane == 0) {
    dists[row] = val;
    if (sym_ids) sym_ids[row] = win;
  }
}

// ---- bundle adjustment: residuals and normal-equation blocks of one linearisation ---------------------------------------------

// forward-mode derivative: (value, d value / d theta_k) for ONE parameter k; the chain rule through the Gram-Schmidt of
// compute_transform_from_pose9d is carried exactly by the arithmetic below (no finite differences)
// Double precision: the normal equations are solved in float64 on the host, and with float32 blocks the LM run of an
// ill-conditioned scene (known cameras: the gauge directions stay in J) takes another accept / reject path than float64 does
// and can stop early; the kernel is a few wavefronts, its cost does not show.
struct Dual {
  double v, d;
};
__device__ inline Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
__device__ inline Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
__device__ inline Dual operator*(Dual a, Dual b) { return {a.v * b.v, fma(a.d, b.v, a.v * b.d)}; }
__device__ inline Dual operator/(Dual a, Dual b) {
  const double q = a.v / b.v;
  return {q, (a.d - q * b.d) / b.v};
}
__device__ inline Dual dsqrt(Dual a) {
  const double r = sqrt(a.v);
  return {r, a.d / (2. * r)};
}

// compute_transform_from_pose9d (CP/lib3d/transform_ops.py:57-67) with compute_rotation_matrix_from_ortho6d
// (TB/lib3d/rotations.py:22-36): x = x_raw / |x_raw|, z = x cross y_raw, z /= |z|, y = z cross x, R = [x y z] (columns); T[12]
// row-major 3 x 4.  `seed` in 0..8 marks the parameter the derivative is taken for (-1: none).
__device__ inline void pose9d_transform(const double* __restrict__ p9, int seed, Dual* T) {
  Dual q[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) q[i] = {p9[i], i == seed ? 1. : 0.};
  const Dual nx = dsqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  const Dual x0 = q[0] / nx, x1 = q[1] / nx, x2 = q[2] / nx;
  Dual z0 = x1 * q[5] - x2 * q[4], z1 = x2 * q[3] - x0 * q[5], z2 = x0 * q[4] - x1 * q[3];
  const Dual nz = dsqrt(z0 * z0 + z1 * z1 + z2 * z2);
  z0 = z0 / nz;
  z1 = z1 / nz;
  z2 = z2 / nz;
  const Dual y0 = z1 * x2 - z2 * x1, y1 = z2 * x0 - z0 * x2, y2 = z0 * x1 - z1 * x0;
  T[0] = x0; T[1] = y0; T[2] = z0; T[3] = q[6];
  T[4] = x1; T[5] = y1; T[6] = z1; T[7] = q[7];
  T[8] = x2; T[9] = y2; T[10] = z2; T[11] = q[8];
}

constexpr int kBaParams = 18;                                // 9 of the candidate's object, 9 of its view
constexpr int kBaEntries = kBaParams * kBaParams + kBaParams;  // JtJ block + Jte
constexpr int kBaPerLane = (kBaEntries + kWave - 1) / kWave;

// One wavefront per candidate.  Lane k < 18 carries d/d theta_k of the projection of every point; the points are walked in
// table order and every lane adds its entries of J^T J and J^T e in that order: the block is a function of the candidate alone.
__global__ void __launch_bounds__(kWave)
    ba_linearize_kernel(int n_cand, const double* __restrict__ TWO_9d, int n_obj, const double* __restrict__ TCW_9d, int n_views,
                        const int32_t* __restrict__ cand_obj, const int32_t* __restrict__ cand_view,
                        const float* __restrict__ TCO_cand, const float* __restrict__ K, const float* __restrict__ obj_points,
                        int n_pts, double residuals_threshold, double* __restrict__ errors, double* __restrict__ clipped,
                        double* __restrict__ JtJ, double* __restrict__ Jte) {
  __shared__ double s_ju[kBaParams], s_jv[kBaParams], s_e[2];
  const int lane = threadIdx.x;
  const int c = blockIdx.x;
  if (c >= n_cand) return;
  const int o = cand_obj[c], v = cand_view[c];
  double* err_c = errors + 2 * (int64_t)c * n_pts;
  double* clip_c = clipped + 2 * (int64_t)c * n_pts;
  if ((unsigned)o >= (unsigned)n_obj || (unsigned)v >= (unsigned)n_views) {
    for (int i = lane; i < 2 * n_pts; i += kWave) err_c[i] = clip_c[i] = NAN;
    for (int i = lane; i < kBaParams * kBaParams; i += kWave) JtJ[(int64_t)c * kBaParams * kBaParams + i] = NAN;
    if (lane < kBaParams) Jte[(int64_t)c * kBaParams + lane] = NAN;
    return;
  }
  // TCO = TCW(theta_view) TWO(theta_obj); lanes 0..8 differentiate the object's parameters, 9..17 the view's, the rest none
  Dual TWO[12], TCW[12], P[12];
  pose9d_transform(TWO_9d + 9 * (int64_t)o, lane < 9 ? lane : -1, TWO);
  pose9d_transform(TCW_9d + 9 * (int64_t)v, lane >= 9 && lane < kBaParams ? lane - 9 : -1, TCW);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      Dual sacc = TCW[4 * i] * TWO[j] + TCW[4 * i + 1] * TWO[4 + j] + TCW[4 * i + 2] * TWO[8 + j];
      P[4 * i + j] = j == 3 ? sacc + TCW[4 * i + 3] : sacc;
    }
  const float* Kv = K + 9 * (int64_t)v;
  // camera matrices K @ T[:3] (project_points, CP/lib3d/camera_geometry.py:15)
  Dual KP[12];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const Dual k0 = {Kv[3 * i], 0.}, k1 = {Kv[3 * i + 1], 0.}, k2 = {Kv[3 * i + 2], 0.};
      KP[4 * i + j] = k0 * P[j] + k1 * P[4 + j] + k2 * P[8 + j];
    }
  const float* Tc = TCO_cand + 16 * (int64_t)c;  // y = project(K, TCO_cand p), in double as well
  double KC[12];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j)
      KC[4 * i + j] = (double)Kv[3 * i] * Tc[j] + (double)Kv[3 * i + 1] * Tc[4 + j] + (double)Kv[3 * i + 2] * Tc[8 + j];
  const float* pts = obj_points + 3 * (int64_t)o * n_pts;
  double acc[kBaPerLane];
#pragma unroll
  for (int m = 0; m < kBaPerLane; ++m) acc[m] = 0.;
  for (int p = 0; p < n_pts; ++p) {
    const double x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
    const Dual dx = {x, 0.}, dy = {y, 0.}, dz = {z, 0.};
    const Dual su = KP[0] * dx + KP[1] * dy + KP[2] * dz + KP[3];
    const Dual sv = KP[4] * dx + KP[5] * dy + KP[6] * dz + KP[7];
    const Dual sw = KP[8] * dx + KP[9] * dy + KP[10] * dz + KP[11];
    const Dual u = su / sw, w = sv / sw;  // yhat
    if (lane < kBaParams) {
      s_ju[lane] = u.d;
      s_jv[lane] = w.d;
    }
    if (lane == 0) {
      const double cu = KC[0] * x + KC[1] * y + KC[2] * z + KC[3], cv = KC[4] * x + KC[5] * y + KC[6] * z + KC[7],
                   cw = KC[8] * x + KC[9] * y + KC[10] * z + KC[11];
      const double eu = cu / cw - u.v, ev = cv / cw - w.v;  // errors = y - yhat (bundle_adjustment.py:257-259)
      s_e[0] = eu;
      s_e[1] = ev;
      err_c[2 * p] = eu;
      err_c[2 * p + 1] = ev;
      clip_c[2 * p] = fmin(eu * eu, residuals_threshold);
      clip_c[2 * p + 1] = fmin(ev * ev, residuals_threshold);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kBaPerLane; ++m) {
      const int e = lane + kWave * m;
      if (e < kBaParams * kBaParams) {
        const int i = e / kBaParams, j = e % kBaParams;
        acc[m] = fma(s_ju[i], s_ju[j], fma(s_jv[i], s_jv[j], acc[m]));
      } else if (e < kBaEntries) {
        const int i = e - kBaParams * kBaParams;
        acc[m] = fma(s_ju[i], s_e[0], fma(s_jv[i], s_e[1], acc[m]));
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < kBaPerLane; ++m) {
    const int e = lane + kWave * m;
    if (e < kBaParams * kBaParams) JtJ[(int64_t)c * kBaParams * kBaParams + e] = acc[m];
    else if (e < kBaEntries) Jte[(int64_t)c * kBaParams + e - kBaParams * kBaParams] = acc[m];
  }
}

int check_tables(const char* what, const void* d_points, const void* d_sym, const void* d_n_sym, int n_obj, int n_pts, int s_max) {
  HP_REQUIRE(d_points && d_sym && d_n_sym, std::string(what) + ": mesh tables missing");
  HP_REQUIRE(n_obj >= 1 && n_pts >= 1 && s_max >= 1, std::string(what) + ": n_obj, n_pts and s_max must be positive");
  HP_REQUIRE((int64_t)n_obj * s_max < (int64_t(1) << 26) && (int64_t)n_obj * n_pts < (int64_t(1) << 28),
             std::string(what) + ": mesh tables too large");
  return HP_OK;
}

}  // namespace
}  // namespace hp

using namespace hp;

extern "C" int hp_mv_estimate_camera_poses(int n_seeds, const int32_t* d_match1_cand1, const int32_t* d_match1_cand2,
                                           const int32_t* d_match2_cand1, const int32_t* d_match2_cand2, const float* d_poses,
                                           const int32_t* d_cand_obj, int n_cand, const float* d_points,
                                           const float* d_symmetries, const int32_t* d_n_sym, int n_obj, int n_pts, int s_max,
                                           float* d_TC1C2, void* stream) {
  HP_REQUIRE(n_seeds >= 0 && n_cand >= 0, "hp_mv_estimate_camera_poses: negative size");
  if (int rc = check_tables("hp_mv_estimate_camera_poses", d_points, d_symmetries, d_n_sym, n_obj, n_pts, s_max)) return rc;
  if (n_seeds == 0) return HP_OK;
  HP_REQUIRE(d_match1_cand1 && d_match1_cand2 && d_match2_cand1 && d_match2_cand2 && d_poses && d_cand_obj && d_TC1C2,
             "hp_mv_estimate_camera_poses: null pointer");
  HP_REQUIRE(n_seeds <= (1 << 29), "hp_mv_estimate_camera_poses: too many seeds");
  const int blocks = (n_seeds + kRowsPerBlock - 1) / kRowsPerBlock;
  hipLaunchKernelGGL(estimate_camera_poses_kernel, dim3(blocks), dim3(kWave * kRowsPerBlock), 0, (hipStream_t)stream, n_seeds,
                     d_match1_cand1, d_match1_cand2, d_match2_cand1, d_match2_cand2, d_poses, d_cand_obj, n_cand, d_points,
                     d_symmetries, d_n_sym, n_obj, n_pts, s_max, d_TC1C2);
  return check_launch("hp_mv_estimate_camera_poses");
}

extern "C" int hp_mv_score_matches(int n_rows, const int32_t* d_hypothesis_id, const int32_t* d_cand1, const int32_t* d_cand2,
                                   const float* d_TC1C2, int n_hyp, const float* d_poses1, const int32_t* d_obj1, int n_cand1,
                                   const float* d_poses2, int n_cand2, const float* d_K, int mode, const float* d_points,
                                   const float* d_symmetries, const int32_t* d_n_sym, int n_obj, int n_pts, int s_max,
                                   float* d_dists, int32_t* d_sym_ids, void* stream) {
  HP_REQUIRE(n_rows >= 0 && n_hyp >= 0 && n_cand1 >= 0 && n_cand2 >= 0, "hp_mv_score_matches: negative size");
  HP_REQUIRE(mode == HP_MV_DIST_3D || mode == HP_MV_DIST_REPROJECTED, "hp_mv_score_matches: unknown mode");
  HP_REQUIRE(mode == HP_MV_DIST_3D || d_K, "hp_mv_score_matches: the reprojected distance needs d_K [n_hyp][9]");
  if (int rc = check_tables("hp_mv_score_matches", d_points, d_symmetries, d_n_sym, n_obj, n_pts, s_max)) return rc;
  if (n_rows == 0) return HP_OK;
  HP_REQUIRE(d_hypothesis_id && d_cand1 && d_cand2 && d_TC1C2 && d_poses1 && d_obj1 && d_poses2 && d_dists,
             "hp_mv_score_matches: null pointer");
  HP_REQUIRE(n_rows <= (1 << 29), "hp_mv_score_matches: too many rows");
  const int blocks = (n_rows + kRowsPerBlock - 1) / kRowsPerBlock;
  auto kernel = mode == HP_MV_DIST_3D ? score_matches_kernel<0> : score_matches_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kWave * kRowsPerBlock), 0, (hipStream_t)stream, SeedRows{}, n_rows, d_hypothesis_id, d_cand1,
                     d_cand2, d_TC1C2, n_hyp, d_poses1, d_obj1, n_cand1, d_poses2, n_cand2, d_K, d_points, d_symmetries, d_n_sym,
                     n_obj, n_pts, s_max, d_dists, d_sym_ids);
  return check_launch("hp_mv_score_matches");
}

extern "C" int hp_mv_score_seed_matches(int n_rows, int n_seeds, const int32_t* d_row_offsets, const int32_t* d_pair_offsets,
                                        const int32_t* d_pair_cand1, const int32_t* d_pair_cand2, int n_pair_matches,
                                        const float* d_TC1C2, const float* d_poses, const int32_t* d_cand_obj, int n_cand,
                                        const float* d_points, const float* d_symmetries, const int32_t* d_n_sym, int n_obj,
                                        int n_pts, int s_max, float* d_dists, void* stream) {
  HP_REQUIRE(n_rows >= 0 && n_seeds >= 0 && n_cand >= 0 && n_pair_matches >= 0, "hp_mv_score_seed_matches: negative size");
  if (int rc = check_tables("hp_mv_score_seed_matches", d_points, d_symmetries, d_n_sym, n_obj, n_pts, s_max)) return rc;
  if (n_rows == 0) return HP_OK;
  HP_REQUIRE(d_row_offsets && d_pair_offsets && d_pair_cand1 && d_pair_cand2 && d_TC1C2 && d_poses && d_cand_obj && d_dists,
             "hp_mv_score_seed_matches: null pointer");
  HP_REQUIRE(n_rows <= (1 << 29) && n_seeds >= 1, "hp_mv_score_seed_matches: rows without seeds, or too many rows");
  const int blocks = (n_rows + kRowsPerBlock - 1) / kRowsPerBlock;
  const SeedRows sr{d_row_offsets, d_pair_offsets, d_pair_cand1, d_pair_cand2, n_pair_matches};
  hipLaunchKernelGGL(score_matches_kernel<0>, dim3(blocks), dim3(kWave * kRowsPerBlock), 0, (hipStream_t)stream, sr, n_rows, nullptr,
                     nullptr, nullptr, d_TC1C2, n_seeds, d_poses, d_cand_obj, n_cand, d_poses, n_cand, nullptr, d_points,
                     d_symmetries, d_n_sym, n_obj, n_pts, s_max, d_dists, nullptr);
  return check_launch("hp_mv_score_seed_matches");
}

extern "C" int hp_mv_ba_linearize(int n_cand, const double* d_TWO_9d, int n_obj, const double* d_TCW_9d, int n_views,
                                  const int32_t* d_cand_obj, const int32_t* d_cand_view, const float* d_TCO_cand, const float* d_K,
                                  const float* d_obj_points, int n_pts, double residuals_threshold, double* d_errors,
                                  double* d_clipped, double* d_JtJ, double* d_Jte, void* stream) {
  HP_REQUIRE(n_cand >= 0 && n_obj >= 1 && n_views >= 1 && n_pts >= 1, "hp_mv_ba_linearize: n_obj, n_views and n_pts must be positive");
  HP_REQUIRE((int64_t)n_obj * n_pts < (int64_t(1) << 28) && n_cand <= (1 << 24), "hp_mv_ba_linearize: tables too large");
  if (n_cand == 0) return HP_OK;
  HP_REQUIRE(d_TWO_9d && d_TCW_9d && d_cand_obj && d_cand_view && d_TCO_cand && d_K && d_obj_points && d_errors && d_clipped &&
                 d_JtJ && d_Jte,
             "hp_mv_ba_linearize: null pointer");
  hipLaunchKernelGGL(ba_linearize_kernel, dim3(n_cand), dim3(kWave), 0, (hipStream_t)stream, n_cand, d_TWO_9d, n_obj, d_TCW_9d,
                     n_views, d_cand_obj, d_cand_view, d_TCO_cand, d_K, d_obj_points, n_pts, residuals_threshold, d_errors,
                     d_clipped, d_JtJ, d_Jte);
  return check_launch("hp_mv_ba_linearize");
}

// ---- host side: RANSAC seeds, tentative matches and the inlier search -------------------------------------------------------

namespace {

struct Match {
  int c1, c2;
};
using ViewPair = std::pair<int, int>;

std::vector<int> shuffled_range(int n, int seed) {
  std::vector<int> v(n);
  std::iota(v.begin(), v.end(), 0);
  std::shuffle(v.begin(), v.end(), std::default_random_engine(seed));
  return v;
}

}  // namespace

extern "C" int hp_ransac_make_infos(int n_cand, const int32_t* h_view_ids, const int32_t* h_label_ids, int n_ransac_iter,
                                    int seed, int64_t* n_seeds, int64_t* n_matches, int32_t* h_seeds, int64_t cap_seeds,
                                    int32_t* h_matches, int64_t cap_matches) {
  HP_REQUIRE(n_cand >= 0 && n_seeds && n_matches, "hp_ransac_make_infos: bad arguments");
  HP_REQUIRE(n_cand == 0 || (h_view_ids && h_label_ids), "hp_ransac_make_infos: null candidate table");
  std::map<ViewPair, std::vector<Match>> tentative;  // key order = (view1, view2) ascending
  for (int n = 0; n < n_cand; ++n)
    for (int m = 0; m < n_cand; ++m)
      if (h_view_ids[n] != h_view_ids[m] && h_label_ids[n] == h_label_ids[m]) tentative[{h_view_ids[n], h_view_ids[m]}].push_back({n, m});
  const bool write = h_seeds || h_matches;
  HP_REQUIRE(!write || (h_seeds && h_matches), "hp_ransac_make_infos: give both output tables or neither");
  int64_t ns = 0, nm = 0;
  for (const auto& kv : tentative) {
    const std::vector<Match>& tm = kv.second;
    const int t = (int)tm.size();
    const std::vector<int> perm1 = shuffled_range(t, seed), perm2 = shuffled_range(t, seed + 1);
    int n_pairs = 0;
    for (int i1 : perm1) {
      if (n_pairs >= n_ransac_iter) break;
      for (int i2 : perm2) {
        if (n_pairs >= n_ransac_iter) break;
        if (i1 == i2) continue;
        if (write) {
          HP_REQUIRE(ns < cap_seeds && nm + t <= cap_matches, "hp_ransac_make_infos: output tables too small");
          const int32_t row[6] = {kv.first.first, kv.first.second, tm[i1].c1, tm[i1].c2, tm[i2].c1, tm[i2].c2};
          for (int k = 0; k < 6; ++k) h_seeds[k * cap_seeds + ns] = row[k];
          for (int i = 0; i < t; ++i) {
            h_matches[0 * cap_matches + nm + i] = (int32_t)ns;
            h_matches[1 * cap_matches + nm + i] = tm[i].c1;
            h_matches[2 * cap_matches + nm + i] = tm[i].c2;
          }
        }
        ++n_pairs;
        ++ns;
        nm += t;
        HP_REQUIRE(ns < (int64_t(1) << 30) && nm < (int64_t(1) << 30), "hp_ransac_make_infos: more than 2^30 rows");
      }
    }
  }
  *n_seeds = ns;
  *n_matches = nm;
  return HP_OK;
}

extern "C" int hp_ransac_find_inliers(int64_t n_hyp, const int32_t* h_view1, const int32_t* h_view2, int64_t n_matches,
                                      const int32_t* h_hypothesis_id, const int32_t* h_cand1, const int32_t* h_cand2,
                                      const float* h_dists, float dist_threshold, int n_min_inliers, int32_t* h_inlier_cand1,
                                      int32_t* h_inlier_cand2, int64_t* n_inliers, int32_t* h_best_hypotheses, int64_t* n_best) {
  HP_REQUIRE(n_hyp >= 0 && n_matches >= 0 && n_inliers && n_best, "hp_ransac_find_inliers: bad arguments");
  HP_REQUIRE(n_hyp == 0 || (h_view1 && h_view2 && h_best_hypotheses), "hp_ransac_find_inliers: null hypothesis table");
  HP_REQUIRE(n_matches == 0 || (h_hypothesis_id && h_cand1 && h_cand2 && h_dists && h_inlier_cand1 && h_inlier_cand2),
             "hp_ransac_find_inliers: null match table");
  struct Hypothesis {
    std::vector<Match> inliers, uniques;
    std::vector<float> dists;
    float dists_sum = 0.f;
    int n_inliers = 0;
  };
  std::vector<Hypothesis> hyps((size_t)n_hyp);
  std::map<ViewPair, std::vector<int>> by_pair;
  for (int64_t n = 0; n < n_hyp; ++n) by_pair[{h_view1[n], h_view2[n]}].push_back((int)n);
  for (int64_t n = 0; n < n_matches; ++n) {
    const int h = h_hypothesis_id[n];
    HP_REQUIRE(h >= 0 && h < n_hyp, "hp_ransac_find_inliers: hypothesis id outside the seed table");
    if (h_dists[n] <= dist_threshold) {
      hyps[h].inliers.push_back({h_cand1[n], h_cand2[n]});
      hyps[h].dists.push_back(h_dists[n]);
    }
  }
  // one-to-one matches of every hypothesis: greedily by ascending distance (stable)
  for (Hypothesis& hy : hyps) {
    std::vector<int> order(hy.dists.size());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int i, int j) { return hy.dists[i] < hy.dists[j]; });
    std::set<int> used1, used2;
    for (int i : order) {
      const Match& m = hy.inliers[i];
      if (used1.count(m.c1) || used2.count(m.c2)) continue;
      used1.insert(m.c1);
      used2.insert(m.c2);
      hy.uniques.push_back(m);
      hy.dists_sum += hy.dists[i];
      hy.n_inliers += 1;
    }
  }
  int64_t ni = 0, nb = 0;
  for (const auto& kv : by_pair) {
    int best = -1, best_n = 0;
    float best_sum = std::numeric_limits<float>::max();
    for (int h : kv.second) {
      const Hypothesis& hy = hyps[h];
      if (hy.n_inliers >= n_min_inliers && (hy.n_inliers > best_n || (hy.n_inliers == best_n && hy.dists_sum < best_sum))) {
        best = h;
        best_n = hy.n_inliers;
        best_sum = hy.dists_sum;
      }
    }
    if (best > 0) {  // the reference's `> 0`: hypothesis 0 can never be kept (see the header)
      h_best_hypotheses[nb++] = best;
      for (const Match& m : hyps[best].uniques) {
        h_inlier_cand1[ni] = m.c1;
        h_inlier_cand2[ni] = m.c2;
        ++ni;
      }
    }
  }
  *n_inliers = ni;
  *n_best = nb;
  return HP_OK;
}
