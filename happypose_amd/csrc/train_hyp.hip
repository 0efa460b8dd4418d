// Hypothesis generation of the trainers' forward-loss step (happypose_amd/training.py): add_noise and TCO_init_from_boxes on rows that
// already live on the device, and the candidate views and hypothesis draw of the coarse classifier.  Entry points and definitions
// are in include/happypose_amd.h (hp_pose_add_noise, hp_tco_init_from_boxes, hp_views_sphere26, hp_coarse_hypotheses).
//
//   add_noise_kernel   a thread is one output row i; it reads pose i / repeat (n_hypotheses noisy copies of a ground truth without
//                      a repeated tensor).  The six noise values of the row are either read (d_noise_in) or drawn:
//                        row   = row_offset + i                                         (64 bits)
//                        call j = 0, 1:  Philox4x32-10, key (seed lo, seed hi), counter (row lo, row hi, j, 0) -> words w[4 j + 0 .. 3]
//                        pair p = 0, 1, 2 takes words (w[2 p], w[2 p + 1]) -- the last two words of call 1 are not used:
//                          u1 = ((w[2 p] >> 8) + 1) 2^-24  in (0, 1],   u2 = (w[2 p + 1] >> 8) 2^-24  in [0, 1)   (exact in fp32: the
//                          mapping of csrc/augment.hip's normal_deviate)
//                          z[2 p] = sqrt(-2 ln u1) cos(2 pi u2),   z[2 p + 1] = sqrt(-2 ln u1) sin(2 pi u2)         (Box-Muller)
//                        noise[k]     = z[k] euler_deg_std[k] pi / 180    k = 0, 1, 2   the angles (ai, aj, ak), radians
//                        noise[3 + k] = z[3 + k] trans_std[k]                           the translation, metres
//                      evaluated in double from the exact u and rounded ONCE to float32: these six floats are what d_noise_out
//                      receives and what the pose part below consumes, so feeding them back as d_noise_in gives the same bits.
//                      Stateless: a row is a function of (seed, row_offset + i) and its pose alone, whatever n and the grid.
//                      Pose part: R_noise = euler2mat(ai, aj, ak) in the static-xyz convention (Rz(ak) Ry(aj) Rx(ai)), sines,
//                      cosines, the nine entries and R R_noise in double from the float32 inputs, each output entry rounded once;
//                      t + dt is one float32 addition.  ai == aj == ak == 0 copies the 3 x 3 block and dt[k] == 0 copies t[k], bit
//                      for bit (a product with the identity would turn -0 into +0); the bottom row is copied.
//                      A thread reads its whole input row before it writes: d_TCO_out may be d_TCO when repeat == 1.
//   init_boxes_kernel  a thread is one row: identity rotation, z = (z_lo + z_hi) / 2, xy = ((box centre - cxcy) z) / fxfy in
//                      float32 in the reference's order of operations; an id outside its table gives a NaN pose and reads row 0.
//   views_sphere26_kernel, coarse_hyp_kernel   described at their definitions; the look-at and the fp32 tail are look_at.h's, the
//                      ones geometry.hip evaluates for the front views.
#include "common.h"
#include "look_at.h"
#include "philox.h"

namespace hp {
namespace {

#pragma clang fp contract(off)  // every product and sum below rounds once, in the order written

constexpr int kThreads = 256;

struct NoiseStd {
  float euler_deg[3], trans[3];
};

// the six float32 noise values of row `row`
__device__ inline void draw_noise(uint64_t row, uint32_t k0, uint32_t k1, const NoiseStd& s, float noise[6]) {
  uint32_t w[8];
#pragma unroll
  for (uint32_t j = 0; j < 2; ++j) {
    uint32_t c[4] = {(uint32_t)row, (uint32_t)(row >> 32), j, 0u};
    philox4x32_10(c, k0, k1);
#pragma unroll
    for (int q = 0; q < 4; ++q) w[4 * j + q] = c[q];
  }
  double z[6];
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const double u1 = (double)((w[2 * p] >> 8) + 1u) * 0x1p-24, u2 = (double)(w[2 * p + 1] >> 8) * 0x1p-24;  // exact
    const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586 * u2;
    z[2 * p] = r * cos(a), z[2 * p + 1] = r * sin(a);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    noise[k] = (float)(z[k] * ((double)s.euler_deg[k] * (3.141592653589793 / 180.0)));
    noise[3 + k] = (float)(z[3 + k] * (double)s.trans[k]);
  }
}

__global__ void __launch_bounds__(kThreads) add_noise_kernel(int n, int repeat, const float* TCO, NoiseStd s, uint32_t k0, uint32_t k1,
                                                             uint64_t row_offset, const float* noise_in, float* TCO_out, float* noise_out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float T[16], nz[6];
  const float* src = TCO + 16 * (i / repeat);  // may alias TCO_out + 16 i (repeat == 1): read whole before the first write
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = src[k];
  if (noise_in) {
#pragma unroll
    for (int k = 0; k < 6; ++k) nz[k] = noise_in[6 * i + k];
  } else {
    draw_noise(row_offset + (uint64_t)i, k0, k1, s, nz);
  }
  float O[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) O[k] = T[k];
  if (!(nz[0] == 0.0f && nz[1] == 0.0f && nz[2] == 0.0f)) {  // NaN angles take this branch and give a NaN block
    const double cx = cos((double)nz[0]), sx = sin((double)nz[0]), cy = cos((double)nz[1]), sy = sin((double)nz[1]);
    const double cz = cos((double)nz[2]), sz = sin((double)nz[2]);
    // transforms3d.euler.euler2mat(ai, aj, ak, 'sxyz') = Rz(ak) Ry(aj) Rx(ai)
    const double Rn[9] = {cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz,
                          cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz,
                          -sy,     sx * cy,                cx * cy};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        O[4 * r + c] = (float)(((double)T[4 * r] * Rn[c] + (double)T[4 * r + 1] * Rn[3 + c]) + (double)T[4 * r + 2] * Rn[6 + c]);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!(nz[3 + k] == 0.0f)) O[4 * k + 3] = T[4 * k + 3] + nz[3 + k];
  }
  float* dst = TCO_out + 16 * i;
#pragma unroll
  for (int k = 0; k < 16; ++k) dst[k] = O[k];
  if (noise_out) {
#pragma unroll
    for (int k = 0; k < 6; ++k) noise_out[6 * i + k] = nz[k];
  }
}

__global__ void __launch_bounds__(kThreads) init_boxes_kernel(int n, const float* __restrict__ boxes, int n_boxes,
                                                              const int32_t* __restrict__ box_ids, const float* __restrict__ K,
                                                              int n_images, const int32_t* __restrict__ im_ids, float z,
                                                              float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t box_id = box_ids ? box_ids[i] : i, im_id = im_ids ? im_ids[i] : i;
  const bool bad_id = (uint64_t)box_id >= (uint64_t)n_boxes || (uint64_t)im_id >= (uint64_t)n_images;
  const float* box = boxes + 4 * (bad_id ? 0 : box_id);
  const float* Ki = K + 9 * (bad_id ? 0 : im_id);
  const float fx = Ki[0], fy = Ki[4], cx = Ki[2], cy = Ki[5];
  const float bcx = (box[0] + box[2]) / 2.0f, bcy = (box[1] + box[3]) / 2.0f;
  float* O = out + 16 * i;
  O[0] = 1.f; O[1] = 0.f; O[2] = 0.f;  O[3] = ((bcx - cx) * z) / fx;
  O[4] = 0.f; O[5] = 1.f; O[6] = 0.f;  O[7] = ((bcy - cy) * z) / fy;
  O[8] = 0.f; O[9] = 0.f; O[10] = 1.f; O[11] = z;
  O[12] = 0.f; O[13] = 0.f; O[14] = 0.f; O[15] = 1.f;
  if (bad_id) {
#pragma unroll
    for (int k = 0; k < 16; ++k) O[k] = __builtin_nanf("");
  }
}

// ---- the coarse classifier's candidate views -------------------------------------------------------------------------------------
constexpr int kSphereViews = HP_SPHERE26_VIEWS;
constexpr int kCandidates = HP_SPHERE26_CANDIDATES;
constexpr int kHypThreads = 128;  // >= kCandidates: one lane per hypothesis slot

// offset `view` of get_26_views_TCO_pos_sphere: y in (0, 1, 2), x in (0, -1, 1), z in (0, 1, -1) nested in that order, (0, 1, 0) left out
__device__ inline void sphere26_offset(int view, int& ox, int& oy, int& oz) {
  const int l = view < 9 ? view : view + 1;  // position among the 27 before (0, 1, 0), the 10th, is removed
  const int xi = (l / 3) % 3, zi = l % 3;
  oy = l / 9;
  ox = xi == 0 ? 0 : (xi == 1 ? -1 : 1);
  oz = zi == 0 ? 0 : (zi == 1 ? 1 : -1);
}

// row-major TCV_O of view `view` of pose T about the reference point tcr (nullptr: T's translation), no in-plane rotation
__device__ inline void sphere26_view(const float* T, const float* tcr_in, int view, float* TV) {
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 12; ++k) fin &= isfinite(T[k]);
  float t[3] = {T[3], T[7], T[11]};
  if (tcr_in) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      t[k] = tcr_in[k];
      fin &= isfinite(t[k]);
    }
  }
  const double tcr[3] = {fin ? (double)t[0] : 0.0, fin ? (double)t[1] : 0.0, fin ? (double)t[2] : 0.0};
  int ox, oy, oz;
  sphere26_offset(view, ox, oy, oz);
  double M[12];
  look_at_view(tcr, ox, oy, oz, true, M);
  view_from_cam0(M, T, TV);
}

// R <- Rz(rot pi / 2) R on the 3 x 3 block with the exact entries 0 / +-1: rows 0 and 1 swap and change sign; t is untouched
__device__ inline void quarter_turns(float* TV, int rot) {
  if (rot == 0) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float r0 = TV[c], r1 = TV[4 + c];
    TV[c] = rot == 1 ? -r1 : (rot == 2 ? -r0 : r1);
    TV[4 + c] = rot == 1 ? r0 : (rot == 2 ? -r1 : -r0);
  }
}

// A lane is one candidate (pose b, view, rot); a wavefront covers 16 views x 4 rotations, or 64 views of two or three poses without
// the rotations.  Unlike pose_prep_kernel, whose 256 lanes all project points with ONE matrix and therefore take it from lane 0,
// every output row here is written by the one lane that evaluated it: no two lanes have to agree on a value but the four
// rotations of a view, which must be exact quarter turns of ONE look-at.  So the lane with rot == 0 is the view's only
// evaluation that is used: the other three of its aligned group of four take its 16 floats by a wavefront shuffle and only
// permute rows.  (All 64 lanes still run the double-precision chain in lockstep; masking three of four would save nothing.)
__global__ void __launch_bounds__(kThreads) views_sphere26_kernel(int64_t n_rows, int rotations, const float* __restrict__ TCO,
                                                                  const float* __restrict__ tCR, float* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = g < n_rows;  // n_rows is a multiple of 4 with rotations: a group of four is live or idle as a whole
  const int64_t row = live ? g : n_rows - 1;
  const int nc = rotations ? kCandidates : kSphereViews;
  const int64_t b = row / nc;
  const int c = (int)(row - b * nc), view = rotations ? c >> 2 : c, rot = rotations ? c & 3 : 0;
  float T[16], TV[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = TCO[16 * b + k];
  sphere26_view(T, tCR ? tCR + 3 * b : nullptr, view, TV);
  if (rotations) {
    const int src = (threadIdx.x & 63) & ~3;
#pragma unroll
    for (int k = 0; k < 16; ++k) TV[k] = __shfl(TV[k], src);
    quarter_turns(TV, rot);
  }
  if (!live) return;
#pragma unroll
  for (int k = 0; k < 16; ++k) out[16 * g + k] = TV[k];
}

// A workgroup is one image.  Lanes 0 .. 26 run one Philox call each (108 words), lane 0 alone walks the partial Fisher-Yates
// over the 104 ids in the LDS (a sequential algorithm of n_hyp <= 104 steps), then lane h evaluates the pose of slot h's id:
// only the selected candidates are formed.
__global__ void __launch_bounds__(kHypThreads) coarse_hyp_kernel(int n_hyp, int n_rendered_views, uint32_t force_threshold,
                                                                 const float* __restrict__ TCO, uint32_t k0, uint32_t k1,
                                                                 uint64_t row_offset, float* __restrict__ hyp,
                                                                 int32_t* __restrict__ view_ids, float* __restrict__ is_positive) {
  __shared__ uint32_t words[4 * (kCandidates / 4 + 1)];
  __shared__ int32_t perm[kCandidates];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (tid <= kCandidates / 4) {
    const uint64_t row = row_offset + (uint64_t)b;
    uint32_t c[4] = {(uint32_t)row, (uint32_t)(row >> 32), (uint32_t)tid, 0u};
    philox4x32_10(c, k0, k1);
#pragma unroll
    for (int q = 0; q < 4; ++q) words[4 * tid + q] = c[q];
  }
  if (tid < kCandidates) perm[tid] = tid;
  __syncthreads();
  if (tid == 0) {
    bool has_positive = false;
    for (int i = 0; i < n_hyp; ++i) {
      const int j = i + (int)(((uint64_t)words[i] * (uint32_t)(kCandidates - i)) >> 32);
      const int32_t pi = perm[i], pj = perm[j];
      perm[i] = pj, perm[j] = pi;
      has_positive |= pj == 0;
    }
    // u = w 2^-32 > p  <=>  w > floor(p 2^32) for the integer w: the host passes the threshold
    if (!has_positive && words[kCandidates] > force_threshold)
      perm[(int)(((uint64_t)words[kCandidates + 1] * (uint32_t)n_rendered_views) >> 32)] = 0;
  }
  __syncthreads();
  if (tid >= n_hyp) return;
  const int id = perm[tid];
  float T[16], TV[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = TCO[16 * b + k];
  sphere26_view(T, nullptr, id >> 2, TV);
  quarter_turns(TV, id & 3);
  const int64_t o = b * n_hyp + tid;
#pragma unroll
  for (int k = 0; k < 16; ++k) hyp[16 * o + k] = TV[k];
  view_ids[o] = id;
  is_positive[o] = id == 0 ? 1.0f : 0.0f;
}

}  // namespace
}  // namespace hp

using namespace hp;

extern "C" int hp_views_sphere26(int b, const float* d_TCO, const float* d_tCR, int inplane_rotations, float* d_TCV_O, void* stream) {
  HP_REQUIRE(b >= 0, "hp_views_sphere26: negative count");
  if (b == 0) return HP_OK;
  HP_REQUIRE(d_TCO && d_TCV_O, "hp_views_sphere26: null pointer");
  const int64_t n_rows = (int64_t)b * (inplane_rotations ? kCandidates : kSphereViews);
  const int64_t n_blocks = (n_rows + kThreads - 1) / kThreads;
  HP_REQUIRE(n_blocks <= 0x7fffffff, "hp_views_sphere26: too many poses");
  hipLaunchKernelGGL(views_sphere26_kernel, dim3((unsigned)n_blocks), dim3(kThreads), 0, (hipStream_t)stream, n_rows,
                     inplane_rotations ? 1 : 0, d_TCO, d_tCR, d_TCV_O);
  return check_launch("hp_views_sphere26");
}

extern "C" int hp_coarse_hypotheses(int b, int n_hyp, int n_rendered_views, double p_force_positive, const float* d_TCO, uint64_t seed,
                                    uint64_t row_offset, float* d_hyp, int32_t* d_view_ids, float* d_is_positive, void* stream) {
  HP_REQUIRE(b >= 0, "hp_coarse_hypotheses: negative count");
  HP_REQUIRE(n_hyp >= 1 && n_hyp <= kCandidates, "hp_coarse_hypotheses: n_hyp must be 1 .. 104");
  HP_REQUIRE(n_rendered_views >= 1 && n_rendered_views <= n_hyp, "hp_coarse_hypotheses: n_rendered_views must be 1 .. n_hyp");
  HP_REQUIRE(p_force_positive >= 0.0 && p_force_positive <= 1.0, "hp_coarse_hypotheses: p_force_positive must be in [0, 1]");
  if (b == 0) return HP_OK;
  HP_REQUIRE(d_TCO && d_hyp && d_view_ids && d_is_positive, "hp_coarse_hypotheses: null pointer");
  // forced where u > 1 - p: the reference's `np.random.rand() > 0.3` for p = 0.7
  const double t = (1.0 - p_force_positive) * 4294967296.0;
  const uint32_t threshold = t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;  // floor; p == 0 never forces
  hipLaunchKernelGGL(coarse_hyp_kernel, dim3((unsigned)b), dim3(kHypThreads), 0, (hipStream_t)stream, n_hyp, n_rendered_views, threshold,
                     d_TCO, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), row_offset, d_hyp, d_view_ids, d_is_positive);
  return check_launch("hp_coarse_hypotheses");
}

extern "C" int hp_pose_add_noise(int n, int repeat, const float* d_TCO, const float* euler_deg_std, const float* trans_std, uint64_t seed,
                                 uint64_t row_offset, const float* d_noise_in, float* d_TCO_out, float* d_noise_out, void* stream) {
  HP_REQUIRE(n >= 0, "hp_pose_add_noise: negative count");
  HP_REQUIRE(repeat >= 1 && n % repeat == 0, "hp_pose_add_noise: repeat must be positive and divide n");
  HP_REQUIRE(d_noise_in || (euler_deg_std && trans_std), "hp_pose_add_noise: standard deviations are needed to draw the noise");
  NoiseStd s{{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  if (!d_noise_in) {
    for (int k = 0; k < 3; ++k) {
      s.euler_deg[k] = euler_deg_std[k], s.trans[k] = trans_std[k];
      HP_REQUIRE(s.euler_deg[k] >= 0.f && s.trans[k] >= 0.f, "hp_pose_add_noise: a standard deviation is negative or NaN");
    }
  }
  if (n == 0) return HP_OK;
  HP_REQUIRE(d_TCO && d_TCO_out, "hp_pose_add_noise: null pointer");
  if (repeat > 1) {  // rows are read by other threads than the one that writes them
    const uintptr_t a0 = (uintptr_t)d_TCO, a1 = a0 + (uintptr_t)(n / repeat) * 64, b0 = (uintptr_t)d_TCO_out, b1 = b0 + (uintptr_t)n * 64;
    HP_REQUIRE(a1 <= b0 || b1 <= a0, "hp_pose_add_noise: d_TCO_out may overlap d_TCO only when repeat == 1");
  } else {
    const uintptr_t a0 = (uintptr_t)d_TCO, b0 = (uintptr_t)d_TCO_out, len = (uintptr_t)n * 64;
    HP_REQUIRE(a0 == b0 || a0 + len <= b0 || b0 + len <= a0, "hp_pose_add_noise: d_TCO_out must be d_TCO itself or not overlap it");
  }
  hipLaunchKernelGGL(add_noise_kernel, dim3((unsigned)(((int64_t)n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, n,
                     repeat, d_TCO, s, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), row_offset, d_noise_in, d_TCO_out,
                     d_noise_out);
  return check_launch("hp_pose_add_noise");
}

extern "C" int hp_tco_init_from_boxes(int n, const float* d_boxes, int n_boxes, const int32_t* d_box_ids, const float* d_K, int n_images,
                                      const int32_t* d_im_ids, float z_lo, float z_hi, float* d_TCO_out, void* stream) {
  HP_REQUIRE(n >= 0, "hp_tco_init_from_boxes: negative count");
  if (n == 0) return HP_OK;
  HP_REQUIRE(n_boxes >= 1 && n_images >= 1, "hp_tco_init_from_boxes: empty box / intrinsics table");
  HP_REQUIRE(d_boxes && d_K && d_TCO_out, "hp_tco_init_from_boxes: null pointer");
  const float z = (z_lo + z_hi) / 2.0f;  // torch.as_tensor(z_range).mean() in float32
  hipLaunchKernelGGL(init_boxes_kernel, dim3((unsigned)(((int64_t)n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, n,
                     d_boxes, n_boxes, d_box_ids, d_K, n_images, d_im_ids, z, d_TCO_out);
  return check_launch("hp_tco_init_from_boxes");
}
