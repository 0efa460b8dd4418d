// Depth refinement, second kind: robust registration in the manner of TEASER++ between the depth
// rendered at the predicted pose and the measured depth (InferenceConfig.depth_refiner = "teaserpp").
//
// Reference: MP/inference/teaserpp_refiner.py:54-294 + refiner_utils.py:27-53 +
// TB/visualization/meshcat_utils.py:297-320.  Its pipeline is kept:
//   mask      = rendered > 0 & measured > 0 ("simple"), & |measured - rendered| <= depth_delta_thresh
//               ("threshold"); fewer than n_min_points pixels -> the pose is kept          (:255-266)
//   points    = back-projection x = (u - cx) d / fx, y = (v - cy) d / fy, z = d of BOTH depth maps at the
//               masked pixels, row-major; the two points of a pixel are a correspondence (a_i, b_i)
//   sampling  = farthest-point sampling of the rendered points down to min(n_points, N): starts at
//               index 0, takes the point farthest from the chosen set, ties to the lowest index
//   solve     = robust registration b ~ R a + t without scale, noise_bound, cbar2 = 1, GNC-TLS rotation
//               with factor 1.4, 100 iterations, cost threshold 1e-12                       (:39-51)
//   accept    = #{i: |R a_i + t - b_i| < noise_bound} >= min_num_inliers -> TCO = T TCO_pred (:280-289)
// The solver itself is the teaserpp_python library there and the sampling is pytorch3d's -- third-party
// code that is not in this image and cannot be restated bit for bit: PARITY UNPINNED.  Here the
// registration is restated from its published definition (Yang, Shi, Carlone, "TEASER: Fast and
// Certifiable Point Cloud Registration", 2020), per prediction, M <= 1024 correspondences,
// beta = 2 noise_bound sqrt(cbar2), alpha = noise_bound sqrt(cbar2):
//   * consistency graph: i ~ j when | |b_j - b_i| - |a_j - a_i| | < beta (fp32), M bit rows of 32 words;
//   * clique: a deterministic GREEDY clique -- candidates C = all; repeat: v = argmax popcount(adj[v] & C)
//     over v in C (ties to the lowest index), append v, C &= adj[v].  THIS DEPARTS from the library's
//     default, an exact maximum clique (NP-hard); with the pixel-aligned correspondences of this refiner
//     the graph is near-complete when the pose is near right, and the two then coincide.  Fewer than 3
//     members -> the pose is kept;
//   * rotation: chain measurements between consecutive clique members (sorted by index), GNC-TLS with
//     nb^2 = beta^2: weighted closed-form rotation from the SVD of sum w a b^T, mu from the largest
//     residual on the first iteration, the TLS weight update, mu <- 1.4 mu, stop on |cost - cost_prev| < 1e-12;
//   * translation: per axis, truncated least squares over the clique's members, the candidates being
//     the midpoints between consecutive sorted interval ends x_i -+ alpha (O(m^2) per axis).
// tests/teaserpp_ref.py restates exactly this definition on the CPU.
//
// Layout of the work: one workgroup of 1024 threads (16 waves) per prediction in every kernel, because each
// stage is a sequence of steps over one prediction's points.  In the solve kernel thread v builds row v of the
// consistency graph itself and KEEPS it in 32 registers for the whole clique search (the row is read at every
// greedy step); the graph is in neither LDS nor global memory.  Everything after the graph runs in fp64 with
// sums in a fixed order (lanes by xor-shuffle, then the 16 waves in turn): results are bit-identical from run to run.
#include <cmath>

#include "common.h"
#include "wave.h"

namespace hp {
namespace {

constexpr int kThreads = 1024;          // one workgroup per prediction
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxM = 1024;             // correspondences per prediction
constexpr int kWords = kMaxM / 32;      // words of a bit row
constexpr double kCbar2 = 1.0;
constexpr double kGncFactor = 1.4;
constexpr int kGncMaxIterations = 100;
constexpr double kGncCostThreshold = 1e-12;

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }

// ---- correspondences: ordered compaction of the masked pixels of one prediction -------------------------
__global__ __launch_bounds__(kThreads) void teaser_correspond_kernel(const float* depth_r, const float* depth_m, const int32_t* im_ids,
                                                                     const float* K, int H, int W, int use_thresh, float delta,
                                                                     float* pts_a, int32_t* pix, int32_t* count) {
  __shared__ int wtot[2][kWaves];
  const int n = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  const int HW = H * W;
  const float* dr = depth_r + (int64_t)n * HW;
  const float* dm = depth_m + (int64_t)im_ids[n] * HW;
  const float* k = K + (int64_t)n * 9;
  const float fx = k[0], fy = k[4], cx = k[2], cy = k[5];
  float* pa = pts_a + (int64_t)n * HW * 3;
  int32_t* px = pix + (int64_t)n * HW;
  int base = 0, buf = 0;
  for (int p0 = 0; p0 < HW; p0 += kThreads, buf ^= 1) {
    const int p = p0 + tid;
    float zr = 0.f, zm = 0.f;
    if (p < HW) { zr = dr[p]; zm = dm[p]; }
    bool ok = zr > 0.f && zm > 0.f;
    if (use_thresh) ok = ok && fabsf(zm - zr) <= delta;
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) wtot[buf][wave] = __popcll(bal);
    __syncthreads();  // wtot is double-buffered: one barrier per chunk
    int off = base, total = 0;
    for (int w = 0; w < kWaves; ++w) {
      const int c = wtot[buf][w];
      if (w < wave) off += c;
      total += c;
    }
    if (ok) {
      const int o = off + __popcll(bal & ((1ull << lane) - 1ull));  // o < HW: one slot per masked pixel
      const int v = p / W, u = p - v * W;
      pa[(int64_t)o * 3 + 0] = ((float)u - cx) * zr / fx;
      pa[(int64_t)o * 3 + 1] = ((float)v - cy) * zr / fy;
      pa[(int64_t)o * 3 + 2] = zr;
      px[o] = p;
    }
    base += total;
  }
  if (tid == 0) count[n] = base;
}

// ---- farthest-point sampling -------------------------------------------------------------------------
// indices[n][0 .. min(k, N)) = the selection in order, -1 after it; nothing is selected when N < min_count.
__global__ __launch_bounds__(kThreads) void teaser_fps_kernel(const float* points, int n_max, const int32_t* counts, int min_count, int k,
                                                              float* mind, int32_t* indices) {
  __shared__ float red_d[2][kWaves];
  __shared__ int red_i[2][kWaves];
  const int n = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  int N = counts[n];
  N = N < 0 ? 0 : (N > n_max ? n_max : N);
  if (N < min_count) N = 0;
  const int M = k < N ? k : N;
  int32_t* out = indices + (int64_t)n * k;
  for (int j = M + tid; j < k; j += kThreads) out[j] = -1;
  if (M == 0) return;
  const float* P = points + (int64_t)n * n_max * 3;
  float* md = mind + (int64_t)n * n_max;
  for (int i = tid; i < N; i += kThreads) md[i] = INFINITY;  // md[i] is only ever touched by thread i % kThreads
  int last = 0;
  if (tid == 0) out[0] = 0;
  for (int s = 1; s < M; ++s) {
    const float lx = P[(int64_t)last * 3], ly = P[(int64_t)last * 3 + 1], lz = P[(int64_t)last * 3 + 2];
    float bd = -1.f;
    int bi = 0x7fffffff;
    for (int i = tid; i < N; i += kThreads) {
      const float dx = P[(int64_t)i * 3] - lx, dy = P[(int64_t)i * 3 + 1] - ly, dz = P[(int64_t)i * 3 + 2] - lz;
      const float m = fminf(md[i], dx * dx + dy * dy + dz * dz);
      md[i] = m;
      if (m > bd) { bd = m; bi = i; }  // increasing i: the lowest index of a tie stays
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float od = __shfl_xor(bd, off);
      const int oi = __shfl_xor(bi, off);
      if (od > bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    const int buf = s & 1;
    if (lane == 0) { red_d[buf][wave] = bd; red_i[buf][wave] = bi; }
    __syncthreads();  // double-buffered: one barrier per step
    bd = red_d[buf][0]; bi = red_i[buf][0];
    for (int w = 1; w < kWaves; ++w) {
      const float od = red_d[buf][w];
      const int oi = red_i[buf][w];
      if (od > bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    last = bi;  // thread 0 owns point 0 and its distance is >= 0 > -1: always an index below N
    if (tid == 0) out[s] = last;
  }
}

// ---- the sampled correspondences: a from the compacted rendered points, b back-projected from the measured depth ----
__global__ __launch_bounds__(kThreads) void teaser_gather_kernel(const float* pts_a, const int32_t* pix, const int32_t* count,
                                                                 const int32_t* indices, const float* depth_m, const int32_t* im_ids,
                                                                 const float* K, int H, int W, int n_min_points, int n_points, int use_fps,
                                                                 float* a, float* b, int32_t* m_sel) {
  const int n = blockIdx.x, j = threadIdx.x;
  const int HW = H * W;
  const int N = count[n];
  const bool enough = N >= n_min_points;
  const int M = enough ? (n_points < N ? n_points : N) : 0;
  if (j == 0) m_sel[n] = enough ? M : -1;
  if (j >= n_points) return;
  float av[3] = {0.f, 0.f, 0.f}, bv[3] = {0.f, 0.f, 0.f};
  if (j < M) {
    int sel = use_fps ? indices[(int64_t)n * n_points + j] : (int)((int64_t)j * N / M);  // evenly spaced: floor(j N / M)
    sel = sel < 0 ? 0 : (sel >= N ? N - 1 : sel);
    const float* k = K + (int64_t)n * 9;
    const float fx = k[0], fy = k[4], cx = k[2], cy = k[5];
    const int p = pix[(int64_t)n * HW + sel];
    const int v = p / W, u = p - v * W;
    const float zm = depth_m[(int64_t)im_ids[n] * HW + p];
#pragma unroll
    for (int c = 0; c < 3; ++c) av[c] = pts_a[((int64_t)n * HW + sel) * 3 + c];
    bv[0] = ((float)u - cx) * zm / fx; bv[1] = ((float)v - cy) * zm / fy; bv[2] = zm;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a[((int64_t)n * n_points + j) * 3 + c] = av[c];
    b[((int64_t)n * n_points + j) * 3 + c] = bv[c];
  }
}

// ---- solve ----------------------------------------------------------------------------------------------
// sum over the workgroup: stage 1 is wave_sum (every lane ends with the wave's sum), lane 0 -> part[wave]; stage 2: the 16 waves
// in turn (every thread computes the same value)
__device__ __forceinline__ double waves_sum(const double* part, int stride) {
  double s = 0.0;
  for (int w = 0; w < kWaves; ++w) s += part[w * stride];
  return s;
}

// R = argmin sum w |b - R a|^2 from Hm = sum w a b^T (row-major): Hm = U S V^T, R = V diag(1, 1, det(V U^T)) U^T.
// One-sided Jacobi: rotations V make the columns of G = Hm V orthogonal (= U S).  With u2 = +-(u0 x u1) the third term
// det(V U^T) v2 u2^T equals det(V) v2 (u0 x u1)^T whatever the sign, so a rank-2 Hm (planar or two measurements) needs no third
// left vector.  Rank below 2 leaves the rotation undetermined: identity.
__device__ __forceinline__ void rotation_from_moment(const double* Hm, double* R) {
  double G[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { G[i][j] = Hm[i * 3 + j]; V[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) { al += G[i][p] * G[i][p]; be += G[i][q] * G[i][q]; ga += G[i][p] * G[i][q]; }
        if (ga == 0.0 || fabs(ga) <= 1e-16 * sqrt(al * be)) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double gp = G[i][p], gq = G[i][q];
          G[i][p] = c * gp - s * gq; G[i][q] = s * gp + c * gq;
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  // columns by decreasing singular value (a fixed three-exchange network: no run-time indexing of G and V)
  double sg[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) sg[j] = sqrt(G[0][j] * G[0][j] + G[1][j] * G[1][j] + G[2][j] * G[2][j]);
  auto order = [&](const int p, const int q) {
    if (sg[p] < sg[q]) {
      double t = sg[p]; sg[p] = sg[q]; sg[q] = t;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        t = G[i][p]; G[i][p] = G[i][q]; G[i][q] = t;
        t = V[i][p]; V[i][p] = V[i][q]; V[i][q] = t;
      }
    }
  };
  order(0, 1); order(1, 2); order(0, 1);
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  const double s0 = sg[0], s1 = sg[1];
  if (!(s1 > 0.0) || !(s0 < INFINITY)) return;
  double u0[3], u1[3], u2[3], v0[3], v1[3], v2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    u0[i] = G[i][0] / s0; u1[i] = G[i][1] / s1;
    v0[i] = V[i][0]; v1[i] = V[i][1]; v2[i] = V[i][2];
  }
  u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
  const double detV = v0[0] * (v1[1] * v2[2] - v1[2] * v2[1]) - v0[1] * (v1[0] * v2[2] - v1[2] * v2[0]) +
                      v0[2] * (v1[0] * v2[1] - v1[1] * v2[0]);
  const double d = detV >= 0.0 ? 1.0 : -1.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = v0[i] * u0[j] + v1[i] * u1[j] + d * v2[i] * u2[j];
}

struct SolveArgs {
  const float* a;          // [n][m_stride][3]
  const float* b;
  const int32_t* m;        // [n]: number of correspondences; negative: too few masked pixels (status -1)
  const float* TCO;        // [n][16] or null: the output is T TCO (TCO itself when rejected) instead of T (identity when rejected)
  float* T_out;            // [n][16]
  int32_t* status;         // [n]
  int32_t* num_inliers;    // [n] or null
  int32_t* clique_size;    // [n] or null
  uint32_t* clique_mask;   // [n][kWords] or null
  int m_stride;
  int min_num_inliers;
  double noise_bound;
};

__global__ __launch_bounds__(kThreads) void teaser_solve_kernel(SolveArgs g) {
  // phase 1 (graph): the points as float [2][kMaxM][3] (24 KB); phase 3 (translation): x [kMaxM], interval ends [2 kMaxM] and the
  // sorted ends [2 kMaxM] as double (40 KB)
  __shared__ double sh_buf[5 * kMaxM];
  __shared__ uint32_t sh_C[kWords], sh_clq[kWords];
  __shared__ int sh_key[2][kWaves], sh_full[2][kWaves], sh_cnt;
  __shared__ uint16_t sh_member[kMaxM];  // the clique, sorted by index
  __shared__ double sh_partH[kWaves * 9], sh_partC[kWaves], sh_partX[kWaves], sh_R[9], sh_t[3];
  __shared__ int sh_parti[kWaves];
  const int n = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  const int m_in = g.m[n];
  const int M = m_in < 0 ? 0 : (m_in > kMaxM ? kMaxM : (m_in > g.m_stride ? g.m_stride : m_in));
  const float* A = g.a + (int64_t)n * g.m_stride * 3;
  const float* Bp = g.b + (int64_t)n * g.m_stride * 3;
  const double alpha = g.noise_bound * sqrt(kCbar2), beta = 2.0 * alpha, nb2 = beta * beta;

  // ---- consistency graph: thread v builds and keeps row v
  float* sa = (float*)sh_buf;
  float* sb = sa + kMaxM * 3;
  if (tid < M)
    for (int c = 0; c < 3; ++c) { sa[tid * 3 + c] = A[tid * 3 + c]; sb[tid * 3 + c] = Bp[tid * 3 + c]; }
  if (tid < kWords) {
    const int lo = tid * 32;
    sh_C[tid] = M >= lo + 32 ? 0xffffffffu : (M > lo ? (1u << (M - lo)) - 1u : 0u);  // bits at positions >= M are zero
    sh_clq[tid] = 0u;
  }
  if (tid == 0) sh_cnt = M;
  __syncthreads();
  uint32_t row[kWords];
  {
    const float betaf = (float)beta;
    const bool mine = tid < M;
    const float ax = mine ? sa[tid * 3] : 0.f, ay = mine ? sa[tid * 3 + 1] : 0.f, az = mine ? sa[tid * 3 + 2] : 0.f;
    const float bx = mine ? sb[tid * 3] : 0.f, by = mine ? sb[tid * 3 + 1] : 0.f, bz = mine ? sb[tid * 3 + 2] : 0.f;
#pragma unroll
    for (int w = 0; w < kWords; ++w) {
      uint32_t bits = 0u;
      if (mine && w * 32 < M) {  // uniform but for the last wave
        for (int jj = 0; jj < 32; ++jj) {
          const int j = w * 32 + jj;
          if (j >= M) break;
          const float dax = sa[j * 3] - ax, day = sa[j * 3 + 1] - ay, daz = sa[j * 3 + 2] - az;
          const float dbx = sb[j * 3] - bx, dby = sb[j * 3 + 1] - by, dbz = sb[j * 3 + 2] - bz;
          const float da = sqrtf(dax * dax + day * day + daz * daz), db = sqrtf(dbx * dbx + dby * dby + dbz * dbz);
          if (j != tid && fabsf(db - da) < betaf) bits |= 1u << jj;
        }
      }
      row[w] = bits;
    }
  }

  // ---- greedy clique
  int clique = 0;
  for (int step = 0; step < kMaxM; ++step) {
    const int buf = step & 1;
    const int cnt = sh_cnt;
    if (cnt == 0) break;  // uniform
    const bool inC = (sh_C[tid >> 5] >> (tid & 31)) & 1u;
    int deg = 0;
#pragma unroll
    for (int w = 0; w < kWords; ++w) deg += __popc(row[w] & sh_C[w]);
    int key = inC ? (deg << 10) | (kMaxM - 1 - tid) : -1;  // largest degree, then lowest index
    const bool full = !inC || deg == cnt - 1;
    key = wave_max(key);
    const int allfull = __all(full);
    if (lane == 0) { sh_key[buf][wave] = key; sh_full[buf][wave] = allfull; }
    __syncthreads();
    int isfull = 1;
    key = -1;
    for (int w = 0; w < kWaves; ++w) { key = sh_key[buf][w] > key ? sh_key[buf][w] : key; isfull &= sh_full[buf][w]; }
    if (isfull) {
      // the candidates are a clique among themselves: the remaining steps would append them one by one in index order
      if (tid < kWords) sh_clq[tid] |= sh_C[tid];
      clique += cnt;
      __syncthreads();
      break;
    }
    const int vstar = kMaxM - 1 - (key & (kMaxM - 1));
    if (tid == vstar) {
      int c = 0;
#pragma unroll
      for (int w = 0; w < kWords; ++w) { const uint32_t x = sh_C[w] & row[w]; sh_C[w] = x; c += __popc(x); }
      sh_cnt = c;
      sh_clq[tid >> 5] |= 1u << (tid & 31);
    }
    clique += 1;
    __syncthreads();
  }
  __syncthreads();

  int status = 0, inliers = 0;
  if (m_in < 0) status = -1;
  else if (clique < 3) status = -2;

  double Rr[9], tt[3];
  if (status == 0) {  // uniform
    // ---- the clique sorted by index; chain measurement r = member r -> member r + 1
    const bool member = (sh_clq[tid >> 5] >> (tid & 31)) & 1u;
    if (member) {
      int rank = __popc(sh_clq[tid >> 5] & ((1u << (tid & 31)) - 1u));
      for (int w = 0; w < (tid >> 5); ++w) rank += __popc(sh_clq[w]);
      sh_member[rank] = (uint16_t)tid;
    }
    __syncthreads();
    const int m = clique;
    const bool meas = tid < m - 1;
    double am[3] = {0, 0, 0}, bm[3] = {0, 0, 0};
    if (meas) {
      const int c0 = sh_member[tid], c1 = sh_member[tid + 1];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        am[c] = (double)sa[c1 * 3 + c] - (double)sa[c0 * 3 + c];
        bm[c] = (double)sb[c1 * 3 + c] - (double)sb[c0 * 3 + c];
      }
    }
    // ---- GNC-TLS rotation
    double wgt = meas ? 1.0 : 0.0, mu = 1.0, cost_prev = INFINITY;
    for (int it = 0; it < kGncMaxIterations; ++it) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double s = wave_sum(wgt * am[i] * bm[j]);
          if (lane == 0) sh_partH[wave * 9 + i * 3 + j] = s;
        }
      __syncthreads();
      if (tid == 0) {
        double Hm[9], Rn[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) Hm[e] = waves_sum(sh_partH + e, 9);
        rotation_from_moment(Hm, Rn);
#pragma unroll
        for (int e = 0; e < 9; ++e) sh_R[e] = Rn[e];
      }
      __syncthreads();
      double r2 = 0.0;
      if (meas) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double e = bm[i] - (sh_R[i * 3] * am[0] + sh_R[i * 3 + 1] * am[1] + sh_R[i * 3 + 2] * am[2]);
          r2 += e * e;
        }
      }
      const double cs = wave_sum(wgt * r2);  // the cost of the weights that produced R
      const double mx = wave_max(r2);
      if (lane == 0) { sh_partC[wave] = cs; sh_partX[wave] = mx; }
      __syncthreads();
      const double cost = waves_sum(sh_partC, 1);
      if (it == 0) {
        double rmax = 0.0;
        for (int w = 0; w < kWaves; ++w) rmax = fmax(rmax, sh_partX[w]);
        mu = 1.0 / (2.0 * rmax / nb2 - 1.0);
        if (mu <= 0.0) break;  // every measurement is an inlier
      }
      const double th1 = (mu + 1.0) / mu * nb2, th2 = mu / (mu + 1.0) * nb2;
      if (meas) wgt = r2 >= th1 ? 0.0 : (r2 <= th2 ? 1.0 : sqrt(nb2 * mu * (mu + 1.0) / r2) - mu);
      const double diff = fabs(cost - cost_prev);
      cost_prev = cost;
      mu *= kGncFactor;
      if (diff < kGncCostThreshold) break;
    }
    // sh_R holds the last rotation solved; every path to here passed the barrier after it was written
#pragma unroll
    for (int e = 0; e < 9; ++e) Rr[e] = sh_R[e];

    // ---- translation: per axis truncated least squares over the clique's members
    double xr[3] = {0, 0, 0};
    if (tid < m) {
      const int c0 = sh_member[tid];
      const double px = (double)sa[c0 * 3], py = (double)sa[c0 * 3 + 1], pz = (double)sa[c0 * 3 + 2];
#pragma unroll
      for (int i = 0; i < 3; ++i) xr[i] = (double)sb[c0 * 3 + i] - (Rr[i * 3] * px + Rr[i * 3 + 1] * py + Rr[i * 3 + 2] * pz);
    }
    __syncthreads();  // the float points in sh_buf are dead from here
    double* sx = sh_buf;
    double* ends = sh_buf + kMaxM;
    double* sorted = sh_buf + 3 * kMaxM;
    const int n_ends = 2 * m, n_cand = 2 * m - 1;
    for (int axis = 0; axis < 3; ++axis) {
      const double xa = axis == 0 ? xr[0] : (axis == 1 ? xr[1] : xr[2]);
      if (tid < m) { sx[tid] = xa; ends[2 * tid] = xa - alpha; ends[2 * tid + 1] = xa + alpha; }
      __syncthreads();
      for (int e = tid; e < n_ends; e += kThreads) {  // sort by rank, equal values in index order
        const double ve = ends[e];
        int rank = 0;
        for (int j = 0; j < n_ends; ++j) { const double vj = ends[j]; rank += (vj < ve || (vj == ve && j < e)) ? 1 : 0; }
        sorted[rank] = ve;
      }
      __syncthreads();
      double bc = INFINITY, bx = 0.0;
      int bk = 0x7fffffff;
      for (int kc = tid; kc < n_cand; kc += kThreads) {
        const double p = 0.5 * (sorted[kc] + sorted[kc + 1]);
        double s = 0.0;
        int cn = 0;
        for (int i = 0; i < m; ++i) { const double xi = sx[i]; if (fabs(xi - p) <= alpha) { s += xi; ++cn; } }
        double cst = INFINITY, xh = 0.0;
        if (cn > 0) {
          xh = s / (double)cn;
          double q = 0.0;
          for (int i = 0; i < m; ++i) { const double xi = sx[i]; if (fabs(xi - p) <= alpha) { const double e = xi - xh; q += e * e; } }
          cst = q / (alpha * alpha) + (double)(m - cn) * kCbar2;
        }
        if (cst < bc) { bc = cst; bk = kc; bx = xh; }  // increasing kc: the lowest candidate of a tie stays
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double oc = __shfl_xor(bc, off), ox = __shfl_xor(bx, off);
        const int ok = __shfl_xor(bk, off);
        if (oc < bc || (oc == bc && ok < bk)) { bc = oc; bk = ok; bx = ox; }
      }
      if (lane == 0) { sh_partC[wave] = bc; sh_partX[wave] = bx; sh_parti[wave] = bk; }
      __syncthreads();
      if (tid == 0) {
        for (int w = 1; w < kWaves; ++w)
          if (sh_partC[w] < bc || (sh_partC[w] == bc && sh_parti[w] < bk)) { bc = sh_partC[w]; bk = sh_parti[w]; bx = sh_partX[w]; }
        sh_t[axis] = bx;
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) tt[i] = sh_t[i];

    // ---- inliers over all M correspondences
    bool inl = false;
    if (tid < M) {
      double e2 = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double e = Rr[i * 3] * (double)A[tid * 3] + Rr[i * 3 + 1] * (double)A[tid * 3 + 1] + Rr[i * 3 + 2] * (double)A[tid * 3 + 2] +
                         tt[i] - (double)Bp[tid * 3 + i];
        e2 += e * e;
      }
      inl = sqrt(e2) < g.noise_bound;
    }
    const unsigned long long bal = __ballot(inl);
    if (lane == 0) sh_parti[wave] = __popcll(bal);
    __syncthreads();
    for (int w = 0; w < kWaves; ++w) inliers += sh_parti[w];
    if (inliers < g.min_num_inliers) status = -3;
  }

  // ---- result
  if (tid < 16) {
    const int i = tid >> 2, j = tid & 3;
    const float* P = g.TCO ? g.TCO + (int64_t)n * 16 : nullptr;
    float v;
    if (status != 0) v = P ? P[tid] : (i == j ? 1.f : 0.f);
    else if (i == 3) v = j == 3 ? 1.f : 0.f;
    else if (P) v = (float)(sh_R[i * 3] * (double)P[j] + sh_R[i * 3 + 1] * (double)P[4 + j] + sh_R[i * 3 + 2] * (double)P[8 + j] + (j == 3 ? sh_t[i] : 0.0));
    else v = (float)(j == 3 ? sh_t[i] : sh_R[i * 3 + j]);  // sh_R, sh_t: the accepted solution (status 0 only)
    g.T_out[(int64_t)n * 16 + tid] = v;
  }
  if (tid == 0) {
    g.status[n] = status;
    if (g.num_inliers) g.num_inliers[n] = inliers;
    if (g.clique_size) g.clique_size[n] = clique;
  }
  if (g.clique_mask && tid < kWords) g.clique_mask[(int64_t)n * kWords + tid] = sh_clq[tid];
}

constexpr int64_t kAlign = 256;

// sections of the refinement's workspace, in order
struct Workspace {
  int64_t pts_a, pix, mind, count, indices, a, b, m_sel, total;
  Workspace(int64_t n, int64_t HW, int64_t n_points) {
    int64_t o = 0;
    pts_a = o; o += round_up(n * HW * 3 * 4, kAlign);
    pix = o; o += round_up(n * HW * 4, kAlign);
    mind = o; o += round_up(n * HW * 4, kAlign);
    count = o; o += round_up(n * 4, kAlign);
    indices = o; o += round_up(n * n_points * 4, kAlign);
    a = o; o += round_up(n * n_points * 3 * 4, kAlign);
    b = o; o += round_up(n * n_points * 3 * 4, kAlign);
    m_sel = o; o += round_up(n * 4, kAlign);
    total = o;
  }
};

}  // namespace
}  // namespace hp

using namespace hp;

extern "C" int64_t hp_teaser_workspace_bytes(int n, int H, int W, int n_points) {
  if (n < 0 || H <= 0 || W <= 0 || (int64_t)H * W > (int64_t)1 << 30 || n_points < 1 || n_points > kMaxM) return -1;
  return Workspace(n, (int64_t)H * W, n_points).total;
}

extern "C" int hp_teaser_fps(int n, int n_max, const float* d_points, const int32_t* d_counts, int k, float* d_scratch,
                             int32_t* d_indices, void* stream) {
  HP_REQUIRE(n >= 0 && n_max >= 1 && k >= 1, "hp_teaser_fps: bad sizes");
  if (n == 0) return HP_OK;
  HP_REQUIRE(d_points && d_counts && d_scratch && d_indices, "hp_teaser_fps: null pointer");
  hipLaunchKernelGGL(teaser_fps_kernel, dim3(n), dim3(kThreads), 0, (hipStream_t)stream, d_points, n_max, d_counts, 0, k, d_scratch,
                     d_indices);
  return check_launch("teaser_fps_kernel");
}

extern "C" int hp_teaser_register(int n, int m_max, const float* d_a, const float* d_b, const int32_t* d_m, double noise_bound,
                                  int min_num_inliers, float* d_T, int32_t* d_status, int32_t* d_num_inliers, int32_t* d_clique_size,
                                  uint32_t* d_clique_mask, void* stream) {
  HP_REQUIRE(n >= 0 && m_max >= 1 && m_max <= kMaxM, "hp_teaser_register: bad sizes (at most 1024 correspondences)");
  HP_REQUIRE(noise_bound > 0.0, "hp_teaser_register: noise_bound must be positive");
  if (n == 0) return HP_OK;
  HP_REQUIRE(d_a && d_b && d_m && d_T && d_status, "hp_teaser_register: null pointer");
  SolveArgs g{};
  g.a = d_a; g.b = d_b; g.m = d_m; g.TCO = nullptr; g.T_out = d_T; g.status = d_status; g.num_inliers = d_num_inliers;
  g.clique_size = d_clique_size; g.clique_mask = d_clique_mask; g.m_stride = m_max; g.min_num_inliers = min_num_inliers;
  g.noise_bound = noise_bound;
  hipLaunchKernelGGL(teaser_solve_kernel, dim3(n), dim3(kThreads), 0, (hipStream_t)stream, g);
  return check_launch("teaser_solve_kernel");
}

extern "C" int hp_teaser_refine(int n, int B, int H, int W, const float* d_depth_rendered, const float* d_depth_measured,
                                const int32_t* d_im_ids, const int32_t* h_im_ids, const float* d_K, const float* d_TCO,
                                int use_threshold_mask, float depth_delta_thresh, int n_min_points, int n_points,
                                int use_farthest_point_sampling, double noise_bound, int min_num_inliers, float* d_TCO_out,
                                int32_t* d_retval, int32_t* d_num_inliers, int32_t* d_clique_size, void* d_workspace,
                                int64_t workspace_bytes, void* stream) {
  HP_REQUIRE(n >= 0 && B >= 1 && H > 0 && W > 0 && (int64_t)H * W <= (int64_t)1 << 30, "hp_teaser_refine: bad sizes");
  HP_REQUIRE(n_points >= 1 && n_points <= kMaxM, "hp_teaser_refine: n_points must be in 1 .. 1024");
  HP_REQUIRE(noise_bound > 0.0, "hp_teaser_refine: noise_bound must be positive");
  if (n == 0) return HP_OK;
  HP_REQUIRE(d_depth_rendered && d_depth_measured && d_im_ids && h_im_ids && d_K && d_TCO && d_TCO_out && d_retval,
             "hp_teaser_refine: null pointer");
  for (int i = 0; i < n; ++i) HP_REQUIRE(h_im_ids[i] >= 0 && h_im_ids[i] < B, "hp_teaser_refine: batch_im_id out of range");
  const Workspace ws(n, (int64_t)H * W, n_points);
  HP_REQUIRE(d_workspace && workspace_bytes >= ws.total,
             "hp_teaser_refine: workspace smaller than hp_teaser_workspace_bytes(n, H, W, n_points)");
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)d_workspace;
  float* pts_a = (float*)(base + ws.pts_a);
  int32_t* pix = (int32_t*)(base + ws.pix);
  float* mind = (float*)(base + ws.mind);
  int32_t* count = (int32_t*)(base + ws.count);
  int32_t* indices = (int32_t*)(base + ws.indices);
  float* a = (float*)(base + ws.a);
  float* b = (float*)(base + ws.b);
  int32_t* m_sel = (int32_t*)(base + ws.m_sel);
  int rc;
  hipLaunchKernelGGL(teaser_correspond_kernel, dim3(n), dim3(kThreads), 0, st, d_depth_rendered, d_depth_measured, d_im_ids, d_K, H, W,
                     use_threshold_mask, depth_delta_thresh, pts_a, pix, count);
  if ((rc = check_launch("teaser_correspond_kernel"))) return rc;
  if (use_farthest_point_sampling) {
    hipLaunchKernelGGL(teaser_fps_kernel, dim3(n), dim3(kThreads), 0, st, pts_a, H * W, count, n_min_points, n_points, mind, indices);
    if ((rc = check_launch("teaser_fps_kernel"))) return rc;
  }
  hipLaunchKernelGGL(teaser_gather_kernel, dim3(n), dim3(kThreads), 0, st, pts_a, pix, count, indices, d_depth_measured, d_im_ids, d_K, H,
                     W, n_min_points, n_points, use_farthest_point_sampling, a, b, m_sel);
  if ((rc = check_launch("teaser_gather_kernel"))) return rc;
  SolveArgs g{};
  g.a = a; g.b = b; g.m = m_sel; g.TCO = d_TCO; g.T_out = d_TCO_out; g.status = d_retval; g.num_inliers = d_num_inliers;
  g.clique_size = d_clique_size; g.clique_mask = nullptr; g.m_stride = n_points; g.min_num_inliers = min_num_inliers;
  g.noise_bound = noise_bound;
  hipLaunchKernelGGL(teaser_solve_kernel, dim3(n), dim3(kThreads), 0, st, g);
  return check_launch("teaser_solve_kernel");
}
