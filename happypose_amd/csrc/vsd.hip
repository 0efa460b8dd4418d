// BOP's visible-surface discrepancy (VSD, BOP19 visibility rule, `step` cost): entry points and the definition are in
// include/happypose_amd.h (hp_vsd).
//
// A row is (estimate layer, ground-truth layer, frame, diameter), gathered through int32 / float32 columns.  Two kernels:
//   vsd_kernel     a workgroup is one (row, chunk of kChunk pixels of the flattened H x W plane).  One pass: a thread owns 4
//                  consecutive pixels per step (16-byte loads of the three depth planes when H * W is a multiple of 4 and the
//                  buffers are 16-byte aligned; the scalar instantiation covers everything else, tail included), computes the
//                  ray factor f(u, v) once per pixel, applies it to the three depths and evaluates the visibility rule and all
//                  n_tau comparisons from registers.  Everything it accumulates is an integer count: 4 + n_tau counters per
//                  thread, an integer butterfly in the wavefront, one LDS step across the wavefronts, and ONE record of
//                  kFields int32 per workgroup in d_workspace.
//   finish_kernel  one wavefront per row adds the row's records in chunk order and writes counts, cost and errors.
// No atomics, no float accumulation: the outputs are a function of the row alone, bit-identical from run to run and whatever the
// grid looks like.
// The grid is (row, chunk) with the ROW in x: workgroups that are dispatched together work on the same chunk of neighbouring
// rows, which in an evaluation share the frame and mostly the ground-truth layer -- those two of a row's three reads are then
// served from the L2 of the XCD instead of from memory.
#include "common.h"
#include "wave.h"

namespace hp {
namespace {

constexpr int kThreads = 256;
constexpr int kVec = 4;                                  // pixels per thread per step
constexpr int kSteps = 4;                                // steps per workgroup: 12 independent 16-byte loads per thread
constexpr int kChunk = kThreads * kVec * kSteps;         // 4096 pixels: 640 x 480 is 75 workgroups per row
constexpr int kMaxTaus = HP_VSD_MAX_TAUS;
constexpr int kCounts = HP_VSD_COUNT_FIELDS;             // n_U, n_I, |V_e|, |V_g|
constexpr int kFields = kCounts + kMaxTaus;              // one workspace record
static_assert(kFields <= kWave, "finish_kernel: one lane per field");

struct Params {
  const float* depth_test;    // [n_frames][P]
  const float* depth_layers;  // [n_layers][P]
  const float* K;             // [n_frames][9]
  const int32_t* est_layer;
  const int32_t* gt_layer;
  const int32_t* frame;
  const float* diameter;
  int n_frames, n_layers, n_rows, w, n_tau, normalized;
  int64_t P;
  float delta;
  float taus[kMaxTaus];
};

// a row whose ids leave their tables reads nothing and is answered with -1 / NaN by finish_kernel
__device__ inline bool load_row(const Params& p, int row, int& e, int& g, int& f) {
  e = p.est_layer[row];
  g = p.gt_layer[row];
  f = p.frame[row];
  return (unsigned)e < (unsigned)p.n_layers && (unsigned)g < (unsigned)p.n_layers && (unsigned)f < (unsigned)p.n_frames;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) vsd_kernel(Params p, int32_t* __restrict__ partials) {
  __shared__ int s_red[kThreads / kWave][kFields];
  const int row = blockIdx.x, chunk = blockIdx.y;
  int le, lg, fr;
  if (!load_row(p, row, le, lg, fr)) return;  // uniform over the workgroup
  const float* __restrict__ dt_p = p.depth_test + (int64_t)fr * p.P;
  const float* __restrict__ de_p = p.depth_layers + (int64_t)le * p.P;
  const float* __restrict__ dg_p = p.depth_layers + (int64_t)lg * p.P;
  const float* Kf = p.K + 9 * (int64_t)fr;
  const float fx = Kf[0], cx = Kf[2], fy = Kf[4], cy = Kf[5];
  const float diam = p.normalized ? p.diameter[row] : 1.f;
  const float delta = p.delta;
  const int w = p.w;

  int cnt[kCounts] = {0, 0, 0, 0};
  int cost[kMaxTaus];
#pragma unroll
  for (int t = 0; t < kMaxTaus; ++t) cost[t] = 0;

  const int64_t base = (int64_t)chunk * kChunk + (int64_t)threadIdx.x * kVec;
  float vt[kSteps][kVec], ve[kSteps][kVec], vg[kSteps][kVec];
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {  // every load of the workgroup is issued before the first use
    const int64_t p0 = base + (int64_t)s * kThreads * kVec;
    if (VEC) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
      if (p0 < p.P) {  // P % 4 == 0: a group is inside or outside as a whole
        a = *reinterpret_cast<const float4*>(dt_p + p0);
        b = *reinterpret_cast<const float4*>(de_p + p0);
        c = *reinterpret_cast<const float4*>(dg_p + p0);
      }
      vt[s][0] = a.x, vt[s][1] = a.y, vt[s][2] = a.z, vt[s][3] = a.w;
      ve[s][0] = b.x, ve[s][1] = b.y, ve[s][2] = b.z, ve[s][3] = b.w;
      vg[s][0] = c.x, vg[s][1] = c.y, vg[s][2] = c.z, vg[s][3] = c.w;
    } else {
#pragma unroll
      for (int i = 0; i < kVec; ++i) {
        const bool in = p0 + i < p.P;  // a pixel past the end has both layers empty: it counts nowhere
        vt[s][i] = in ? dt_p[p0 + i] : 0.f;
        ve[s][i] = in ? de_p[p0 + i] : 0.f;
        vg[s][i] = in ? dg_p[p0 + i] : 0.f;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int64_t p0 = base + (int64_t)s * kThreads * kVec;
    bool any = false;
#pragma unroll
    for (int i = 0; i < kVec; ++i) any = any || ve[s][i] > 0.f || vg[s][i] > 0.f;
    if (!any) continue;  // background in both renders (most of a frame): S_e = S_g = 0, no set holds the pixel
    int v = (int)((uint32_t)p0 / (uint32_t)w), u = (int)((uint32_t)p0 - (uint32_t)v * (uint32_t)w);  // p0 < P < 2^31 here
#pragma unroll
    for (int i = 0; i < kVec; ++i) {
      while (u >= w) {  // a group may cross the end of an image row (several, when w < 4)
        u -= w;
        ++v;
      }
      const float xs = ((float)u - cx) / fx, ys = ((float)v - cy) / fy;
      const float f = sqrtf(fmaf(xs, xs, fmaf(ys, ys, 1.f)));
      const float st = vt[s][i] * f, se = ve[s][i] * f, sg = vg[s][i] * f;
      const bool free_t = st == 0.f;  // no measurement: visible by the BOP19 rule
      const bool vis_g = sg > 0.f && (sg - st <= delta || free_t);
      const bool vis_e = (se > 0.f && (se - st <= delta || free_t)) || (vis_g && se > 0.f);
      const bool both = vis_g && vis_e;
      cnt[0] += (vis_g || vis_e) ? 1 : 0;
      cnt[1] += both ? 1 : 0;
      cnt[2] += vis_e ? 1 : 0;
      cnt[3] += vis_g ? 1 : 0;
      const float q = fabsf(sg - se) / diam;
#pragma unroll
      for (int t = 0; t < kMaxTaus; ++t) cost[t] += (t < p.n_tau && both && q >= p.taus[t]) ? 1 : 0;
      ++u;
    }
  }

  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < kCounts; ++k) {
    const int r = wave_sum(cnt[k]);
    if (lane == 0) s_red[wave][k] = r;
  }
#pragma unroll
  for (int t = 0; t < kMaxTaus; ++t) {
    const int r = t < p.n_tau ? wave_sum(cost[t]) : 0;  // n_tau is uniform
    if (lane == 0) s_red[wave][kCounts + t] = r;
  }
  __syncthreads();
  if (threadIdx.x < kFields) {
    int r = 0;
#pragma unroll
    for (int wv = 0; wv < kThreads / kWave; ++wv) r += s_red[wv][threadIdx.x];
    partials[((int64_t)row * gridDim.y + chunk) * kFields + threadIdx.x] = r;
  }
}

__global__ void __launch_bounds__(kWave) finish_kernel(Params p, int n_chunks, const int32_t* __restrict__ partials,
                                                       int32_t* __restrict__ counts, int32_t* __restrict__ cost,
                                                       float* __restrict__ errors) {
  const int row = blockIdx.x, k = threadIdx.x;
  int le, lg, fr;
  const bool ok = load_row(p, row, le, lg, fr);
  int sum = 0;
  if (ok && k < kFields)
    for (int c = 0; c < n_chunks; ++c) sum += partials[((int64_t)row * n_chunks + c) * kFields + k];  // chunk order
  const int n_u = __shfl(sum, 0, kWave), n_i = __shfl(sum, 1, kWave);
  if (k < kCounts) counts[(int64_t)row * kCounts + k] = ok ? sum : -1;
  const int t = k - kCounts;
  if (t >= 0 && t < p.n_tau) {
    cost[(int64_t)row * p.n_tau + t] = ok ? sum : -1;
    // integers in double, one division, one rounding to float: (c + n_U - n_I) / n_U to one float32 rounding for any frame size
    const float e = !ok ? NAN : (n_u == 0 ? 1.f : (float)(((double)sum + (double)n_u - (double)n_i) / (double)n_u));
    errors[(int64_t)row * p.n_tau + t] = e;
  }
}


inline int64_t chunks_of(int64_t P) { return (P + kChunk - 1) / kChunk; }

}  // namespace
}  // namespace hp

using namespace hp;

extern "C" int64_t hp_vsd_workspace_bytes(int n_rows, int h, int w) {
  if (n_rows < 0 || h < 1 || w < 1 || (int64_t)h * w >= (int64_t(1) << 31)) return -1;
  return (int64_t)n_rows * chunks_of((int64_t)h * w) * kFields * (int64_t)sizeof(int32_t);
}

extern "C" int hp_vsd(int n_rows, const int32_t* d_est_layer, const int32_t* d_gt_layer, const int32_t* d_frame,
                      const float* d_diameter, const float* d_depth_test, int n_frames, const float* d_depth_layers, int n_layers,
                      const float* d_K, int h, int w, float delta, int n_tau, const float* taus, int normalized_by_diameter,
                      int32_t* d_counts, int32_t* d_cost, float* d_errors, void* d_workspace, int64_t workspace_bytes,
                      void* stream) {
  HP_REQUIRE(n_rows >= 0 && n_frames >= 0 && n_layers >= 0, "hp_vsd: negative size");
  HP_REQUIRE(h >= 1 && w >= 1, "hp_vsd: h and w must be positive");
  HP_REQUIRE((int64_t)h * w < (int64_t(1) << 31), "hp_vsd: frame of 2^31 pixels or more");
  HP_REQUIRE(n_tau >= 1 && n_tau <= kMaxTaus && taus, "hp_vsd: n_tau outside 1..16 or taus missing");
  if (n_rows == 0) return HP_OK;
  HP_REQUIRE(d_est_layer && d_gt_layer && d_frame && d_depth_test && d_depth_layers && d_K && d_counts && d_cost && d_errors,
             "hp_vsd: null pointer");
  HP_REQUIRE(!normalized_by_diameter || d_diameter, "hp_vsd: normalized_by_diameter needs d_diameter");
  const int64_t P = (int64_t)h * w;
  const int64_t chunks = chunks_of(P);
  HP_REQUIRE(chunks <= 65535, "hp_vsd: frame too large for one launch");
  HP_REQUIRE((int64_t)n_rows * n_tau < (int64_t(1) << 31) && (int64_t)n_rows * chunks * kFields < (int64_t(1) << 31),
             "hp_vsd: tables of 2^31 entries or more");
  HP_REQUIRE(d_workspace && workspace_bytes >= hp_vsd_workspace_bytes(n_rows, h, w),
             "hp_vsd: workspace smaller than hp_vsd_workspace_bytes(n_rows, h, w)");
  Params p;
  p.depth_test = d_depth_test, p.depth_layers = d_depth_layers, p.K = d_K;
  p.est_layer = d_est_layer, p.gt_layer = d_gt_layer, p.frame = d_frame, p.diameter = d_diameter;
  p.n_frames = n_frames, p.n_layers = n_layers, p.n_rows = n_rows, p.w = w, p.n_tau = n_tau;
  p.normalized = normalized_by_diameter ? 1 : 0;
  p.P = P;
  p.delta = delta;
  for (int t = 0; t < kMaxTaus; ++t) p.taus[t] = t < n_tau ? taus[t] : INFINITY;
  hipStream_t st = (hipStream_t)stream;
  int32_t* partials = (int32_t*)d_workspace;
  const dim3 grid((unsigned)n_rows, (unsigned)chunks);
  if (P % 4 == 0 && aligned(d_depth_test, 16) && aligned(d_depth_layers, 16))
    hipLaunchKernelGGL(vsd_kernel<true>, grid, dim3(kThreads), 0, st, p, partials);
  else
    hipLaunchKernelGGL(vsd_kernel<false>, grid, dim3(kThreads), 0, st, p, partials);
  if (int rc = check_launch("hp_vsd (pixels)")) return rc;
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)n_rows), dim3(kWave), 0, st, p, (int)chunks, (const int32_t*)partials, d_counts,
                     d_cost, d_errors);
  return check_launch("hp_vsd (rows)");
}
