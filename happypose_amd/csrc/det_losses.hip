// The detector's training targets and losses (torchvision 0.14's train-mode MaskRCNN.forward without the networks): entry points
// and definitions are in include/happypose_amd.h (hp_det_assign, hp_det_sample_keys, hp_det_box_encode, hp_det_mask_targets,
// hp_loss_rpn, hp_loss_fastrcnn, hp_loss_mask).
//
//   gt_max_kernel      a workgroup is one (ground truth, chunk of kChunk boxes): IoU of the boxes of the ground truth's image,
//                      maximum over lane, wavefront (shuffle) and LDS, one partial per workgroup in the workspace.
//   gt_finish_kernel   a thread per ground truth: maximum over its partials.  A maximum does not depend on the order.
//   assign_kernel      a thread per box: the first maximum over the ground truths of its image, the thresholds, and the
//                      low-quality restore by float equality with the ground truth's maximum.  Both passes call box_iou().
//   keys_kernel        a thread per row: one Philox4x32-10 call, word 0.
//   encode_kernel      a thread per row.
//   mask_targets_kernel a workgroup per roi, threads strided over the M x M bins.
//   rpn / fastrcnn / mask loss kernels: every term and its gradient are evaluated in double from the float32 inputs, summed per
//                      lane in row order, over the wavefront by xor butterflies, over the wavefronts in LDS in wavefront order; one
//                      partial per workgroup goes to the workspace and sum_kernel (one workgroup) adds the partials in a fixed
//                      order.  No atomics: two calls give the same bits, and a row's gradient is a function of the row alone.
#include "common.h"
#include "philox.h"
#include "wave.h"

namespace hp {
namespace {

#pragma clang fp contract(off)  // box_iou is compiled into two kernels whose results are compared for equality

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kChunk = 4096;  // boxes per workgroup of gt_max_kernel
constexpr double kBeta = 1.0 / 9.0;

// torchvision.ops.boxes.box_iou for one pair, float32, in its order: areas, lt / rb, clamped wh, inter / (a1 + a2 - inter)
__device__ inline float box_iou(const float* g, const float* b) {
  const float a1 = (g[2] - g[0]) * (g[3] - g[1]);
  const float a2 = (b[2] - b[0]) * (b[3] - b[1]);
  const float ltx = fmaxf(g[0], b[0]), lty = fmaxf(g[1], b[1]);
  const float rbx = fminf(g[2], b[2]), rby = fminf(g[3], b[3]);
  const float w = fmaxf(rbx - ltx, 0.f), h = fmaxf(rby - lty, 0.f);
  const float inter = w * h;
  return inter / ((a1 + a2) - inter);
}

__device__ inline int image_of_gt(const int32_t* __restrict__ gt_off, int n_images, int g) {
  int im = 0;
  while (im + 1 < n_images && g >= gt_off[im + 1]) ++im;
  return im;
}

__global__ void __launch_bounds__(kThreads) gt_max_kernel(int n, const float* __restrict__ boxes, const int32_t* __restrict__ image_of,
                                                          int n_images, const float* __restrict__ gt, const int32_t* __restrict__ gt_off,
                                                          int n_chunks, float* __restrict__ partial) {
  __shared__ float s_red[kWaves];
  const int g = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int im = image_of_gt(gt_off, n_images, g);
  float gb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) gb[k] = gt[4 * (int64_t)g + k];
  float best = -1.f;  // below every IoU; NaN never wins
  const int64_t end = min((int64_t)n, ((int64_t)chunk + 1) * kChunk);
  for (int64_t i = (int64_t)chunk * kChunk + tid; i < end; i += kThreads) {
    if (image_of[i] != im) continue;
    const float v = box_iou(gb, boxes + 4 * i);
    if (v > best) best = v;
  }
  best = wave_max(best);
  if (tid % kWave == 0) s_red[tid / kWave] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) best = fmaxf(best, s_red[w]);
    partial[(int64_t)g * n_chunks + chunk] = best;
  }
}

__global__ void __launch_bounds__(kWave) gt_finish_kernel(int n_gt, int n_chunks, const float* __restrict__ partial, float* __restrict__ gt_max) {
  const int g = blockIdx.x * kWave + threadIdx.x;
  if (g >= n_gt) return;
  float best = -1.f;
  for (int c = 0; c < n_chunks; ++c) best = fmaxf(best, partial[(int64_t)g * n_chunks + c]);
  gt_max[g] = best;
}

__global__ void __launch_bounds__(kThreads) assign_kernel(int n, const float* __restrict__ boxes, const int32_t* __restrict__ image_of,
                                                          int n_images, const float* __restrict__ gt, const int32_t* __restrict__ gt_off,
                                                          int n_gt, float high, float low, int allow_low_quality,
                                                          const float* __restrict__ gt_max, int32_t* __restrict__ match,
                                                          float* __restrict__ iou) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int im = image_of[i];
  int g0 = 0, g1 = 0;
  if ((unsigned)im < (unsigned)n_images) {
    g0 = max(gt_off[im], 0), g1 = min(gt_off[im + 1], n_gt);
  }
  if (g1 <= g0) {  // an image without ground truths (or an image id outside the batch): background
    match[i] = -1;
    iou[i] = 0.f;
    return;
  }
  float b[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) b[k] = boxes[4 * i + k];
  float best = box_iou(gt + 4 * (int64_t)g0, b);
  int arg = g0;
  bool restore = allow_low_quality && best == gt_max[g0];
  for (int g = g0 + 1; g < g1; ++g) {
    const float v = box_iou(gt + 4 * (int64_t)g, b);
    if (v > best) best = v, arg = g;  // strict: the first maximum in ground-truth order
    restore |= allow_low_quality && v == gt_max[g];
  }
  int m = arg;
  if (best < low) m = -1;
  else if (best < high) m = -2;
  if (restore) m = arg;
  match[i] = m;
  iou[i] = best;
}

// ---- one Philox4x32-10 call (philox.h), counter (index in image, image, stream, 0), word 0 --------------------------------------------
__global__ void __launch_bounds__(kThreads) keys_kernel(int n, const int32_t* __restrict__ index_in_image, const int32_t* __restrict__ image_of,
                                                        uint32_t stream_id, uint32_t k0, uint32_t k1, uint32_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  uint32_t c[4] = {(uint32_t)index_in_image[i], (uint32_t)image_of[i], stream_id, 0u};
  philox4x32_10(c, k0, k1);
  keys[i] = c[0];
}

// ---- BoxCoder.encode_single ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) encode_kernel(int n, const float* __restrict__ boxes, const int32_t* __restrict__ match,
                                                          const float* __restrict__ gt, int n_gt, float wx, float wy, float ww, float wh,
                                                          float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int m = match[i];
  float g[4] = {0.f, 0.f, 0.f, 0.f};
  if ((unsigned)m < (unsigned)n_gt) {
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = gt[4 * (int64_t)m + k];
  }
  const float px1 = boxes[4 * i], py1 = boxes[4 * i + 1], px2 = boxes[4 * i + 2], py2 = boxes[4 * i + 3];
  const float ex_w = px2 - px1, ex_h = py2 - py1;
  const float ex_cx = px1 + 0.5f * ex_w, ex_cy = py1 + 0.5f * ex_h;
  const float gt_w = g[2] - g[0], gt_h = g[3] - g[1];
  const float gt_cx = g[0] + 0.5f * gt_w, gt_cy = g[1] + 0.5f * gt_h;
  out[4 * i] = wx * (gt_cx - ex_cx) / ex_w;
  out[4 * i + 1] = wy * (gt_cy - ex_cy) / ex_h;
  out[4 * i + 2] = ww * logf(gt_w / ex_w);
  out[4 * i + 3] = wh * logf(gt_h / ex_h);
}

// ---- project_masks_on_boxes: torchvision's roi_align, aligned = False, sampling_ratio = -1, spatial_scale = 1 ------------------------
__device__ inline float bilinear_u8(const uint8_t* __restrict__ m, int H, int W, float y, float x) {
  if (!(y >= -1.0f && y <= (float)H && x >= -1.0f && x <= (float)W)) return 0.f;  // NaN coordinates land here too
  if (y <= 0.f) y = 0.f;
  if (x <= 0.f) x = 0.f;
  int y_low = (int)y, x_low = (int)x, y_high, x_high;
  if (y_low >= H - 1) {
    y_high = y_low = H - 1;
    y = (float)y_low;
  } else {
    y_high = y_low + 1;
  }
  if (x_low >= W - 1) {
    x_high = x_low = W - 1;
    x = (float)x_low;
  } else {
    x_high = x_low + 1;
  }
  const float ly = y - (float)y_low, lx = x - (float)x_low, hy = 1.f - ly, hx = 1.f - lx;
  const float v1 = m[(int64_t)y_low * W + x_low], v2 = m[(int64_t)y_low * W + x_high];
  const float v3 = m[(int64_t)y_high * W + x_low], v4 = m[(int64_t)y_high * W + x_high];
  const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
  return w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
}

__global__ void __launch_bounds__(kThreads) mask_targets_kernel(const uint8_t* __restrict__ masks, int n_gt, int H, int W,
                                                                const int32_t* __restrict__ match, const float* __restrict__ rois, int M,
                                                                int max_grid, float* __restrict__ out) {
  const int64_t r = blockIdx.x;
  const int m = match[r];
  float* __restrict__ dst = out + r * M * M;
  const float x1 = rois[4 * r], y1 = rois[4 * r + 1], x2 = rois[4 * r + 2], y2 = rois[4 * r + 3];
  const float roi_w = fmaxf(x2 - x1, 1.f), roi_h = fmaxf(y2 - y1, 1.f);
  const float gh_f = ceilf(roi_h / (float)M), gw_f = ceilf(roi_w / (float)M);
  // an id outside the table, a non-finite roi or a sampling grid beyond the frame's own (a roi many times the frame): NaN
  const bool bad = (unsigned)m >= (unsigned)n_gt || !(gh_f >= 1.f && gh_f <= (float)max_grid) || !(gw_f >= 1.f && gw_f <= (float)max_grid) ||
                   !isfinite(x1) || !isfinite(y1);
  if (bad) {  // uniform over the workgroup
    for (int p = threadIdx.x; p < M * M; p += kThreads) dst[p] = __builtin_nanf("");
    return;
  }
  const uint8_t* __restrict__ src = masks + (int64_t)m * H * W;
  const int gh = (int)gh_f, gw = (int)gw_f;
  const float bin_h = roi_h / (float)M, bin_w = roi_w / (float)M;
  const float count = (float)max(gh * gw, 1);
  for (int p = threadIdx.x; p < M * M; p += kThreads) {
    const int ph = p / M, pw = p % M;
    float acc = 0.f;
    for (int iy = 0; iy < gh; ++iy) {
      const float y = y1 + (float)ph * bin_h + ((float)iy + .5f) * bin_h / (float)gh;
      for (int ix = 0; ix < gw; ++ix) {
        const float x = x1 + (float)pw * bin_w + ((float)ix + .5f) * bin_w / (float)gw;
        acc += bilinear_u8(src, H, W, y, x);
      }
    }
    dst[p] = acc / count;
  }
}

// ---- sums ---------------------------------------------------------------------------------------------------------------------------
// the workgroup's sums of NS values, valid in thread 0: lane, wavefront butterfly, LDS in wavefront order
template <int NS>
__device__ inline void block_sums(double v[NS], double (*s_red)[NS]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const double s = wave_sum(v[k]);
    if (tid % kWave == 0) s_red[tid / kWave][k] = s;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      double s = s_red[0][k];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) s += s_red[w][k];
      v[k] = s;
    }
  }
}

// partial [n_part][NS] -> out[k] = (float)(sum_p partial[p][k] * scale[k]): one workgroup, thread t adds partials t, t + 256, ...
template <int NS>
__global__ void __launch_bounds__(kThreads) sum_kernel(int n_part, const double* __restrict__ partial, double scale0, double scale1,
                                                       float* __restrict__ out) {
  __shared__ double s_red[kWaves][NS];
  double v[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) v[k] = 0.0;
  for (int p = threadIdx.x; p < n_part; p += kThreads)
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] += partial[(int64_t)p * NS + k];
  block_sums<NS>(v, s_red);
  if (threadIdx.x == 0) {
    out[0] = (float)(v[0] * scale0);
    if (NS > 1) out[NS - 1] = (float)(v[NS - 1] * scale1);
  }
}

// binary_cross_entropy_with_logits for one element and its derivative: max(x, 0) - x y + log1p(exp(-|x|)), sigmoid(x) - y
__device__ inline void bce(double x, double y, double& loss, double& grad) {
  const double e = exp(-fabs(x));
  loss = (fmax(x, 0.0) - x * y) + log1p(e);
  const double sig = x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
  grad = sig - y;
  if (!isfinite(x) || !isfinite(y)) loss = grad = __builtin_nan("");
}

// smooth_l1_loss(beta) for one element and its derivative
__device__ inline void smooth_l1(double d, double& loss, double& grad) {
  const double a = fabs(d);
  if (a < kBeta) {
    loss = 0.5 * d * d / kBeta;
    grad = d / kBeta;
  } else {
    loss = a - 0.5 * kBeta;
    grad = d > 0.0 ? 1.0 : -1.0;
  }
  if (!isfinite(d)) loss = grad = __builtin_nan("");
}

__global__ void __launch_bounds__(kThreads) rpn_loss_kernel(int n_anchors, int n_sampled, const int32_t* __restrict__ sampled,
                                                            const float* __restrict__ objectness, const float* __restrict__ deltas,
                                                            const int32_t* __restrict__ labels, const float* __restrict__ targets,
                                                            double inv_n, double* __restrict__ partial, float* __restrict__ grad_obj,
                                                            float* __restrict__ grad_deltas) {
  __shared__ double s_red[kWaves][2];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  double v[2] = {0.0, 0.0};
  if (i < n_sampled) {
    const int64_t a = sampled[i];
    if ((uint64_t)a < (uint64_t)n_anchors) {
      const int lab = labels[a];
      double l, g;
      bce((double)objectness[a], lab >= 1 ? 1.0 : 0.0, l, g);
      v[0] = l;
      grad_obj[a] = (float)(g * inv_n);
      if (lab >= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          smooth_l1((double)deltas[4 * a + k] - (double)targets[4 * a + k], l, g);
          v[1] += l;
          grad_deltas[4 * a + k] = (float)(g * inv_n);
        }
      }
    } else {
      v[0] = v[1] = __builtin_nan("");  // an id outside the table: nothing is read or written
    }
  }
  block_sums<2>(v, s_red);
  if (threadIdx.x == 0) partial[2 * (int64_t)blockIdx.x] = v[0], partial[2 * (int64_t)blockIdx.x + 1] = v[1];
}

__global__ void __launch_bounds__(kThreads) fastrcnn_loss_kernel(int n, int C, int ld, int ld_reg, const float* __restrict__ logits,
                                                                 const float* __restrict__ box_reg, const int32_t* __restrict__ labels,
                                                                 const float* __restrict__ targets, double inv_n,
                                                                 double* __restrict__ partial, float* __restrict__ grad_logits,
                                                                 float* __restrict__ grad_reg) {
  __shared__ double s_red[kWaves][2];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  double v[2] = {0.0, 0.0};
  if (i < n) {
    const float* __restrict__ x = logits + i * ld;
    float* __restrict__ gx = grad_logits + i * ld;
    float* __restrict__ gr = grad_reg + i * ld_reg;
    const int lab = labels[i];
    const bool bad_label = (unsigned)lab >= (unsigned)C;
    float mx = x[0];
    bool finite = isfinite(x[0]);
    for (int c = 1; c < C; ++c) {
      mx = fmaxf(mx, x[c]);
      finite &= isfinite(x[c]);
    }
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += exp((double)x[c] - (double)mx);
    const double lse = log(s);
    const bool bad = bad_label || !finite;
    v[0] = bad ? __builtin_nan("") : lse - ((double)x[lab] - (double)mx);
    for (int c = 0; c < C; ++c) {
      const double p = exp((double)x[c] - (double)mx) / s;
      gx[c] = bad ? __builtin_nanf("") : (float)((p - (c == lab ? 1.0 : 0.0)) * inv_n);
    }
    for (int c = C; c < ld; ++c) gx[c] = 0.f;
    for (int c = 0; c < ld_reg; ++c) gr[c] = 0.f;
    if (!bad_label && lab > 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        double l, g;
        smooth_l1((double)box_reg[i * ld_reg + 4 * lab + k] - (double)targets[4 * i + k], l, g);
        v[1] += l;
        gr[4 * lab + k] = (float)(g * inv_n);
      }
    }
  }
  block_sums<2>(v, s_red);
  if (threadIdx.x == 0) partial[2 * (int64_t)blockIdx.x] = v[0], partial[2 * (int64_t)blockIdx.x + 1] = v[1];
}

__global__ void __launch_bounds__(kThreads) mask_loss_kernel(int C, int P, const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                             const float* __restrict__ targets, double inv_n, double* __restrict__ partial,
                                                             float* __restrict__ grad) {
  __shared__ double s_red[kWaves][1];
  const int64_t r = blockIdx.x;
  const int lab = labels[r];
  const bool bad_label = (unsigned)lab >= (unsigned)C;  // uniform over the workgroup
  double v[1] = {0.0};
  for (int c = 0; c < C; ++c) {
    if (c == lab) continue;
    float* __restrict__ g0 = grad + (r * C + c) * P;
    for (int p = threadIdx.x; p < P; p += kThreads) g0[p] = 0.f;
  }
  if (bad_label) {
    v[0] = __builtin_nan("");
  } else {
    const float* __restrict__ x = logits + (r * C + lab) * P;
    const float* __restrict__ t = targets + r * P;
    float* __restrict__ g = grad + (r * C + lab) * P;
    for (int p = threadIdx.x; p < P; p += kThreads) {
      double l, d;
      bce((double)x[p], (double)t[p], l, d);
      v[0] += l;
      g[p] = (float)(d * inv_n);
    }
  }
  block_sums<1>(v, s_red);
  if (threadIdx.x == 0) partial[r] = v[0];
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace
}  // namespace hp

using namespace hp;

extern "C" int64_t hp_det_assign_workspace_bytes(int n, int n_gt) {
  if (n < 0 || n_gt < 0) return -1;
  const int64_t chunks = ((int64_t)n + kChunk - 1) / kChunk;
  return round_up(((int64_t)n_gt * chunks + n_gt) * (int64_t)sizeof(float), 8);
}

extern "C" int hp_det_assign(int n, const float* d_boxes, const int32_t* d_image_of, int n_images, const float* d_gt, int n_gt,
                             const int32_t* d_gt_off, float high, float low, int allow_low_quality, int32_t* d_match, float* d_iou,
                             void* d_workspace, int64_t workspace_bytes, void* stream) {
  HP_REQUIRE(n >= 0 && n_gt >= 0 && n_images >= 0, "hp_det_assign: negative count");
  if (n == 0) return HP_OK;
  HP_REQUIRE(n_images >= 1 && n_gt <= 65535, "hp_det_assign: no image, or more than 65535 ground truths");
  HP_REQUIRE(low <= high, "hp_det_assign: low threshold above high (or NaN)");
  HP_REQUIRE(d_boxes && d_image_of && d_gt_off && d_match && d_iou && (n_gt == 0 || d_gt), "hp_det_assign: null pointer");
  HP_REQUIRE(n_gt == 0 || (d_workspace && workspace_bytes >= hp_det_assign_workspace_bytes(n, n_gt)),
             "hp_det_assign: workspace smaller than hp_det_assign_workspace_bytes(n, n_gt)");
  hipStream_t st = (hipStream_t)stream;
  const int chunks = (int)(((int64_t)n + kChunk - 1) / kChunk);
  float* partial = (float*)d_workspace;
  float* gt_max = partial ? partial + (int64_t)n_gt * chunks : nullptr;
  if (n_gt > 0) {
    hipLaunchKernelGGL(gt_max_kernel, dim3(chunks, n_gt), dim3(kThreads), 0, st, n, d_boxes, d_image_of, n_images, d_gt, d_gt_off, chunks,
                       partial);
    if (int rc = check_launch("hp_det_assign")) return rc;
    hipLaunchKernelGGL(gt_finish_kernel, dim3((n_gt + kWave - 1) / kWave), dim3(kWave), 0, st, n_gt, chunks, (const float*)partial, gt_max);
    if (int rc = check_launch("hp_det_assign")) return rc;
  }
  hipLaunchKernelGGL(assign_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, st, n, d_boxes, d_image_of, n_images, d_gt, d_gt_off, n_gt, high,
                     low, allow_low_quality, (const float*)gt_max, d_match, d_iou);
  return check_launch("hp_det_assign");
}

extern "C" int hp_det_sample_keys(int n, const int32_t* d_index_in_image, const int32_t* d_image_of, uint32_t stream_id, uint64_t seed,
                                  uint32_t* d_keys, void* stream) {
  HP_REQUIRE(n >= 0, "hp_det_sample_keys: negative count");
  if (n == 0) return HP_OK;
  HP_REQUIRE(d_index_in_image && d_image_of && d_keys, "hp_det_sample_keys: null pointer");
  hipLaunchKernelGGL(keys_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, (hipStream_t)stream, n, d_index_in_image, d_image_of, stream_id,
                     (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), d_keys);
  return check_launch("hp_det_sample_keys");
}

extern "C" int hp_det_box_encode(int n, const float* d_boxes, const int32_t* d_match, const float* d_gt, int n_gt, float wx, float wy,
                                 float ww, float wh, float* d_out, void* stream) {
  HP_REQUIRE(n >= 0 && n_gt >= 0, "hp_det_box_encode: negative count");
  if (n == 0) return HP_OK;
  HP_REQUIRE(d_boxes && d_match && d_out && (n_gt == 0 || d_gt), "hp_det_box_encode: null pointer");
  hipLaunchKernelGGL(encode_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, (hipStream_t)stream, n, d_boxes, d_match, d_gt, n_gt, wx, wy, ww, wh,
                     d_out);
  return check_launch("hp_det_box_encode");
}

extern "C" int hp_det_mask_targets(int n, const uint8_t* d_masks, int n_gt, int h, int w, const int32_t* d_match, const float* d_rois, int m,
                                   float* d_out, void* stream) {
  HP_REQUIRE(n >= 0, "hp_det_mask_targets: negative count");
  if (n == 0) return HP_OK;
  HP_REQUIRE(n_gt >= 1 && h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "hp_det_mask_targets: empty mask table, or a side outside 1 .. 16384");
  HP_REQUIRE(m >= 1 && m <= 256, "hp_det_mask_targets: M outside 1 .. 256");
  HP_REQUIRE(d_masks && d_match && d_rois && d_out, "hp_det_mask_targets: null pointer");
  const int max_grid = 4 * ((h > w ? h : w) + m - 1) / m + 4;
  hipLaunchKernelGGL(mask_targets_kernel, dim3(n), dim3(kThreads), 0, (hipStream_t)stream, d_masks, n_gt, h, w, d_match, d_rois, m, max_grid,
                     d_out);
  return check_launch("hp_det_mask_targets");
}

extern "C" int64_t hp_det_loss_workspace_bytes(int n_rows) {
  if (n_rows < 0) return -1;
  return ((int64_t)n_rows + 1) * 2 * (int64_t)sizeof(double);
}

extern "C" int hp_loss_rpn(int n_anchors, int n_sampled, const int32_t* d_sampled, const float* d_objectness, const float* d_deltas,
                           const int32_t* d_labels, const float* d_targets, float* d_loss, float* d_grad_objectness, float* d_grad_deltas,
                           void* d_workspace, int64_t workspace_bytes, void* stream) {
  HP_REQUIRE(n_anchors >= 0 && n_sampled >= 0, "hp_loss_rpn: negative count");
  if (n_sampled == 0) return HP_OK;
  HP_REQUIRE(n_anchors >= 1, "hp_loss_rpn: sampled rows but no anchors");
  HP_REQUIRE(d_sampled && d_objectness && d_deltas && d_labels && d_targets && d_loss && d_grad_objectness && d_grad_deltas,
             "hp_loss_rpn: null pointer");
  const unsigned blocks = blocks_of(n_sampled);
  HP_REQUIRE(d_workspace && workspace_bytes >= hp_det_loss_workspace_bytes((int)blocks),
             "hp_loss_rpn: workspace smaller than hp_det_loss_workspace_bytes(ceil(n_sampled / 256))");
  hipStream_t st = (hipStream_t)stream;
  HP_CHECK_HIP(hipMemsetAsync(d_grad_objectness, 0, (size_t)n_anchors * sizeof(float), st));
  HP_CHECK_HIP(hipMemsetAsync(d_grad_deltas, 0, (size_t)n_anchors * 4 * sizeof(float), st));
  const double inv_n = 1.0 / (double)n_sampled;
  double* partial = (double*)d_workspace;
  hipLaunchKernelGGL(rpn_loss_kernel, dim3(blocks), dim3(kThreads), 0, st, n_anchors, n_sampled, d_sampled, d_objectness, d_deltas, d_labels,
                     d_targets, inv_n, partial, d_grad_objectness, d_grad_deltas);
  if (int rc = check_launch("hp_loss_rpn")) return rc;
  hipLaunchKernelGGL(sum_kernel<2>, dim3(1), dim3(kThreads), 0, st, (int)blocks, (const double*)partial, inv_n, inv_n, d_loss);
  return check_launch("hp_loss_rpn");
}

extern "C" int hp_loss_fastrcnn(int n, int n_classes, int ld, int ld_reg, const float* d_class_logits, const float* d_box_regression,
                                const int32_t* d_labels, const float* d_targets, float* d_loss, float* d_grad_logits,
                                float* d_grad_regression, void* d_workspace, int64_t workspace_bytes, void* stream) {
  HP_REQUIRE(n >= 0, "hp_loss_fastrcnn: negative count");
  if (n == 0) return HP_OK;
  HP_REQUIRE(n_classes >= 1 && ld >= n_classes && ld_reg >= 4 * n_classes, "hp_loss_fastrcnn: need 1 <= C <= ld and 4 C <= ld_reg");
  HP_REQUIRE(d_class_logits && d_box_regression && d_labels && d_targets && d_loss && d_grad_logits && d_grad_regression,
             "hp_loss_fastrcnn: null pointer");
  const unsigned blocks = blocks_of(n);
  HP_REQUIRE(d_workspace && workspace_bytes >= hp_det_loss_workspace_bytes((int)blocks),
             "hp_loss_fastrcnn: workspace smaller than hp_det_loss_workspace_bytes(ceil(n / 256))");
  hipStream_t st = (hipStream_t)stream;
  const double inv_n = 1.0 / (double)n;
  double* partial = (double*)d_workspace;
  hipLaunchKernelGGL(fastrcnn_loss_kernel, dim3(blocks), dim3(kThreads), 0, st, n, n_classes, ld, ld_reg, d_class_logits, d_box_regression,
                     d_labels, d_targets, inv_n, partial, d_grad_logits, d_grad_regression);
  if (int rc = check_launch("hp_loss_fastrcnn")) return rc;
  hipLaunchKernelGGL(sum_kernel<2>, dim3(1), dim3(kThreads), 0, st, (int)blocks, (const double*)partial, inv_n, inv_n, d_loss);
  return check_launch("hp_loss_fastrcnn");
}

extern "C" int hp_loss_mask(int n, int n_classes, int m, const float* d_mask_logits, const int32_t* d_labels, const float* d_targets,
                            float* d_loss, float* d_grad_logits, void* d_workspace, int64_t workspace_bytes, void* stream) {
  HP_REQUIRE(n >= 0, "hp_loss_mask: negative count");
  if (n == 0) return HP_OK;
  HP_REQUIRE(n_classes >= 1 && m >= 1 && m <= 1024, "hp_loss_mask: need C >= 1 and 1 <= M <= 1024");
  HP_REQUIRE(d_mask_logits && d_labels && d_targets && d_loss && d_grad_logits, "hp_loss_mask: null pointer");
  HP_REQUIRE(d_workspace && workspace_bytes >= hp_det_loss_workspace_bytes(n),
             "hp_loss_mask: workspace smaller than hp_det_loss_workspace_bytes(n)");
  hipStream_t st = (hipStream_t)stream;
  const double inv_n = 1.0 / ((double)n * m * m);
  double* partial = (double*)d_workspace;
  hipLaunchKernelGGL(mask_loss_kernel, dim3(n), dim3(kThreads), 0, st, n_classes, m * m, d_mask_logits, d_labels, d_targets, inv_n, partial,
                     d_grad_logits);
  if (int rc = check_launch("hp_loss_mask")) return rc;
  hipLaunchKernelGGL(sum_kernel<1>, dim3(1), dim3(kThreads), 0, st, n, (const double*)partial, inv_n, inv_n, d_loss);
  return check_launch("hp_loss_mask");
}
