// Training-image augmentations on dense device batches: entry points and every definition are in include/happypose_amd.h
// (hp_aug_*).  The RGB half restates Pillow's integer / unfused-float32 arithmetic and is pinned to it byte for byte; the depth half
// restates the reference's OpenCV calls from their documentation (parity unpinned: OpenCV is not a dependency).
//
//   gray_sum_kernel     the 64-bit sum of an image's gray values for Contrast: shuffles, one integer atomic per workgroup (exact
//                       whatever the order).  A workgroup whose image does not ask for Contrast leaves at once.
//   enhance_kernel      a thread is 4 pixels = 3 dwords (byte loads when H W is no multiple of 4 or a buffer is not 4-byte aligned);
//                       the image's op picks the degenerate value, Sharpness reads its 3 x 3 neighbourhood through the caches.
//   blur_rows_kernel    a workgroup is one line of W <= kLine pixels: the three passes run in the LDS, one trip through memory.
//   blur_cols_kernel    a workgroup is kColTile columns of H <= kLine rows: the same for the three passes along the columns.
//   box_pass_kernel     the general path, one pass per launch through global memory, for a line longer than kLine.
//   noise / grid / correlated / blur / mask / background kernels: a thread is one pixel (4 pixels for the background).
//   missing_kernel      a workgroup is one image: Philox words to the workspace, n_valid, then a radix select (8 bits a pass, LDS
//                       histogram with integer atomics) of the m-th smallest (word, pixel) key; no sort, no host round trip.
//   ellipse_prep_kernel a workgroup is one image: valid pixels per group of 64 (ballot), a carried inclusive scan as in
//                       mesh_sample.hip, then a thread per ellipse finds its centre by binary search and writes the ellipse's record.
//   ellipse_apply_kernel a thread is one pixel against the image's records (uniform reads), the last covering ellipse wins.
// No floating-point atomics anywhere: every result is bit-identical from run to run and independent of the other images.
#include <algorithm>
#include <cfloat>

#include "common.h"
#include "philox.h"
#include "wave.h"

namespace hp {
namespace {

constexpr int kThreads = 256;
constexpr int kLine = 1024;    // the longest line the blur's LDS paths take
constexpr int kColTile = 8;    // columns per workgroup of blur_cols_kernel: 24 bytes = 6 dwords per row
constexpr int kImgThreads = 1024;  // missing_kernel / ellipse_prep_kernel: one workgroup per image
constexpr int kImgWaves = kImgThreads / kWave;
constexpr int64_t kMaxPixels = int64_t(1) << 28;
constexpr uint32_t kStreamNoise = HP_AUG_STREAM_NOISE, kStreamGrid = HP_AUG_STREAM_GRID, kStreamMissing = HP_AUG_STREAM_MISSING;

// Box-Muller on the 24 high bits of words 0 and 1 of counter (index, image, stream, 0)
__device__ inline float normal_deviate(uint32_t index, uint32_t image, uint32_t stream, uint32_t k0, uint32_t k1) {
#pragma clang fp contract(off)
  uint32_t r[4] = {index, image, stream, 0u};
  philox4x32_10(r, k0, k1);
  const float u1 = (float)((r[0] >> 8) + 1u) * 0x1p-24f, u2 = (float)(r[1] >> 8) * 0x1p-24f;  // exact
  return sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
}

// ---------------------------------------------------------------------------------------------------------------- RGB: 4 pixels
template <bool VEC>
__device__ inline void load_px4(const uint8_t* __restrict__ img, int p0, int n, uint8_t c[12]) {
  if (VEC) {
    const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(img + 3 * (int64_t)p0);
    const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = (uint8_t)(w0 >> (8 * i)), c[4 + i] = (uint8_t)(w1 >> (8 * i)), c[8 + i] = (uint8_t)(w2 >> (8 * i));
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) c[i] = i < 3 * n ? img[3 * (int64_t)p0 + i] : (uint8_t)0;
  }
}

template <bool VEC>
__device__ inline void store_px4(uint8_t* __restrict__ img, int p0, int n, const uint8_t c[12]) {
  if (VEC) {
    uint32_t* __restrict__ q = reinterpret_cast<uint32_t*>(img + 3 * (int64_t)p0);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      q[k] = (uint32_t)c[4 * k] | ((uint32_t)c[4 * k + 1] << 8) | ((uint32_t)c[4 * k + 2] << 16) | ((uint32_t)c[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i < 3 * n) img[3 * (int64_t)p0 + i] = c[i];
  }
}

__device__ inline int gray_of(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

template <bool VEC>
__global__ void __launch_bounds__(kThreads) gray_sum_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ op,
                                                            const uint8_t* __restrict__ apply, unsigned long long* __restrict__ sum,
                                                            int hw) {
  __shared__ unsigned long long s_part[kThreads / kWave];
  const int b = blockIdx.y;
  if (!apply[b] || op[b] != HP_AUG_OP_CONTRAST) return;  // uniform over the workgroup
  const uint8_t* __restrict__ img = in + 3 * (int64_t)b * hw;
  unsigned long long acc = 0;
  const int groups = (hw + 3) / 4;
  for (int g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
    const int p0 = 4 * g, n = min(4, hw - p0);
    uint8_t c[12];
    load_px4<VEC>(img, p0, n, c);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n) acc += (unsigned)gray_of(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
  }
  acc = wave_sum(acc);
  if (threadIdx.x % kWave == 0) s_part[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int i = 0; i < kThreads / kWave; ++i) t += s_part[i];
    atomicAdd(&sum[b], t);  // integers: exact in any order
  }
}

__device__ inline uint8_t blend_u8(float a, float x, float f, bool inside) {
  const float t = __fadd_rn(a, __fmul_rn(f, __fsub_rn(x, a)));
  if (inside) return (uint8_t)(int)t;
  return t <= 0.0f ? (uint8_t)0 : t >= 255.0f ? (uint8_t)255 : (uint8_t)(int)t;
}

// Pillow's SMOOTH at an interior pixel: taps float32(k / 13), summed onto 0.5 with row y + 1 first, each row left to right
__device__ inline float smooth_at(const uint8_t* __restrict__ img, int y, int x, int w, int ch) {
  const float k1 = (float)(1.0 / 13.0), k5 = (float)(5.0 / 13.0);
  float s = 0.5f;
#pragma unroll
  for (int dy = 1; dy >= -1; --dy) {
    const uint8_t* __restrict__ row = img + 3 * ((int64_t)(y + dy) * w + x) + ch;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) s = __fadd_rn(s, __fmul_rn((float)row[3 * dx], (dy == 0 && dx == 0) ? k5 : k1));
  }
  s = floorf(s);
  return s < 0.0f ? 0.0f : s > 255.0f ? 255.0f : s;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) enhance_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ op,
                                                           const float* __restrict__ factor, const uint8_t* __restrict__ apply,
                                                           const unsigned long long* __restrict__ sum, uint8_t* __restrict__ out, int h,
                                                           int w) {
  const int b = blockIdx.y, hw = h * w;
  const int p0 = 4 * (blockIdx.x * kThreads + threadIdx.x);
  if (p0 >= hw) return;
  const int n = min(4, hw - p0);
  const uint8_t* __restrict__ img = in + 3 * (int64_t)b * hw;
  uint8_t c[12], o[12];
  load_px4<VEC>(img, p0, n, c);
  const int kind = op[b];  // uniform over the workgroup
  if (apply[b] && kind >= 0 && kind <= HP_AUG_OP_SHARPNESS) {
    const float f = factor[b];
    const bool inside = f >= 0.0f && f <= 1.0f;
    const float mean = kind == HP_AUG_OP_CONTRAST ? (float)(int)((double)sum[b] / (double)hw + 0.5) : 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float a[3] = {mean, mean, mean};
      if (kind == HP_AUG_OP_COLOR) {
        a[0] = a[1] = a[2] = (float)gray_of(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
      } else if (kind == HP_AUG_OP_SHARPNESS) {
        const int p = p0 + i, y = p / w, x = p - y * w;
        const bool interior = i < n && y >= 1 && y < h - 1 && x >= 1 && x < w - 1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a[ch] = interior ? smooth_at(img, y, x, w, ch) : (float)c[3 * i + ch];  // the border is copied
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[3 * i + ch] = blend_u8(a[ch], (float)c[3 * i + ch], f, inside);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) o[i] = c[i];
  }
  store_px4<VEC>(out + 3 * (int64_t)b * hw, p0, n, o);
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) background_kernel(const uint8_t* in, const int32_t* __restrict__ seg,
                                                              const uint8_t* __restrict__ bg, const uint8_t* __restrict__ apply,
                                                              uint8_t* out, int hw) {
  const int b = blockIdx.y;
  const int p0 = 4 * (blockIdx.x * kThreads + threadIdx.x);
  if (p0 >= hw) return;
  const int n = min(4, hw - p0);
  uint8_t c[12];
  load_px4<VEC>(in + 3 * (int64_t)b * hw, p0, n, c);
  if (apply[b]) {
    uint8_t g[12];
    load_px4<VEC>(bg + 3 * (int64_t)b * hw, p0, n, g);
    const int32_t* __restrict__ s = seg + (int64_t)b * hw + p0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n && s[i] == 0) c[3 * i] = g[3 * i], c[3 * i + 1] = g[3 * i + 1], c[3 * i + 2] = g[3 * i + 2];
  }
  store_px4<VEC>(out + 3 * (int64_t)b * hw, p0, n, c);
}

// ---------------------------------------------------------------------------------------------------------------- RGB: blur
// one pass at position i of a line of n samples, `stride` bytes apart (Pillow's ImagingLineBoxBlur: 32-bit integers throughout)
__device__ inline uint8_t box_at(const uint8_t* __restrict__ line, int i, int n, int stride, int r, uint32_t ww, uint32_t fw) {
  uint32_t acc = 0;
  for (int k = -r; k <= r; ++k) acc += line[(int64_t)min(max(i + k, 0), n - 1) * stride];
  const uint32_t edge = (uint32_t)line[(int64_t)min(max(i - r - 1, 0), n - 1) * stride] + line[(int64_t)min(max(i + r + 1, 0), n - 1) * stride];
  return (uint8_t)((ww * acc + fw * edge + (1u << 23)) >> 24);
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) blur_rows_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ radius,
                                                             const uint32_t* __restrict__ ww_, const uint32_t* __restrict__ fw_,
                                                             const uint8_t* __restrict__ apply, uint8_t* __restrict__ out, int h, int w) {
  __shared__ uint32_t s_buf[2][3 * kLine / 4];
  const int b = blockIdx.y, y = blockIdx.x, tid = threadIdx.x, nb = 3 * w;  // w <= kLine
  const int64_t base = 3 * ((int64_t)b * h + y) * w;
  uint8_t* s0 = reinterpret_cast<uint8_t*>(s_buf[0]);
  uint8_t* s1 = reinterpret_cast<uint8_t*>(s_buf[1]);
  if (VEC) {
    const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(in + base);
    for (int i = tid; i < nb / 4; i += kThreads) s_buf[0][i] = q[i];
  } else {
    for (int i = tid; i < nb; i += kThreads) s0[i] = in[base + i];
  }
  __syncthreads();
  const uint8_t* res = s0;
  if (apply[b]) {
    const int r = max(radius[b], 0);
    const uint32_t ww = ww_[b], fw = fw_[b];
    for (int i = tid; i < nb; i += kThreads) s1[i] = box_at(s0 + i % 3, i / 3, w, 3, r, ww, fw);
    __syncthreads();
    for (int i = tid; i < nb; i += kThreads) s0[i] = box_at(s1 + i % 3, i / 3, w, 3, r, ww, fw);
    __syncthreads();
    for (int i = tid; i < nb; i += kThreads) s1[i] = box_at(s0 + i % 3, i / 3, w, 3, r, ww, fw);
    __syncthreads();
    res = s1;
  }
  if (VEC) {
    uint32_t* __restrict__ q = reinterpret_cast<uint32_t*>(out + base);
    const uint32_t* rw = reinterpret_cast<const uint32_t*>(res);
    for (int i = tid; i < nb / 4; i += kThreads) q[i] = rw[i];
  } else {
    for (int i = tid; i < nb; i += kThreads) out[base + i] = res[i];
  }
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) blur_cols_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ radius,
                                                             const uint32_t* __restrict__ ww_, const uint32_t* __restrict__ fw_,
                                                             const uint8_t* __restrict__ apply, uint8_t* __restrict__ out, int h, int w) {
  constexpr int kRow = 3 * kColTile;  // bytes per row of the tile
  __shared__ uint32_t s_buf[2][kRow * kLine / 4];
  const int b = blockIdx.y, x0 = blockIdx.x * kColTile, tid = threadIdx.x;  // h <= kLine
  const int tb = 3 * min(kColTile, w - x0);  // bytes per row that exist; a multiple of 4 with VEC (w % 4 == 0)
  const int64_t base = 3 * ((int64_t)b * h * w + x0);
  uint8_t* s0 = reinterpret_cast<uint8_t*>(s_buf[0]);
  uint8_t* s1 = reinterpret_cast<uint8_t*>(s_buf[1]);
  if (VEC) {
    const int td = tb / 4;
    for (int e = tid; e < h * td; e += kThreads) {
      const int yy = e / td, j = e - yy * td;
      s_buf[0][yy * (kRow / 4) + j] = reinterpret_cast<const uint32_t*>(in + base + 3 * (int64_t)yy * w)[j];
    }
  } else {
    for (int e = tid; e < h * tb; e += kThreads) {
      const int yy = e / tb, j = e - yy * tb;
      s0[yy * kRow + j] = in[base + 3 * (int64_t)yy * w + j];
    }
  }
  __syncthreads();
  const uint8_t* res = s0;
  if (apply[b]) {
    const int r = max(radius[b], 0);
    const uint32_t ww = ww_[b], fw = fw_[b];
    for (int pass = 0; pass < 3; ++pass) {
      const uint8_t* src = pass == 1 ? s1 : s0;
      uint8_t* dst = pass == 1 ? s0 : s1;
      for (int e = tid; e < h * tb; e += kThreads) {
        const int yy = e / tb, j = e - yy * tb;
        dst[yy * kRow + j] = box_at(src + j, yy, h, kRow, r, ww, fw);
      }
      __syncthreads();
    }
    res = s1;
  }
  if (VEC) {
    const int td = tb / 4;
    const uint32_t* rw = reinterpret_cast<const uint32_t*>(res);
    for (int e = tid; e < h * td; e += kThreads) {
      const int yy = e / td, j = e - yy * td;
      reinterpret_cast<uint32_t*>(out + base + 3 * (int64_t)yy * w)[j] = rw[yy * (kRow / 4) + j];
    }
  } else {
    for (int e = tid; e < h * tb; e += kThreads) {
      const int yy = e / tb, j = e - yy * tb;
      out[base + 3 * (int64_t)yy * w + j] = res[yy * kRow + j];
    }
  }
}

// the general path: one pass per launch, a thread is one byte; along_rows: the line is a row, else a column
__global__ void __launch_bounds__(kThreads) box_pass_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ radius,
                                                            const uint32_t* __restrict__ ww_, const uint32_t* __restrict__ fw_,
                                                            const uint8_t* __restrict__ apply, uint8_t* __restrict__ out, int h, int w,
                                                            int along_rows) {
  const int b = blockIdx.y;
  const int64_t nb = 3 * (int64_t)h * w, e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= nb) return;
  const uint8_t* __restrict__ img = in + (int64_t)b * nb;
  uint8_t v = img[e];
  if (apply[b]) {
    const int p = (int)(e / 3), ch = (int)(e - 3 * (int64_t)p), y = p / w, x = p - y * w;
    const int r = max(radius[b], 0);
    v = along_rows ? box_at(img + 3 * (int64_t)y * w + ch, x, w, 3, r, ww_[b], fw_[b])
                   : box_at(img + 3 * (int64_t)x + ch, y, h, 3 * w, r, ww_[b], fw_[b]);
  }
  out[(int64_t)b * nb + e] = v;
}

// ---------------------------------------------------------------------------------------------------------------- depth
__device__ inline float clip_depth(float v) { return v < 0.0f ? 0.0f : v > FLT_MAX ? FLT_MAX : v; }  // NaN passes through

__global__ void __launch_bounds__(kThreads) noise_kernel(const float* depth, const float* __restrict__ std_,
                                                         const uint8_t* __restrict__ apply, uint32_t k0, uint32_t k1,
                                                         float* out, int hw) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= hw) return;
  float v = depth[(int64_t)b * hw + p];
  if (apply[b] && v > 0.0f) v = clip_depth(v + std_[b] * normal_deviate((uint32_t)p, (uint32_t)b, kStreamNoise, k0, k1));
  out[(int64_t)b * hw + p] = v;
}

__device__ inline bool grid_ok(int gh, int gw, int hw) { return gh > 0 && gw > 0 && (int64_t)gh * gw <= hw; }

__global__ void __launch_bounds__(kThreads) grid_kernel(const float* __restrict__ std_, const int32_t* __restrict__ grid_h,
                                                        const int32_t* __restrict__ grid_w, const uint8_t* __restrict__ apply,
                                                        uint32_t k0, uint32_t k1, float* __restrict__ grid, int hw) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, c = blockIdx.x * kThreads + threadIdx.x;
  const int gh = grid_h[b], gw = grid_w[b];
  if (!apply[b] || !grid_ok(gh, gw, hw) || c >= gh * gw) return;
  grid[(int64_t)b * hw + c] = std_[b] * normal_deviate((uint32_t)c, (uint32_t)b, kStreamGrid, k0, k1);
}

__device__ inline void cubic_weights(float t, float wgt[4]) {
#pragma clang fp contract(off)
  const float A = -0.75f, t1 = t + 1.0f, u = 1.0f - t;
  wgt[0] = ((A * t1 - 5.0f * A) * t1 + 8.0f * A) * t1 - 4.0f * A;
  wgt[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  wgt[2] = ((A + 2.0f) * u - (A + 3.0f)) * u * u + 1.0f;
  wgt[3] = 1.0f - wgt[0] - wgt[1] - wgt[2];
}

__global__ void __launch_bounds__(kThreads) correlated_kernel(const float* depth, const int32_t* __restrict__ grid_h,
                                                              const int32_t* __restrict__ grid_w, const uint8_t* __restrict__ apply,
                                                              const float* __restrict__ grid, float* out, int h, int w) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, hw = h * w, p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= hw) return;
  float v = depth[(int64_t)b * hw + p];
  const int gh = grid_h[b], gw = grid_w[b];
  if (apply[b] && grid_ok(gh, gw, hw) && v > 0.0f) {
    const int y = p / w, x = p - y * w;
    const float* __restrict__ g = grid + (int64_t)b * hw;
    const float fy = ((float)y + 0.5f) * ((float)gh / (float)h) - 0.5f, fx = ((float)x + 0.5f) * ((float)gw / (float)w) - 0.5f;
    const float sy = floorf(fy), sx = floorf(fx);
    float wy[4], wx[4];
    cubic_weights(fy - sy, wy);
    cubic_weights(fx - sx, wx);
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int yy = min(max((int)sy - 1 + j, 0), gh - 1);
      float row = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) row = row + wx[i] * g[yy * gw + min(max((int)sx - 1 + i, 0), gw - 1)];
      acc = acc + wy[j] * row;
    }
    v = clip_depth(v + acc);
  }
  out[(int64_t)b * hw + p] = v;
}

__device__ inline int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);  // a no-op for k <= n; keeps a bad k inside the image
}

__global__ void __launch_bounds__(kThreads) depth_blur_kernel(const float* __restrict__ depth, const int32_t* __restrict__ ksize,
                                                              int k_max, const uint8_t* __restrict__ apply, float* __restrict__ out,
                                                              int h, int w) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, hw = h * w, p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= hw) return;
  const float* __restrict__ d = depth + (int64_t)b * hw;
  float v = d[p];
  const int k = ksize[b];
  if (apply[b] && k >= 1 && k <= k_max) {
    const int y = p / w, x = p - y * w, a = k / 2;
    float s = 0.0f;
    for (int dy = 0; dy < k; ++dy) {
      const float* __restrict__ row = d + (int64_t)reflect101(y - a + dy, h) * w;
      for (int dx = 0; dx < k; ++dx) s = s + row[reflect101(x - a + dx, w)];
    }
    v = s / (float)(k * k);
  }
  out[(int64_t)b * hw + p] = v;
}

__global__ void __launch_bounds__(kThreads) depth_mask_kernel(const float* depth, const int32_t* __restrict__ seg,
                                                              const uint8_t* __restrict__ apply, float* out, int hw) {
  const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= hw) return;
  float v = depth[(int64_t)b * hw + p];
  if (apply[b] && (!seg || seg[(int64_t)b * hw + p] == 0)) v = 0.0f;
  out[(int64_t)b * hw + p] = v;
}

// sum of one int per thread over the workgroup of kImgThreads, to every thread; s_red [kImgWaves] is free again on return
__device__ inline int block_sum(int v, int* s_red) {
  v = wave_sum(v);
  if (threadIdx.x % kWave == 0) s_red[threadIdx.x / kWave] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int i = 0; i < kImgWaves; ++i) t += s_red[i];
  __syncthreads();
  return t;
}

__global__ void __launch_bounds__(kImgThreads) missing_kernel(const float* __restrict__ depth, const double* __restrict__ fraction,
                                                              const uint8_t* __restrict__ apply, uint32_t k0, uint32_t k1,
                                                              uint32_t* __restrict__ words, float* out, int hw) {
  __shared__ int s_hist[256];
  __shared__ int s_red[kImgWaves];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_k, s_done;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* d = depth + (int64_t)b * hw;  // may alias o: a pixel is read and written by the same thread
  float* o = out + (int64_t)b * hw;
  uint32_t* __restrict__ wd = words + (int64_t)b * hw;
  const bool on = apply[b] != 0;
  int cnt = 0;
  if (on)
    for (int p = tid; p < hw; p += kImgThreads)
      if (d[p] > 0.0f) {
        uint32_t r[4] = {(uint32_t)p, (uint32_t)b, kStreamMissing, 0u};
        philox4x32_10(r, k0, k1);
        wd[p] = r[0];  // read back by this thread alone
        ++cnt;
      }
  const int n_valid = block_sum(cnt, s_red);
  const double fr = on ? fraction[b] : 0.0;
  int m = fr > 0.0 ? (int)fmin(fr * (double)n_valid, (double)n_valid) : 0;
  if (m <= 0) {  // uniform
    if (o != d)
      for (int p = tid; p < hw; p += kImgThreads) o[p] = d[p];
    return;
  }
  // the m-th smallest key (word << 32 | pixel): keys are distinct, so exactly m keys are <= it
  unsigned long long prefix = 0, thr = 0;
  int k = m;
  for (int shift = 56; shift >= 0; shift -= 8) {
    const unsigned long long hi_mask = shift == 56 ? 0ull : ~0ull << (shift + 8);
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    for (int p = tid; p < hw; p += kImgThreads)
      if (d[p] > 0.0f) {
        const unsigned long long key = ((unsigned long long)wd[p] << 32) | (uint32_t)p;
        if ((key & hi_mask) == prefix) atomicAdd(&s_hist[(int)((key >> shift) & 255)], 1);
      }
    __syncthreads();
    if (tid == 0) {
      int c = 0, bin = 0;
      for (; bin < 255; ++bin) {
        if (c + s_hist[bin] >= k) break;
        c += s_hist[bin];
      }
      s_k = k - c;
      s_prefix = prefix | ((unsigned long long)bin << shift);
      s_done = s_hist[bin] == k - c;  // the whole bin goes: every lower digit may be anything
    }
    __syncthreads();
    prefix = s_prefix, k = s_k;
    const int done = s_done;
    __syncthreads();
    thr = prefix | (shift ? (1ull << shift) - 1 : 0ull);
    if (done) break;
  }
  for (int p = tid; p < hw; p += kImgThreads) {
    float v = d[p];
    if (v > 0.0f && (((unsigned long long)wd[p] << 32) | (uint32_t)p) <= thr) v = 0.0f;
    o[p] = v;
  }
}

// record of one ellipse: cx, cy, cos, sin, a, b, value, unused
__global__ void __launch_bounds__(kImgThreads) ellipse_prep_kernel(const float* __restrict__ depth, const float* __restrict__ table,
                                                                   const int32_t* __restrict__ count, int E,
                                                                   const uint8_t* __restrict__ apply, int32_t* __restrict__ n_valid_out,
                                                                   int32_t* __restrict__ group_cum, float* __restrict__ recs, int h,
                                                                   int w) {
#pragma clang fp contract(off)
  __shared__ int s_tot[2][kImgWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave, hw = h * w;
  const int cnt = min(max(count[b], 0), E);
  if (!apply[b] || cnt == 0) {  // uniform
    if (tid == 0) n_valid_out[2 * b] = 0;
    return;
  }
  const float* __restrict__ d = depth + (int64_t)b * hw;
  int32_t* gc = group_cum + (int64_t)b * hw;  // groups <= hw entries
  const int groups = (hw + kWave - 1) / kWave;
  for (int g = wave; g < groups; g += kImgWaves) {
    const int p = g * kWave + lane;
    const unsigned long long mask = __ballot(p < hw && d[p] > 0.0f);
    if (lane == 0) gc[g] = __popcll(mask);
  }
  __syncthreads();
  int carry = 0;
  for (int c0 = 0, step = 0; c0 < groups; c0 += kImgThreads, ++step) {  // inclusive scan in place, the prefix carried
    const int g = c0 + tid;
    int a = g < groups ? gc[g] : 0;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int t = __shfl_up(a, off, kWave);
      if (lane >= off) a += t;
    }
    const int buf = step & 1;
    if (lane == kWave - 1) s_tot[buf][wave] = a;
    __syncthreads();
    int prefix = 0, chunk = 0;
#pragma unroll
    for (int wv = 0; wv < kImgWaves; ++wv) {
      if (wv == wave) prefix = chunk;
      chunk += s_tot[buf][wv];
    }
    if (g < groups) gc[g] = carry + prefix + a;
    carry += chunk;
  }
  __syncthreads();
  const int n_valid = carry;
  if (tid == 0) n_valid_out[2 * b] = n_valid;
  if (n_valid == 0) return;
  for (int e = tid; e < cnt; e += kImgThreads) {
    const float* __restrict__ t = table + ((int64_t)b * E + e) * 5;
    const float u = t[0];
    int64_t target = u > 0.0f ? (int64_t)floor(fmin((double)u * (double)n_valid, (double)n_valid)) : 0;
    target = target > n_valid - 1 ? n_valid - 1 : target;
    int lo = 0, hi = groups - 1;  // the first group whose inclusive count exceeds target: it exists, as target < n_valid
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (gc[mid] > target)
        hi = mid;
      else
        lo = mid + 1;
    }
    int rank = (int)(target - (lo ? gc[lo - 1] : 0));
    int p = lo * kWave;
    const int p_end = min(p + kWave, hw) - 1;
    for (; p < p_end; ++p)
      if (d[p] > 0.0f && rank-- == 0) break;
    const float ang = t[3] * 0.017453292f;
    float* __restrict__ r = recs + ((int64_t)b * E + e) * 8;
    r[0] = (float)(p % w), r[1] = (float)(p / w);
    r[2] = cosf(ang), r[3] = sinf(ang);
    r[4] = fmaxf(t[1], 0.5f), r[5] = fmaxf(t[2], 0.5f);
    r[6] = t[4], r[7] = 0.0f;
  }
}

__global__ void __launch_bounds__(kThreads) ellipse_apply_kernel(const float* depth, const int32_t* __restrict__ count,
                                                                 int E, const int32_t* __restrict__ n_valid_in,
                                                                 const float* __restrict__ recs, int noise, float* out,
                                                                 int h, int w) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, hw = h * w, p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= hw) return;
  float v = depth[(int64_t)b * hw + p];
  if (n_valid_in[2 * b] > 0) {  // 0 as well where the image's apply flag or count is 0
    const int cnt = min(max(count[b], 0), E);
    const int y = p / w, x = p - y * w;
    bool hit = false;
    float add = 0.0f;
    for (int e = 0; e < cnt; ++e) {
      const float* __restrict__ r = recs + ((int64_t)b * E + e) * 8;  // uniform over the workgroup
      const float dx = (float)x - r[0], dy = (float)y - r[1];
      const float xr = dx * r[2] + dy * r[3], yr = dy * r[2] - dx * r[3];
      const float qa = xr / r[4], qb = yr / r[5];
      if (qa * qa + qb * qb <= 1.0f) hit = true, add = r[6];
    }
    if (hit) v = noise ? (v > 0.0f ? v + add : v) : 0.0f;
  }
  out[(int64_t)b * hw + p] = v;
}

// ---------------------------------------------------------------------------------------------------------------- host side
struct Workspace {
  unsigned long long* head;  // [B] 8 bytes per image: the gray sum, or n_valid in its low word
  uint8_t* region;           // 4 H W bytes per image
  float* recs;               // [B][E][8]
};

inline int64_t region_bytes(int B, int64_t hw) { return round_up(4 * (int64_t)B * hw, 8); }
inline int64_t ws_bytes(int B, int64_t hw, int E) { return 8 * (int64_t)B + region_bytes(B, hw) + 32 * (int64_t)B * E; }

inline Workspace carve(void* ws, int B, int64_t hw) {
  uint8_t* p = static_cast<uint8_t*>(ws);
  return {reinterpret_cast<unsigned long long*>(p), p + 8 * (int64_t)B, reinterpret_cast<float*>(p + 8 * (int64_t)B + region_bytes(B, hw))};
}

inline dim3 pixel_grid(int64_t items, int B) { return dim3((unsigned)((items + kThreads - 1) / kThreads), (unsigned)B); }

}  // namespace
}  // namespace hp

using namespace hp;

// the scalar checks shared by every entry point; B == 0 returns HP_OK from the caller before any pointer is looked at
#define HP_AUG_DIMS(name)                                                                           \
  HP_REQUIRE(B >= 0 && h > 0 && w > 0, name ": B >= 0, h > 0 and w > 0");                           \
  HP_REQUIRE(B <= 65535 && (int64_t)h * w <= kMaxPixels, name ": at most 65535 images of 2^28 pixels"); \
  if (B == 0) return HP_OK
#define HP_AUG_WS(name, E)                                                                                              \
  HP_REQUIRE(d_workspace && workspace_bytes >= ws_bytes(B, (int64_t)h * w, (E)), name ": workspace smaller than hp_aug_workspace_bytes"); \
  HP_REQUIRE(aligned(d_workspace, 8), name ": d_workspace must be 8-byte aligned")

extern "C" int64_t hp_aug_workspace_bytes(int B, int h, int w, int max_ellipses) {
  if (B < 0 || B > 65535 || h <= 0 || w <= 0 || (int64_t)h * w > kMaxPixels || max_ellipses < 0) return -1;
  return ws_bytes(B, (int64_t)h * w, max_ellipses);
}

extern "C" int hp_aug_rgb_enhance(int B, int h, int w, const uint8_t* d_rgb, const int32_t* d_op, const float* d_factor,
                                  const uint8_t* d_apply, uint8_t* d_out, void* d_workspace, int64_t workspace_bytes, void* stream) {
  HP_AUG_DIMS("hp_aug_rgb_enhance");
  HP_REQUIRE(d_rgb && d_op && d_factor && d_apply && d_out, "hp_aug_rgb_enhance: null pointer");
  HP_REQUIRE(d_rgb != d_out, "hp_aug_rgb_enhance: d_out must not alias d_rgb (Sharpness reads a neighbourhood)");
  HP_AUG_WS("hp_aug_rgb_enhance", 0);
  hipStream_t st = (hipStream_t)stream;
  const int hw = h * w;
  const Workspace ws = carve(d_workspace, B, hw);
  HP_CHECK_HIP(hipMemsetAsync(ws.head, 0, 8 * (size_t)B, st));
  const bool vec = hw % 4 == 0 && aligned(d_rgb, 4) && aligned(d_out, 4);
  const int groups = (hw + 3) / 4;
  const dim3 sum_grid((unsigned)std::min((groups + kThreads - 1) / kThreads, 256), (unsigned)B);
  if (vec) {
    hipLaunchKernelGGL(gray_sum_kernel<true>, sum_grid, dim3(kThreads), 0, st, d_rgb, d_op, d_apply, ws.head, hw);
    hipLaunchKernelGGL(enhance_kernel<true>, pixel_grid(groups, B), dim3(kThreads), 0, st, d_rgb, d_op, d_factor, d_apply, ws.head, d_out, h, w);
  } else {
    hipLaunchKernelGGL(gray_sum_kernel<false>, sum_grid, dim3(kThreads), 0, st, d_rgb, d_op, d_apply, ws.head, hw);
    hipLaunchKernelGGL(enhance_kernel<false>, pixel_grid(groups, B), dim3(kThreads), 0, st, d_rgb, d_op, d_factor, d_apply, ws.head, d_out, h, w);
  }
  return check_launch("hp_aug_rgb_enhance");
}

extern "C" int hp_aug_rgb_blur(int B, int h, int w, const uint8_t* d_rgb, const int32_t* d_radius, const uint32_t* d_ww,
                               const uint32_t* d_fw, const uint8_t* d_apply, uint8_t* d_out, int force_general, void* d_workspace,
                               int64_t workspace_bytes, void* stream) {
  HP_AUG_DIMS("hp_aug_rgb_blur");
  HP_REQUIRE(d_rgb && d_radius && d_ww && d_fw && d_apply && d_out, "hp_aug_rgb_blur: null pointer");
  HP_REQUIRE(d_rgb != d_out, "hp_aug_rgb_blur: d_out must not alias d_rgb");
  HP_AUG_WS("hp_aug_rgb_blur", 0);
  hipStream_t st = (hipStream_t)stream;
  const Workspace ws = carve(d_workspace, B, (int64_t)h * w);
  uint8_t* tmp = ws.region;  // [B][h][w][3]; 4-byte aligned
  const bool vec = w % 4 == 0 && aligned(d_rgb, 4) && aligned(d_out, 4);
  const dim3 bytes_grid = pixel_grid(3 * (int64_t)h * w, B);
#define HP_AUG_PASS(src, dst, rows) \
  hipLaunchKernelGGL(box_pass_kernel, bytes_grid, dim3(kThreads), 0, st, (src), d_radius, d_ww, d_fw, d_apply, (dst), h, w, (rows))
  // the rows: d_rgb -> tmp
  if (w <= kLine && !force_general) {
    if (vec)
      hipLaunchKernelGGL(blur_rows_kernel<true>, dim3((unsigned)h, (unsigned)B), dim3(kThreads), 0, st, d_rgb, d_radius, d_ww, d_fw, d_apply, tmp, h, w);
    else
      hipLaunchKernelGGL(blur_rows_kernel<false>, dim3((unsigned)h, (unsigned)B), dim3(kThreads), 0, st, d_rgb, d_radius, d_ww, d_fw, d_apply, tmp, h, w);
  } else {
    HP_AUG_PASS(d_rgb, tmp, 1);
    HP_AUG_PASS((const uint8_t*)tmp, d_out, 1);
    HP_AUG_PASS((const uint8_t*)d_out, tmp, 1);
  }
  if (int rc = check_launch("hp_aug_rgb_blur (rows)")) return rc;
  // the columns: tmp -> d_out
  if (h <= kLine && !force_general) {
    const dim3 grid((unsigned)((w + kColTile - 1) / kColTile), (unsigned)B);
    if (vec)
      hipLaunchKernelGGL(blur_cols_kernel<true>, grid, dim3(kThreads), 0, st, (const uint8_t*)tmp, d_radius, d_ww, d_fw, d_apply, d_out, h, w);
    else
      hipLaunchKernelGGL(blur_cols_kernel<false>, grid, dim3(kThreads), 0, st, (const uint8_t*)tmp, d_radius, d_ww, d_fw, d_apply, d_out, h, w);
  } else {
    HP_AUG_PASS((const uint8_t*)tmp, d_out, 0);
    HP_AUG_PASS((const uint8_t*)d_out, tmp, 0);
    HP_AUG_PASS((const uint8_t*)tmp, d_out, 0);
  }
#undef HP_AUG_PASS
  return check_launch("hp_aug_rgb_blur (columns)");
}

extern "C" int hp_aug_replace_background(int B, int h, int w, const uint8_t* d_rgb, const int32_t* d_segmentation,
                                         const uint8_t* d_background, const uint8_t* d_apply, uint8_t* d_out, void* stream) {
  HP_AUG_DIMS("hp_aug_replace_background");
  HP_REQUIRE(d_rgb && d_segmentation && d_background && d_apply && d_out, "hp_aug_replace_background: null pointer");
  const int hw = h * w;
  const bool vec = hw % 4 == 0 && aligned(d_rgb, 4) && aligned(d_out, 4) && aligned(d_background, 4);
  if (vec)
    hipLaunchKernelGGL(background_kernel<true>, pixel_grid((hw + 3) / 4, B), dim3(kThreads), 0, (hipStream_t)stream, d_rgb, d_segmentation, d_background, d_apply, d_out, hw);
  else
    hipLaunchKernelGGL(background_kernel<false>, pixel_grid((hw + 3) / 4, B), dim3(kThreads), 0, (hipStream_t)stream, d_rgb, d_segmentation, d_background, d_apply, d_out, hw);
  return check_launch("hp_aug_replace_background");
}

extern "C" int hp_aug_depth_noise(int B, int h, int w, const float* d_depth, const float* d_std, int correlated, const int32_t* d_grid_h,
                                  const int32_t* d_grid_w, const uint8_t* d_apply, uint64_t seed, float* d_out, void* d_workspace,
                                  int64_t workspace_bytes, void* stream) {
  HP_AUG_DIMS("hp_aug_depth_noise");
  HP_REQUIRE(d_depth && d_std && d_apply && d_out, "hp_aug_depth_noise: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int hw = h * w;
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
  if (!correlated) {
    hipLaunchKernelGGL(noise_kernel, pixel_grid(hw, B), dim3(kThreads), 0, st, d_depth, d_std, d_apply, k0, k1, d_out, hw);
    return check_launch("hp_aug_depth_noise");
  }
  HP_REQUIRE(d_grid_h && d_grid_w, "hp_aug_depth_noise: correlated noise needs d_grid_h and d_grid_w");
  HP_AUG_WS("hp_aug_depth_noise", 0);
  float* grid = reinterpret_cast<float*>(carve(d_workspace, B, hw).region);
  hipLaunchKernelGGL(grid_kernel, pixel_grid(hw, B), dim3(kThreads), 0, st, d_std, d_grid_h, d_grid_w, d_apply, k0, k1, grid, hw);
  if (int rc = check_launch("hp_aug_depth_noise (grid)")) return rc;
  hipLaunchKernelGGL(correlated_kernel, pixel_grid(hw, B), dim3(kThreads), 0, st, d_depth, d_grid_h, d_grid_w, d_apply, (const float*)grid, d_out, h, w);
  return check_launch("hp_aug_depth_noise (upsample)");
}

extern "C" int hp_aug_depth_missing(int B, int h, int w, const float* d_depth, const double* d_fraction, const uint8_t* d_apply,
                                    uint64_t seed, float* d_out, void* d_workspace, int64_t workspace_bytes, void* stream) {
  HP_AUG_DIMS("hp_aug_depth_missing");
  HP_REQUIRE(d_depth && d_fraction && d_apply && d_out, "hp_aug_depth_missing: null pointer");
  HP_AUG_WS("hp_aug_depth_missing", 0);
  const int hw = h * w;
  uint32_t* words = reinterpret_cast<uint32_t*>(carve(d_workspace, B, hw).region);
  hipLaunchKernelGGL(missing_kernel, dim3((unsigned)B), dim3(kImgThreads), 0, (hipStream_t)stream, d_depth, d_fraction, d_apply,
                     (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), words, d_out, hw);
  return check_launch("hp_aug_depth_missing");
}

extern "C" int hp_aug_depth_ellipses(int B, int h, int w, const float* d_depth, const float* d_table, const int32_t* d_count,
                                     int max_ellipses, int noise, const uint8_t* d_apply, float* d_out, void* d_workspace,
                                     int64_t workspace_bytes, void* stream) {
  HP_AUG_DIMS("hp_aug_depth_ellipses");
  HP_REQUIRE(max_ellipses >= 0, "hp_aug_depth_ellipses: negative max_ellipses");
  HP_REQUIRE(d_depth && d_count && d_apply && d_out && (d_table || max_ellipses == 0), "hp_aug_depth_ellipses: null pointer");
  HP_AUG_WS("hp_aug_depth_ellipses", max_ellipses);
  hipStream_t st = (hipStream_t)stream;
  const Workspace ws = carve(d_workspace, B, (int64_t)h * w);
  int32_t* n_valid = reinterpret_cast<int32_t*>(ws.head);
  hipLaunchKernelGGL(ellipse_prep_kernel, dim3((unsigned)B), dim3(kImgThreads), 0, st, d_depth, d_table, d_count, max_ellipses, d_apply,
                     n_valid, reinterpret_cast<int32_t*>(ws.region), ws.recs, h, w);
  if (int rc = check_launch("hp_aug_depth_ellipses (centres)")) return rc;
  hipLaunchKernelGGL(ellipse_apply_kernel, pixel_grid((int64_t)h * w, B), dim3(kThreads), 0, st, d_depth, d_count, max_ellipses,
                     (const int32_t*)n_valid, (const float*)ws.recs, noise, d_out, h, w);
  return check_launch("hp_aug_depth_ellipses");
}

extern "C" int hp_aug_depth_blur(int B, int h, int w, const float* d_depth, const int32_t* d_ksize, int k_max, const uint8_t* d_apply,
                                 float* d_out, void* stream) {
  HP_AUG_DIMS("hp_aug_depth_blur");
  HP_REQUIRE(d_depth && d_ksize && d_apply && d_out, "hp_aug_depth_blur: null pointer");
  HP_REQUIRE(k_max >= 1, "hp_aug_depth_blur: k_max >= 1");
  HP_REQUIRE(k_max <= h && k_max <= w, "hp_aug_depth_blur: a side shorter than k_max (reflect-101 is not defined)");
  HP_REQUIRE(d_depth != d_out, "hp_aug_depth_blur: d_out must not alias d_depth");
  hipLaunchKernelGGL(depth_blur_kernel, pixel_grid((int64_t)h * w, B), dim3(kThreads), 0, (hipStream_t)stream, d_depth, d_ksize, k_max,
                     d_apply, d_out, h, w);
  return check_launch("hp_aug_depth_blur");
}

extern "C" int hp_aug_depth_mask(int B, int h, int w, const float* d_depth, const int32_t* d_segmentation, const uint8_t* d_apply,
                                 float* d_out, void* stream) {
  HP_AUG_DIMS("hp_aug_depth_mask");
  HP_REQUIRE(d_depth && d_apply && d_out, "hp_aug_depth_mask: null pointer");
  hipLaunchKernelGGL(depth_mask_kernel, pixel_grid((int64_t)h * w, B), dim3(kThreads), 0, (hipStream_t)stream, d_depth, d_segmentation,
                     d_apply, d_out, h * w);
  return check_launch("hp_aug_depth_mask");
}
