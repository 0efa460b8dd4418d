// Frame geometry on dense device batches: Pillow-exact resize of uint8 RGB frames, nearest resize of 4-byte frames and modal
// boxes from an id map.  Entry points and every definition are in include/happypose_amd.h (hp_resize_*, hp_seg_boxes).
//
//   resize_rows_kernel  the pass along x.  A workgroup is kRowsPerGroup source rows x kTile output pixels; per row it stages the
//                       bytes its windows cover (one band, dword loads from the 4-byte aligned address below the first byte) in
//                       the LDS, a thread is one output pixel and loops over its window, the tile's 3 kTile bytes go back through
//                       the LDS so that they leave as dwords.  A tap outside the frame or outside the band reads 0: the host's
//                       tables and band cannot make the kernel touch memory it was not given.
//   resize_cols_kernel  the pass along y.  A thread is 4 consecutive bytes of an output row (single bytes when rows are not dword
//                       multiples): every tap is one coalesced dword row read, rows outside the frame read 0.
//   copy_kernel         both passes skipped: the applied frames are copied.
//   nearest_kernel      a thread is one output pixel: one 4-byte copy through the two index tables.
//   seg_boxes kernels   a workgroup reduces kSegChunk pixels into per-slot min / max / count in the LDS (integer atomics), then one
//                       global integer atomic per touched slot and field.
// Integer arithmetic and copies only: results are bit-identical from run to run and do not depend on the other images.
#include <algorithm>
#include <climits>

#include "common.h"

namespace hp {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 256;           // output pixels per workgroup of resize_rows_kernel (one per thread)
constexpr int kRowsPerGroup = 4;     // source rows per workgroup of resize_rows_kernel
constexpr int kMaxBand = 12288;      // pixels: the longest band resize_rows_kernel stages (36 KiB + 8 bytes of LDS)
constexpr int kMaxTaps = 4096;       // the longest window (entries per output index of a weight table)
constexpr int kPrecisionBits = 22;   // Pillow's 8-bit weights: 32 - 8 - 2 fractional bits
constexpr int kMaxIds = 256;         // hp_seg_boxes: slots per image
constexpr int kSegChunk = 2048;      // hp_seg_boxes: pixels per workgroup (8 per thread)
constexpr int64_t kMaxPixels = int64_t(1) << 28;

__device__ inline uint8_t clip8(int32_t acc) {
  const int32_t v = acc >> kPrecisionBits;  // arithmetic shift: floor, as Pillow's look-up table
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// bounds of the rows the pass along y reads for this table: rows outside need no pass along x
__device__ inline void used_rows(const int32_t* __restrict__ yb, int out_h, int ks_y, int& lo, int& hi) {
  lo = yb[0];
  hi = yb[2 * (out_h - 1)] + min(max(yb[2 * (out_h - 1) + 1], 0), ks_y);
}

// d_in [B][in_h][in_w][3] -> d_dst [B][in_h][out_w][3]; grid (tiles of out_w, groups of rows, B)
__global__ __launch_bounds__(kThreads) void resize_rows_kernel(const uint8_t* __restrict__ d_in, const int32_t* __restrict__ d_table_of,
                                                               int n_tables, const int32_t* __restrict__ d_xb,
                                                               const int32_t* __restrict__ d_xw, int ks_x,
                                                               const int32_t* __restrict__ d_yb, int ks_y, int out_h,
                                                               const uint8_t* __restrict__ d_apply, uint8_t* __restrict__ d_dst,
                                                               int in_h, int in_w, int out_w, int band, int64_t in_bytes) {
  extern __shared__ __align__(16) uint8_t s_mem[];  // [4 * ceil((3 band + 3) / 4)] the band, then [3 kTile] the tile's results
  const int b = blockIdx.z;
  if (!d_apply[b]) return;
  const int t = d_table_of[b];
  if (t < 0 || t >= n_tables) return;
  const int band_bytes = (3 * band + 3 + 3) / 4 * 4;
  uint8_t* s_band = s_mem;
  uint8_t* s_out = s_mem + band_bytes;
  const int32_t* __restrict__ xb = d_xb + 2 * (int64_t)t * out_w;
  const int32_t* __restrict__ xw = d_xw + (int64_t)t * out_w * ks_x;
  const int x0 = blockIdx.x * kTile, x1 = min(x0 + kTile, out_w);
  int row_lo = 0, row_hi = in_h;
  if (d_yb) used_rows(d_yb + 2 * (int64_t)t * out_h, out_h, ks_y, row_lo, row_hi);
  // the source pixels [lo, hi) the tile's windows cover, cut to the frame and to the band
  const int last_n = min(max(xb[2 * (x1 - 1) + 1], 0), ks_x);
  const int lo = min(max(xb[2 * x0], 0), in_w);
  const int hi = min(min(max(xb[2 * (x1 - 1)] + last_n, lo), in_w), lo + band);
  const int x = x0 + (int)threadIdx.x;
  int xmin = 0, n = 0;
  if (x < x1) xmin = xb[2 * x], n = min(max(xb[2 * x + 1], 0), ks_x);
  const int32_t* __restrict__ wk = xw + (int64_t)x * ks_x;
  const bool dwords = (reinterpret_cast<uintptr_t>(d_in) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_dst) & 3) == 0;
  for (int r = 0; r < kRowsPerGroup; ++r) {
    const int y = blockIdx.y * kRowsPerGroup + r;
    if (y >= in_h) break;              // uniform
    if (y < row_lo || y >= row_hi) continue;  // uniform
    const int64_t g0 = (((int64_t)b * in_h + y) * in_w + lo) * 3, g1 = g0 + 3 * (int64_t)(hi - lo);  // the band's bytes
    const int64_t a0 = dwords ? (g0 & ~(int64_t)3) : g0;
    const int shift = (int)(g0 - a0);
    if (dwords) {
      const int n_dw = (int)((g1 - a0 + 3) / 4);
      for (int i = threadIdx.x; i < n_dw; i += kThreads) {
        const int64_t a = a0 + 4 * (int64_t)i;
        uint32_t v = 0;
        if (a + 4 <= in_bytes) {
          v = *reinterpret_cast<const uint32_t*>(d_in + a);
        } else {
          for (int k = 0; k < 4; ++k)
            if (a + k < in_bytes) v |= (uint32_t)d_in[a + k] << (8 * k);
        }
        *reinterpret_cast<uint32_t*>(s_band + 4 * i) = v;
      }
    } else {
      for (int i = threadIdx.x; i < (int)(g1 - g0); i += kThreads) s_band[i] = d_in[g0 + i];
    }
    __syncthreads();
    if (x < x1) {
      int32_t acc0 = 1 << (kPrecisionBits - 1), acc1 = acc0, acc2 = acc0;
      for (int k = 0; k < n; ++k) {
        const int sx = xmin + k;
        if (sx >= lo && sx < hi) {
          const int32_t w = wk[k];
          const uint8_t* p = s_band + shift + 3 * (sx - lo);
          acc0 += w * (int32_t)p[0], acc1 += w * (int32_t)p[1], acc2 += w * (int32_t)p[2];
        }
      }
      uint8_t* q = s_out + 3 * (int)threadIdx.x;
      q[0] = clip8(acc0), q[1] = clip8(acc1), q[2] = clip8(acc2);
    }
    __syncthreads();
    // the tile's bytes [o0, o1) of d_dst: whole dwords in the middle, single bytes at the two ends
    const int64_t o0 = (((int64_t)b * in_h + y) * out_w + x0) * 3, o1 = o0 + 3 * (int64_t)(x1 - x0);
    const int64_t up = (o0 + 3) & ~(int64_t)3, down = o1 & ~(int64_t)3;
    const int64_t m0 = dwords ? (up < o1 ? up : o1) : o1, m1 = dwords ? (down > m0 ? down : m0) : o1;
    for (int i = threadIdx.x; i < (int)((m1 - m0) / 4); i += kThreads) {
      const uint8_t* p = s_out + (m0 - o0) + 4 * i;
      *reinterpret_cast<uint32_t*>(d_dst + m0 + 4 * (int64_t)i) =
          (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
    const int head = (int)(m0 - o0), tail = (int)(o1 - m1);
    for (int i = threadIdx.x; i < head; i += kThreads) d_dst[o0 + i] = s_out[i];
    for (int i = threadIdx.x; i < tail; i += kThreads) d_dst[m1 + i] = s_out[(m1 - o0) + i];
    __syncthreads();
  }
}

// d_src [B][in_h][row_bytes] -> d_out [B][out_h][row_bytes]; VEC: a thread is one dword of the row (row_bytes % 4 == 0, aligned)
template <bool VEC>
__global__ __launch_bounds__(kThreads) void resize_cols_kernel(const uint8_t* __restrict__ d_src, const int32_t* __restrict__ d_table_of,
                                                               int n_tables, const int32_t* __restrict__ d_yb,
                                                               const int32_t* __restrict__ d_yw, int ks_y,
                                                               const uint8_t* __restrict__ d_apply, uint8_t* __restrict__ d_out,
                                                               int in_h, int out_h, int row_bytes) {
  const int b = blockIdx.z, y = blockIdx.y;
  if (!d_apply[b]) return;
  const int t = d_table_of[b];
  if (t < 0 || t >= n_tables) return;
  const int item = blockIdx.x * kThreads + threadIdx.x;
  const int col = VEC ? 4 * item : item;
  if (col >= row_bytes) return;
  const int32_t* __restrict__ yb = d_yb + 2 * ((int64_t)t * out_h + y);
  const int32_t* __restrict__ wk = d_yw + ((int64_t)t * out_h + y) * ks_y;
  const int ymin = yb[0], n = min(max(yb[1], 0), ks_y);
  const uint8_t* __restrict__ src = d_src + (int64_t)b * in_h * row_bytes + col;
  int32_t acc[VEC ? 4 : 1];
#pragma unroll
  for (int j = 0; j < (VEC ? 4 : 1); ++j) acc[j] = 1 << (kPrecisionBits - 1);
  for (int k = 0; k < n; ++k) {
    const int sy = ymin + k;
    if (sy < 0 || sy >= in_h) continue;  // uniform: a row outside the frame is 0
    const int32_t w = wk[k];
    if (VEC) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(src + (int64_t)sy * row_bytes);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += w * (int32_t)((v >> (8 * j)) & 0xffu);
    } else {
      acc[0] += w * (int32_t)src[(int64_t)sy * row_bytes];
    }
  }
  uint8_t* dst = d_out + ((int64_t)b * out_h + y) * row_bytes + col;
  if (VEC) {
    *reinterpret_cast<uint32_t*>(dst) =
        (uint32_t)clip8(acc[0]) | ((uint32_t)clip8(acc[1]) << 8) | ((uint32_t)clip8(acc[2]) << 16) | ((uint32_t)clip8(acc[3]) << 24);
  } else {
    *dst = clip8(acc[0]);
  }
}

__global__ __launch_bounds__(kThreads) void copy_kernel(const uint8_t* __restrict__ d_in, const uint8_t* __restrict__ d_apply,
                                                        uint8_t* __restrict__ d_out, int64_t bytes) {
  const int b = blockIdx.y;
  if (!d_apply[b]) return;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < bytes) d_out[b * bytes + i] = d_in[b * bytes + i];
}

__global__ __launch_bounds__(kThreads) void nearest_kernel(const uint32_t* __restrict__ d_in, const int32_t* __restrict__ d_table_of,
                                                           int n_tables, const int32_t* __restrict__ d_xi,
                                                           const int32_t* __restrict__ d_yi, const uint8_t* __restrict__ d_apply,
                                                           uint32_t* __restrict__ d_out, int in_h, int in_w, int out_h, int out_w) {
  const int b = blockIdx.y;
  if (!d_apply[b]) return;
  const int t = d_table_of[b];
  if (t < 0 || t >= n_tables) return;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)out_h * out_w) return;
  const int y = (int)(i / out_w), x = (int)(i - (int64_t)y * out_w);
  const int sx = d_xi[(int64_t)t * out_w + x], sy = d_yi[(int64_t)t * out_h + y];
  uint32_t v = 0;  // outside the frame: Pillow leaves the new image's 0
  if (sx >= 0 && sx < in_w && sy >= 0 && sy < in_h) v = d_in[((int64_t)b * in_h + sy) * in_w + sx];
  d_out[(int64_t)b * out_h * out_w + i] = v;
}

__global__ __launch_bounds__(kThreads) void seg_boxes_init_kernel(int32_t* __restrict__ d_boxes, int32_t* __restrict__ d_n_px, int n) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  d_boxes[4 * i + 0] = INT_MAX, d_boxes[4 * i + 1] = INT_MAX, d_boxes[4 * i + 2] = -1, d_boxes[4 * i + 3] = -1;
  d_n_px[i] = 0;
}

// grid (chunks of kSegChunk pixels, B)
__global__ __launch_bounds__(kThreads) void seg_boxes_kernel(const int32_t* __restrict__ d_seg, const int32_t* __restrict__ d_ids,
                                                             const int32_t* __restrict__ d_count, int max_ids,
                                                             int32_t* __restrict__ d_boxes, int32_t* __restrict__ d_n_px, int h, int w) {
  __shared__ int32_t s_id[kMaxIds], s_x1[kMaxIds], s_y1[kMaxIds], s_x2[kMaxIds], s_y2[kMaxIds], s_n[kMaxIds];
  const int b = blockIdx.y;
  const int count = min(max(d_count[b], 0), max_ids);
  if (count == 0) return;
  for (int k = threadIdx.x; k < count; k += kThreads)
    s_id[k] = d_ids[(int64_t)b * max_ids + k], s_x1[k] = INT_MAX, s_y1[k] = INT_MAX, s_x2[k] = -1, s_y2[k] = -1, s_n[k] = 0;
  __syncthreads();
  const int hw = h * w;
  const int p_end = min((int)(blockIdx.x + 1) * kSegChunk, hw);
  const int32_t* __restrict__ seg = d_seg + (int64_t)b * hw;
  for (int p = blockIdx.x * kSegChunk + threadIdx.x; p < p_end; p += kThreads) {
    const int32_t v = seg[p];
    int slot = -1;
    for (int k = 0; k < count; ++k)  // the first slot that names the value
      if (s_id[k] == v) {
        slot = k;
        break;
      }
    if (slot >= 0) {
      const int y = p / w, x = p - y * w;
      atomicMin(&s_x1[slot], x), atomicMin(&s_y1[slot], y), atomicMax(&s_x2[slot], x), atomicMax(&s_y2[slot], y);
      atomicAdd(&s_n[slot], 1);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < count; k += kThreads)
    if (s_n[k] > 0) {
      int32_t* box = d_boxes + 4 * ((int64_t)b * max_ids + k);
      atomicMin(box + 0, s_x1[k]), atomicMin(box + 1, s_y1[k]), atomicMax(box + 2, s_x2[k]), atomicMax(box + 3, s_y2[k]);
      atomicAdd(d_n_px + (int64_t)b * max_ids + k, s_n[k]);
    }
}

inline int64_t tmp_bytes(int B, int in_h, int out_w) { return round_up((int64_t)B * in_h * out_w * 3, 8); }

}  // namespace
}  // namespace hp

using namespace hp;

#define HP_RESIZE_DIMS(name)                                                                                                   \
  HP_REQUIRE(B >= 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0, name ": B >= 0 and positive sizes");                      \
  HP_REQUIRE(B <= 65535 && (int64_t)in_h * in_w <= kMaxPixels && (int64_t)out_h * out_w <= kMaxPixels && in_h <= 65535 * kRowsPerGroup && \
                 out_h <= 65535,                                                                                               \
             name ": at most 65535 images of 2^28 pixels and 65535 output rows");                                              \
  if (B == 0) return HP_OK

extern "C" int64_t hp_resize_workspace_bytes(int B, int in_h, int out_w) {
  if (B < 0 || B > 65535 || in_h <= 0 || out_w <= 0 || (int64_t)in_h * out_w > kMaxPixels) return -1;
  return tmp_bytes(B, in_h, out_w);
}

extern "C" int hp_resize_rgb(int B, int in_h, int in_w, int out_h, int out_w, const uint8_t* d_in, int n_tables,
                             const int32_t* d_table_of, const int32_t* d_xbounds, const int32_t* d_xweights, int ksize_x, int band_x,
                             const int32_t* d_ybounds, const int32_t* d_yweights, int ksize_y, const uint8_t* d_apply,
                             uint8_t* d_out, void* d_workspace, int64_t workspace_bytes, void* stream) {
  HP_RESIZE_DIMS("hp_resize_rgb");
  HP_REQUIRE(d_in && d_table_of && d_apply && d_out, "hp_resize_rgb: null pointer");
  HP_REQUIRE(d_in != d_out, "hp_resize_rgb: d_out must not alias d_in");
  HP_REQUIRE(n_tables >= 1 && n_tables <= B, "hp_resize_rgb: 1 <= n_tables <= B");
  const bool pass_x = ksize_x > 0, pass_y = ksize_y > 0;
  HP_REQUIRE(ksize_x >= 0 && ksize_y >= 0 && ksize_x <= kMaxTaps && ksize_y <= kMaxTaps, "hp_resize_rgb: a window of 0 .. 4096 taps");
  HP_REQUIRE(!pass_x || (d_xbounds && d_xweights), "hp_resize_rgb: the pass along x needs d_xbounds and d_xweights");
  HP_REQUIRE(!pass_y || (d_ybounds && d_yweights), "hp_resize_rgb: the pass along y needs d_ybounds and d_yweights");
  HP_REQUIRE(pass_x || out_w == in_w, "hp_resize_rgb: ksize_x == 0 (pass skipped) needs out_w == in_w");
  HP_REQUIRE(pass_y || out_h == in_h, "hp_resize_rgb: ksize_y == 0 (pass skipped) needs out_h == in_h");
  HP_REQUIRE(!pass_x || (band_x >= 1 && band_x <= kMaxBand), "hp_resize_rgb: band_x must be 1 .. 12288 pixels");
  hipStream_t st = (hipStream_t)stream;
  const int64_t in_bytes = (int64_t)B * in_h * in_w * 3;
  if (!pass_x && !pass_y) {
    const int64_t bytes = (int64_t)in_h * in_w * 3;
    hipLaunchKernelGGL(copy_kernel, dim3((unsigned)((bytes + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads), 0, st, d_in, d_apply,
                       d_out, bytes);
    return check_launch("hp_resize_rgb (copy)");
  }
  uint8_t* tmp = d_out;  // the pass along x writes the result itself when there is no pass along y
  if (pass_x && pass_y) {
    HP_REQUIRE(d_workspace && workspace_bytes >= tmp_bytes(B, in_h, out_w), "hp_resize_rgb: workspace smaller than hp_resize_workspace_bytes");
    tmp = static_cast<uint8_t*>(d_workspace);
  }
  if (pass_x) {
    const int band_bytes = (3 * band_x + 3 + 3) / 4 * 4;
    const dim3 grid((unsigned)((out_w + kTile - 1) / kTile), (unsigned)((in_h + kRowsPerGroup - 1) / kRowsPerGroup), (unsigned)B);
    hipLaunchKernelGGL(resize_rows_kernel, grid, dim3(kThreads), (size_t)(band_bytes + 3 * kTile), st, d_in, d_table_of, n_tables, d_xbounds,
                       d_xweights, ksize_x, pass_y ? d_ybounds : (const int32_t*)nullptr, ksize_y, out_h, d_apply, tmp, in_h, in_w, out_w,
                       band_x, in_bytes);
    if (int rc = check_launch("hp_resize_rgb (rows)")) return rc;
  }
  if (pass_y) {
    const uint8_t* src = pass_x ? tmp : d_in;
    const int row_bytes = 3 * out_w;
    const bool vec = row_bytes % 4 == 0 && aligned(src, 4) && aligned(d_out, 4);
    const int items = vec ? row_bytes / 4 : row_bytes;
    const dim3 grid((unsigned)((items + kThreads - 1) / kThreads), (unsigned)out_h, (unsigned)B);
    if (vec)
      hipLaunchKernelGGL(resize_cols_kernel<true>, grid, dim3(kThreads), 0, st, src, d_table_of, n_tables, d_ybounds, d_yweights, ksize_y,
                         d_apply, d_out, in_h, out_h, row_bytes);
    else
      hipLaunchKernelGGL(resize_cols_kernel<false>, grid, dim3(kThreads), 0, st, src, d_table_of, n_tables, d_ybounds, d_yweights, ksize_y,
                         d_apply, d_out, in_h, out_h, row_bytes);
    return check_launch("hp_resize_rgb (columns)");
  }
  return HP_OK;
}

extern "C" int hp_resize_nearest(int B, int in_h, int in_w, int out_h, int out_w, const void* d_in, int n_tables,
                                 const int32_t* d_table_of, const int32_t* d_xindex, const int32_t* d_yindex, const uint8_t* d_apply,
                                 void* d_out, void* stream) {
  HP_RESIZE_DIMS("hp_resize_nearest");
  HP_REQUIRE(d_in && d_table_of && d_xindex && d_yindex && d_apply && d_out, "hp_resize_nearest: null pointer");
  HP_REQUIRE(d_in != d_out, "hp_resize_nearest: d_out must not alias d_in");
  HP_REQUIRE(n_tables >= 1 && n_tables <= B, "hp_resize_nearest: 1 <= n_tables <= B");
  const int64_t n = (int64_t)out_h * out_w;
  hipLaunchKernelGGL(nearest_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream,
                     static_cast<const uint32_t*>(d_in), d_table_of, n_tables, d_xindex, d_yindex, d_apply, static_cast<uint32_t*>(d_out),
                     in_h, in_w, out_h, out_w);
  return check_launch("hp_resize_nearest");
}

extern "C" int hp_seg_boxes(int B, int h, int w, const int32_t* d_segmentation, const int32_t* d_ids, const int32_t* d_count,
                            int max_ids, int32_t* d_boxes, int32_t* d_n_px, void* stream) {
  HP_REQUIRE(B >= 0 && h > 0 && w > 0, "hp_seg_boxes: B >= 0, h > 0 and w > 0");
  HP_REQUIRE(B <= 65535 && (int64_t)h * w <= kMaxPixels, "hp_seg_boxes: at most 65535 images of 2^28 pixels");
  HP_REQUIRE(max_ids >= 1 && max_ids <= kMaxIds, "hp_seg_boxes: max_ids must be 1 .. 256");
  if (B == 0) return HP_OK;
  HP_REQUIRE(d_segmentation && d_ids && d_count && d_boxes && d_n_px, "hp_seg_boxes: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int n = B * max_ids;
  hipLaunchKernelGGL(seg_boxes_init_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_boxes, d_n_px, n);
  if (int rc = check_launch("hp_seg_boxes (init)")) return rc;
  const int64_t hw = (int64_t)h * w;
  hipLaunchKernelGGL(seg_boxes_kernel, dim3((unsigned)((hw + kSegChunk - 1) / kSegChunk), (unsigned)B), dim3(kThreads), 0, st,
                     d_segmentation, d_ids, d_count, max_ids, d_boxes, d_n_px, h, w);
  return check_launch("hp_seg_boxes");
}
