// Multi-object scenes on top of the one-object-per-view rasteriser: entry points and the reference lines they replace are in
// include/happypose_amd.h (hp_scene_*).
//
// A scene is rendered as LAYERS -- one hp_rasterize view per (camera, object) pair, sorted by camera -- that the kernels here merge:
//   compose_kernel     per pixel the layer of the camera with the smallest depth > 0 (strict <, ascending layer: the lowest layer on
//                      a tie); colour, normals and depth are COPIES of the winner's values, so every output is a bit-exact function
//                      of the layers.  All depth planes of a camera are read, colour and normals of the winner only: about
//                      4 K + 28 bytes per pixel for K layers instead of 28 K.  One thread owns 4 consecutive pixels of the flattened
//                      H x W plane (16-byte loads and stores when H * W is a multiple of 4 and every buffer is 16-byte aligned; the
//                      scalar instantiation covers everything else, tail included).
//   visibility_*       per layer px_count_all / px_count_visib and the two inclusive bounding boxes: integer wave reduction, one LDS
//                      step across the wavefronts, then integer add / min / max atomics into a table the init kernel has written.
//                      Integers only: the table does not depend on the order in which workgroups arrive.
//   contour_kernel     this repository's outline definition (header) in one launch: a tile of labels with a halo of
//                      dilate_iterations + 1 in LDS, the undilated edge on the tile + dilate_iterations, then the dilation.
//   overlay_kernel     BokehPlotter.plot_overlay: each branch is a function of one byte, read from a 256-entry table.
//
// LIMITATION.  Every layer is resolved on its own, 4x multisampled against BLACK.  Where the silhouette of a nearer
// object crosses a farther one the edge pixels of the nearer layer therefore blend with black, not with the object behind; the band
// is at most one pixel wide.  Depth, ids, mask and the visibility table are exact, and in the single-sample state (no
// HP_RASTER_MSAA4) the colour too is exactly what one shared z-buffer gives.  A multi-object rasteriser pass is out of scope.
#include "common.h"
#include "wave.h"

namespace hp {
namespace {

constexpr int kThreads = 256;
constexpr int kVisRows = 16;       // image rows per visibility workgroup (4 wavefronts, 4 rows each)
constexpr int kTileW = 64, kTileH = 4;  // contour tile: one wavefront per row
constexpr int kMaxDilate = HP_SCENE_MAX_DILATE;
constexpr int kHalo = kMaxDilate + 1;
constexpr int kOutside = INT32_MIN;  // label of a position outside the image: never a neighbour, never an edge

struct LayerRange {
  int begin, end;
};

// the camera's layer range, clamped into [0, n_layers]: a corrupt offset table reads nothing outside the layer buffers
__device__ inline LayerRange layer_range(const int32_t* __restrict__ off, int cam, int n_layers) {
  LayerRange r;
  r.begin = min(max(off[cam], 0), n_layers);
  r.end = min(max(off[cam + 1], r.begin), n_layers);
  return r;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads)
compose_kernel(const int32_t* __restrict__ layer_off, int n_layers, int64_t P, const float* __restrict__ l_rgb,
               const float* __restrict__ l_nrm, const float* __restrict__ l_depth, float* __restrict__ o_rgb, float* __restrict__ o_nrm,
               float* __restrict__ o_depth, int32_t* __restrict__ o_ids, uint8_t* __restrict__ o_mask) {
  const int cam = blockIdx.y;
  const int64_t p0 = 4 * ((int64_t)blockIdx.x * kThreads + threadIdx.x);
  if (p0 >= P) return;
  const int n = VEC ? 4 : (int)min((int64_t)4, P - p0);
  const LayerRange lr = layer_range(layer_off, cam, n_layers);
  float best[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
  int win[4] = {-1, -1, -1, -1};
  for (int l = lr.begin; l < lr.end; ++l) {
    const float* d = l_depth + (int64_t)l * P + p0;
    float v[4];
    if (VEC) {
      const float4 q = *reinterpret_cast<const float4*>(d);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = i < n ? d[i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (v[i] > 0.f && v[i] < best[i]) {  // NaN and +inf never win; strict <: the lowest layer on a tie
        best[i] = v[i];
        win[i] = l;
      }
    }
  }
  const bool same = win[0] == win[1] && win[0] == win[2] && win[0] == win[3];
  // depth / ids / mask
  {
    float dv[4];
    int iv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      dv[i] = win[i] >= 0 ? best[i] : 0.f;
      iv[i] = win[i] >= 0 ? win[i] - lr.begin : -1;
    }
    float* od = o_depth + (int64_t)cam * P + p0;
    int32_t* oi = o_ids + (int64_t)cam * P + p0;
    uint8_t* om = o_mask + (int64_t)cam * P + p0;
    if (VEC) {
      *reinterpret_cast<float4*>(od) = make_float4(dv[0], dv[1], dv[2], dv[3]);
      *reinterpret_cast<int4*>(oi) = make_int4(iv[0], iv[1], iv[2], iv[3]);
      *reinterpret_cast<uint32_t*>(om) = (win[0] >= 0 ? 1u : 0u) | (win[1] >= 0 ? 1u << 8 : 0u) | (win[2] >= 0 ? 1u << 16 : 0u) |
                                         (win[3] >= 0 ? 1u << 24 : 0u);
    } else {
      for (int i = 0; i < n; ++i) {
        od[i] = dv[i];
        oi[i] = iv[i];
        om[i] = win[i] >= 0 ? 1 : 0;
      }
    }
  }
  // colour and normals: the winner's values, copied
#pragma unroll
  for (int buf = 0; buf < 2; ++buf) {
    const float* src = buf ? l_nrm : l_rgb;
    float* dst = buf ? o_nrm : o_rgb;
    if (!dst) continue;  // normals not asked for (uniform); without layers nothing wins and src is never read
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = dst + ((int64_t)cam * 3 + c) * P + p0;
      if (VEC && same) {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (win[0] >= 0) q = *reinterpret_cast<const float4*>(src + ((int64_t)win[0] * 3 + c) * P + p0);
        *reinterpret_cast<float4*>(o) = q;
      } else {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (i < n && win[i] >= 0) ? src[((int64_t)win[i] * 3 + c) * P + p0 + i] : 0.f;
        if (VEC) {
          *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
          for (int i = 0; i < n; ++i) o[i] = v[i];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- visibility
// table row: {px_count_all, px_count_visib, all: x_min y_min x_max y_max, visib: x_min y_min x_max y_max}.  Empty boxes are -1:
// the maxima start at -1 and grow by signed atomicMax; the minima start at -1 too, which is the LARGEST value of an unsigned
// atomicMin, so an untouched minimum stays -1 and no finishing pass is needed.
__global__ void __launch_bounds__(kThreads) visibility_init_kernel(int n, int32_t* __restrict__ table) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) table[i] = (i % HP_SCENE_VIS_FIELDS) < 2 ? 0 : -1;
}

__global__ void __launch_bounds__(kThreads)
visibility_kernel(int n_cam, const int32_t* __restrict__ layer_off, int n_layers, int H, int W, const float* __restrict__ l_depth,
                  const int32_t* __restrict__ ids, int32_t* __restrict__ table) {
  __shared__ int s_red[kThreads / kWave][HP_SCENE_VIS_FIELDS];
  const int layer = blockIdx.y;
  int cam = -1, local = 0;
  for (int c = 0; c < n_cam; ++c) {  // uniform: the camera whose (clamped) range holds this layer
    const LayerRange lr = layer_range(layer_off, c, n_layers);
    if (layer >= lr.begin && layer < lr.end) {
      cam = c;
      local = layer - lr.begin;
      break;
    }
  }
  if (cam < 0) return;  // a layer no camera owns keeps its empty row
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int y0 = blockIdx.x * kVisRows, y1 = min(y0 + kVisRows, H);
  const float* d = l_depth + (int64_t)layer * H * W;
  const int32_t* id = ids + (int64_t)cam * H * W;
  // acc: counts, then (x_min, y_min, x_max, y_max) twice; minima as INT_MAX until something is seen
  int acc[HP_SCENE_VIS_FIELDS] = {0, 0, INT32_MAX, INT32_MAX, -1, -1, INT32_MAX, INT32_MAX, -1, -1};
  for (int y = y0 + wave; y < y1; y += kThreads / kWave) {
    for (int x = lane; x < W; x += kWave) {
      const int64_t p = (int64_t)y * W + x;
      const bool all = d[p] > 0.f, vis = id[p] == local;
      if (all) {
        ++acc[0];
        acc[2] = min(acc[2], x), acc[3] = min(acc[3], y), acc[4] = max(acc[4], x), acc[5] = max(acc[5], y);
      }
      if (vis) {
        ++acc[1];
        acc[6] = min(acc[6], x), acc[7] = min(acc[7], y), acc[8] = max(acc[8], x), acc[9] = max(acc[9], y);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < HP_SCENE_VIS_FIELDS; ++k) {
    const bool is_min = k == 2 || k == 3 || k == 6 || k == 7;
    acc[k] = k < 2 ? wave_sum(acc[k]) : (is_min ? wave_min(acc[k]) : wave_max(acc[k]));
    if (lane == 0) s_red[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < HP_SCENE_VIS_FIELDS) {
    const int k = threadIdx.x;
    const bool is_min = k == 2 || k == 3 || k == 6 || k == 7;
    int v = s_red[0][k];
    for (int w = 1; w < kThreads / kWave; ++w) {
      const int u = s_red[w][k];
      v = k < 2 ? v + u : (is_min ? min(v, u) : max(v, u));
    }
    int32_t* t = table + (int64_t)layer * HP_SCENE_VIS_FIELDS + k;
    if (k < 2) {
      if (v) atomicAdd(t, v);
    } else if (is_min) {
      if (v != INT32_MAX) atomicMin(reinterpret_cast<unsigned int*>(t), (unsigned int)v);  // v >= 0; the initial -1 is UINT_MAX
    } else {
      if (v >= 0) atomicMax(t, v);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- contour
__global__ void __launch_bounds__(kThreads)
contour_kernel(int H, int W, const uint8_t* __restrict__ frame, const uint8_t* __restrict__ mask, const int32_t* __restrict__ ids,
               int per_object, int cr, int cg, int cb, int dil, uint8_t* __restrict__ out, uint8_t* __restrict__ edge_out) {
  __shared__ int s_lab[kTileH + 2 * kHalo][kTileW + 2 * kHalo];
  __shared__ uint8_t s_edge[kTileH + 2 * kMaxDilate][kTileW + 2 * kMaxDilate];
  const int cam = blockIdx.z;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const int64_t plane = (int64_t)cam * H * W;
  const int halo = dil + 1;
  // labels of the tile and a halo of dil + 1: >= 0 inside an object (0 in mask mode), -1 background, kOutside off the image
  const int lw = kTileW + 2 * halo, lh = kTileH + 2 * halo;
  for (int i = threadIdx.x; i < lw * lh; i += kThreads) {
    const int ly = i / lw, lx = i - ly * lw;
    const int x = x0 + lx - halo, y = y0 + ly - halo;
    int lab = kOutside;
    if (x >= 0 && x < W && y >= 0 && y < H) {
      const int64_t p = plane + (int64_t)y * W + x;
      if (mask)
        lab = mask[p] ? 0 : -1;
      else
        lab = per_object ? max(ids[p], -1) : (ids[p] >= 0 ? 0 : -1);
    }
    s_lab[ly][lx] = lab;
  }
  __syncthreads();
  // edge0 on the tile and a halo of dil: inside, and a 4-neighbour inside the image carries another label
  const int ew = kTileW + 2 * dil, eh = kTileH + 2 * dil;
  for (int i = threadIdx.x; i < ew * eh; i += kThreads) {
    const int ey = i / ew, ex = i - ey * ew;
    const int ly = ey + 1, lx = ex + 1;  // the same position in s_lab (its halo is one wider)
    const int c = s_lab[ly][lx];
    bool e = false;
    if (c >= 0) {
      const int nb[4] = {s_lab[ly][lx - 1], s_lab[ly][lx + 1], s_lab[ly - 1][lx], s_lab[ly + 1][lx]};
#pragma unroll
      for (int k = 0; k < 4; ++k) e = e || (nb[k] != kOutside && nb[k] != c);
    }
    s_edge[ey][ex] = e ? 1 : 0;
  }
  __syncthreads();
  const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  bool e = false;
  for (int dy = 0; dy <= 2 * dil; ++dy)
    for (int dx = 0; dx <= 2 * dil; ++dx) e = e || s_edge[ty + dy][tx + dx];
  const int64_t p = plane + (int64_t)y * W + x;
  out[3 * p] = e ? (uint8_t)cr : frame[3 * p];
  out[3 * p + 1] = e ? (uint8_t)cg : frame[3 * p + 1];
  out[3 * p + 2] = e ? (uint8_t)cb : frame[3 * p + 2];
  if (edge_out) edge_out[p] = e ? 255 : 0;
}

// ------------------------------------------------------------------------------------------------------------------- overlay
__global__ void __launch_bounds__(kThreads)
overlay_kernel(int64_t n_px, const uint8_t* __restrict__ input, const uint8_t* __restrict__ render, const uint8_t* __restrict__ mask,
               const uint8_t* __restrict__ lut_render, const uint8_t* __restrict__ lut_input, uint8_t* __restrict__ out) {
  __shared__ uint8_t s_lut[2][256];
  s_lut[0][threadIdx.x] = lut_input[threadIdx.x];  // kThreads == 256
  s_lut[1][threadIdx.x] = lut_render[threadIdx.x];
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n_px) return;
  const uint8_t r0 = render[3 * p], r1 = render[3 * p + 1], r2 = render[3 * p + 2];
  const bool m = mask ? mask[p] != 0 : (r0 | r1 | r2) != 0;
  out[3 * p] = m ? s_lut[1][r0] : s_lut[0][input[3 * p]];
  out[3 * p + 1] = m ? s_lut[1][r1] : s_lut[0][input[3 * p + 1]];
  out[3 * p + 2] = m ? s_lut[1][r2] : s_lut[0][input[3 * p + 2]];
}

static_assert(kThreads == 256 && kTileW * kTileH == kThreads, "overlay tables and contour tiles are one entry per thread");

// shared shape checks: sizes the 64-bit pixel arithmetic and the launch grids hold
inline const char* check_frame(int n_cam, int h, int w) {
  if (n_cam < 0) return "negative n_cam";
  if (h < 1 || w < 1) return "h and w must be positive";
  if (n_cam > 65535) return "more than 65535 cameras in one call";
  if ((int64_t)h * w >= (int64_t(1) << 31)) return "frame of 2^31 pixels or more";
  return nullptr;
}

}  // namespace
}  // namespace hp

using namespace hp;

extern "C" int hp_scene_compose(int n_cam, const int32_t* d_layer_off, int n_layers, int h, int w, const float* d_layer_rgb,
                                const float* d_layer_nrm, const float* d_layer_depth, float* d_rgb, float* d_nrm, float* d_depth,
                                int32_t* d_ids, uint8_t* d_mask, void* stream) {
  if (const char* e = check_frame(n_cam, h, w)) return fail(HP_ERR_ARG, std::string("hp_scene_compose: ") + e);
  HP_REQUIRE(n_layers >= 0, "hp_scene_compose: negative n_layers");
  if (n_cam == 0) return HP_OK;
  HP_REQUIRE(d_layer_off && d_rgb && d_depth && d_ids && d_mask, "hp_scene_compose: null pointer");
  HP_REQUIRE(n_layers == 0 || (d_layer_rgb && d_layer_depth), "hp_scene_compose: layer buffers missing");
  HP_REQUIRE(!d_nrm || d_layer_nrm || n_layers == 0, "hp_scene_compose: d_nrm needs d_layer_nrm");
  const int64_t P = (int64_t)h * w;
  const int64_t groups = (P + 3) / 4;
  const int64_t blocks = (groups + kThreads - 1) / kThreads;
  HP_REQUIRE(blocks < (int64_t(1) << 31), "hp_scene_compose: frame too large");
  const bool vec = P % 4 == 0 && aligned(d_layer_rgb, 16) && aligned(d_layer_nrm, 16) && aligned(d_layer_depth, 16) && aligned(d_rgb, 16) &&
                   aligned(d_nrm, 16) && aligned(d_depth, 16) && aligned(d_ids, 16) && aligned(d_mask, 16);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks, (unsigned)n_cam);
  if (vec)
    hipLaunchKernelGGL(compose_kernel<true>, grid, dim3(kThreads), 0, st, d_layer_off, n_layers, P, d_layer_rgb, d_layer_nrm, d_layer_depth,
                       d_rgb, d_nrm, d_depth, d_ids, d_mask);
  else
    hipLaunchKernelGGL(compose_kernel<false>, grid, dim3(kThreads), 0, st, d_layer_off, n_layers, P, d_layer_rgb, d_layer_nrm, d_layer_depth,
                       d_rgb, d_nrm, d_depth, d_ids, d_mask);
  return check_launch("hp_scene_compose");
}

extern "C" int hp_scene_visibility(int n_cam, const int32_t* d_layer_off, int n_layers, int h, int w, const float* d_layer_depth,
                                   const int32_t* d_ids, int32_t* d_table, void* stream) {
  if (const char* e = check_frame(n_cam, h, w)) return fail(HP_ERR_ARG, std::string("hp_scene_visibility: ") + e);
  HP_REQUIRE(n_layers >= 0 && n_layers <= 65535, "hp_scene_visibility: n_layers outside 0..65535");
  if (n_layers == 0) return HP_OK;
  HP_REQUIRE(d_layer_off && d_layer_depth && d_ids && d_table, "hp_scene_visibility: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int n = n_layers * HP_SCENE_VIS_FIELDS;
  hipLaunchKernelGGL(visibility_init_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, n, d_table);
  if (int rc = check_launch("hp_scene_visibility (init)")) return rc;
  if (n_cam == 0) return HP_OK;
  hipLaunchKernelGGL(visibility_kernel, dim3((h + kVisRows - 1) / kVisRows, n_layers), dim3(kThreads), 0, st, n_cam, d_layer_off,
                     n_layers, h, w, d_layer_depth, d_ids, d_table);
  return check_launch("hp_scene_visibility");
}

extern "C" int hp_scene_contour(int n_cam, int h, int w, const uint8_t* d_frame, const uint8_t* d_mask, const int32_t* d_ids,
                                int per_object, int color_r, int color_g, int color_b, int dilate_iterations, uint8_t* d_out,
                                uint8_t* d_edge, void* stream) {
  if (const char* e = check_frame(n_cam, h, w)) return fail(HP_ERR_ARG, std::string("hp_scene_contour: ") + e);
  HP_REQUIRE(dilate_iterations >= 0 && dilate_iterations <= kMaxDilate, "hp_scene_contour: dilate_iterations outside 0..3");
  HP_REQUIRE((unsigned)color_r < 256u && (unsigned)color_g < 256u && (unsigned)color_b < 256u, "hp_scene_contour: colour outside 0..255");
  HP_REQUIRE((d_mask != nullptr) != (d_ids != nullptr), "hp_scene_contour: exactly one of d_mask and d_ids");
  HP_REQUIRE(!per_object || d_ids, "hp_scene_contour: per_object needs d_ids");
  HP_REQUIRE(d_frame && d_out, "hp_scene_contour: null pointer");
  HP_REQUIRE(d_frame != d_out, "hp_scene_contour: d_out must not be d_frame");
  if (n_cam == 0) return HP_OK;
  const int gy = (h + kTileH - 1) / kTileH;
  HP_REQUIRE(gy <= 65535, "hp_scene_contour: frame too tall");
  hipLaunchKernelGGL(contour_kernel, dim3((w + kTileW - 1) / kTileW, gy, n_cam), dim3(kThreads), 0, (hipStream_t)stream, h, w, d_frame,
                     d_mask, d_ids, per_object ? 1 : 0, color_r, color_g, color_b, dilate_iterations, d_out, d_edge);
  return check_launch("hp_scene_contour");
}

extern "C" int hp_scene_overlay(int n_cam, int h, int w, const uint8_t* d_input, const uint8_t* d_render, const uint8_t* d_mask,
                                const uint8_t* d_lut_render, const uint8_t* d_lut_input, uint8_t* d_out, void* stream) {
  if (const char* e = check_frame(n_cam, h, w)) return fail(HP_ERR_ARG, std::string("hp_scene_overlay: ") + e);
  HP_REQUIRE(d_input && d_render && d_lut_render && d_lut_input && d_out, "hp_scene_overlay: null pointer");
  if (n_cam == 0) return HP_OK;
  const int64_t n_px = (int64_t)n_cam * h * w;
  const int64_t blocks = (n_px + kThreads - 1) / kThreads;
  HP_REQUIRE(blocks < (int64_t(1) << 31), "hp_scene_overlay: too many pixels in one call");
  hipLaunchKernelGGL(overlay_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, n_px, d_input, d_render, d_mask,
                     d_lut_render, d_lut_input, d_out);
  return check_launch("hp_scene_overlay");
}
