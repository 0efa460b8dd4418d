// Scoring 2D detections and instance masks: entry points and definitions are in include/happypose_amd.h (hp_mask_pack,
// hp_det_iou, hp_det_match).
//
//   pack_kernel<VEC>   a workgroup is one (mask, chunk of kChunkWords output words).  VEC: a thread loads 8 consecutive mask bytes
//                      (one 8-byte load, coalesced over the wavefront), folds them to 8 bits with two 32-bit multiplies, and the
//                      8 lanes of a word OR their bytes together with three xor-shuffles.  Scalar (plane size not a multiple of 8,
//                      or an unaligned base): lane i loads pixel 64 k + i and ONE ballot is word k.  Set pixels are counted with
//                      popcount, added over the wavefront and the LDS, and ONE integer atomic per workgroup lands in area[mask]
//                      (zeroed on the stream before the launch): integer addition, so the order does not matter.
//   box_iou_kernel     a thread per row.
//   mask_iou_kernel    a workgroup per row: 8-byte loads of both packed masks, popcount(a & b) per word, integer butterfly in the
//                      wavefront, one LDS step, thread 0 writes inter / union / IoU.  Nothing but integers is accumulated and a
//                      row is a function of its two masks alone (DESIGN.md 4.8 for why there is no LDS staging of a prediction).
//   match_kernel       a wavefront per (group, threshold): detections in order, lanes strided over the ground truths, the arg-max
//                      by a wave butterfly on (class, IoU, position).  Ground truth j is read AND marked by lane j % 64 only, so the
//                      matched flags need no fence.
#include "common.h"
#include "wave.h"

namespace hp {
namespace {

constexpr int kThreads = 256;
constexpr int kPackSteps = 4;                               // 8-byte groups per thread
constexpr int kChunkWords = kThreads * kPackSteps / 8;      // 128 words = 8192 pixels per workgroup
constexpr int64_t kMaxPlane = int64_t(1) << 24;             // every count is exact in float32

// sum over the workgroup, valid in thread 0
__device__ inline int block_add(int v, int* s_red) {
  v = wave_sum(v);
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  int r = 0;
  if (threadIdx.x == 0)
#pragma unroll
    for (int wv = 0; wv < kThreads / kWave; ++wv) r += s_red[wv];
  return r;
}

// 4 bytes -> 4 bits (bit j = byte j is non-zero).  t has bit 8 j set per non-zero byte; t * (2^7 + 2^14 + 2^21 + 2^28) moves bit
// 8 j to 28 + j (k = 4 - j), no two products share a bit position, and everything else lands below 28 or past 31.
__device__ inline uint32_t fold4(uint32_t x) {
  const uint32_t t = ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7) & 0x01010101u;
  return (t * 0x10204080u) >> 28;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) pack_kernel(const uint8_t* __restrict__ masks, int64_t P, int w64,
                                                        uint64_t* __restrict__ words, int32_t* __restrict__ area) {
  __shared__ int s_red[kThreads / kWave];
  const int m = blockIdx.x, chunk = blockIdx.y;
  const uint8_t* __restrict__ src = masks + (int64_t)m * P;
  uint64_t* __restrict__ dst = words + (int64_t)m * w64;
  const int lane = threadIdx.x % kWave;
  int cnt = 0;
  if (VEC) {
    uint2 v[kPackSteps];
    int64_t g[kPackSteps];
#pragma unroll
    for (int s = 0; s < kPackSteps; ++s) {  // every load is issued before the first use
      g[s] = (int64_t)chunk * (kChunkWords * 8) + s * kThreads + threadIdx.x;  // index of the 8-byte group
      v[s] = make_uint2(0u, 0u);
      if (g[s] * 8 < P) v[s] = *reinterpret_cast<const uint2*>(src + g[s] * 8);  // P % 8 == 0: inside or outside as a whole
    }
#pragma unroll
    for (int s = 0; s < kPackSteps; ++s) {
      const uint32_t bits = fold4(v[s].x) | (fold4(v[s].y) << 4);
      cnt += __popc(bits);
      unsigned long long wd = (unsigned long long)bits << (8 * (lane & 7));
      wd |= __shfl_xor(wd, 1, kWave);
      wd |= __shfl_xor(wd, 2, kWave);
      wd |= __shfl_xor(wd, 4, kWave);
      if ((lane & 7) == 0 && g[s] * 8 < P) dst[g[s] / 8] = wd;  // lanes past the plane gave 0: the tail bits are 0
    }
  } else {
    const int wave = threadIdx.x / kWave;
    constexpr int kPerWave = kChunkWords / (kThreads / kWave);
    const int64_t w0 = (int64_t)chunk * kChunkWords + wave * kPerWave;
#pragma unroll 8
    for (int k = 0; k < kPerWave; ++k) {
      const int64_t wi = w0 + k, px = wi * 64 + lane;
      const uint8_t b = px < P ? src[px] : (uint8_t)0;
      const uint64_t wd = __ballot(b != 0);
      if (wi < w64 && lane == 0) {  // wi is uniform over the wavefront
        dst[wi] = wd;
        cnt += __popcll(wd);
      }
    }
  }
  const int total = block_add(cnt, s_red);
  if (threadIdx.x == 0 && total) atomicAdd(area + m, total);
}

struct IouParams {
  const int32_t* pred_idx;
  const int32_t* gt_idx;
  const float* boxes_pred;
  const float* boxes_gt;
  const uint64_t* words_pred;
  const uint64_t* words_gt;
  const int32_t* area_pred;
  const int32_t* area_gt;
  int n_pred, n_gt, n_rows, w64;
};

__global__ void __launch_bounds__(kThreads) box_iou_kernel(IouParams p, float* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= p.n_rows) return;
  const int i = p.pred_idx[r], j = p.gt_idx[r];
  float iou = NAN;  // an id outside its table reads nothing
  if ((unsigned)i < (unsigned)p.n_pred && (unsigned)j < (unsigned)p.n_gt) {
    const float* pa = p.boxes_pred + 4 * (int64_t)i;
    const float* pb = p.boxes_gt + 4 * (int64_t)j;
    const float4 a = make_float4(pa[0], pa[1], pa[2], pa[3]), b = make_float4(pb[0], pb[1], pb[2], pb[3]);
    const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
    const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f), h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
    const float inter = w * h;
    iou = inter / (area_a + area_b - inter);  // 0 / 0 stays NaN, as in torchvision
  }
  out[r] = iou;
}

__global__ void __launch_bounds__(kThreads) mask_iou_kernel(IouParams p, int32_t* __restrict__ inter_out,
                                                            int32_t* __restrict__ union_out, float* __restrict__ iou_out) {
  __shared__ int s_red[kThreads / kWave];
  const int r = blockIdx.x;
  const int i = p.pred_idx[r], j = p.gt_idx[r];
  if ((unsigned)i >= (unsigned)p.n_pred || (unsigned)j >= (unsigned)p.n_gt) {  // uniform over the workgroup
    if (threadIdx.x == 0) inter_out[r] = -1, union_out[r] = -1, iou_out[r] = NAN;
    return;
  }
  const uint64_t* __restrict__ a = p.words_pred + (int64_t)i * p.w64;
  const uint64_t* __restrict__ b = p.words_gt + (int64_t)j * p.w64;
  int cnt = 0;
#pragma unroll 4
  for (int k = threadIdx.x; k < p.w64; k += kThreads) cnt += __popcll(a[k] & b[k]);
  const int inter = block_add(cnt, s_red);
  if (threadIdx.x == 0) {
    const int uni = p.area_pred[i] + p.area_gt[j] - inter;
    inter_out[r] = inter;
    union_out[r] = uni;
    iou_out[r] = uni == 0 ? 0.f : (float)inter / (float)uni;  // both below 2^24: exact operands, one rounding
  }
}

struct MatchParams {
  const float* iou;
  const int32_t* n_det;
  const int32_t* n_gt;
  const int32_t* row_off;
  const int32_t* det_off;
  const int32_t* gt_off;
  const uint8_t* gt_ignore;
  const float* thr;
  int n_groups, n_thr;
  int64_t total_rows, total_dets, total_gts;
};

// candidates are ordered by (class, IoU, position): class 1 = a free non-ignored ground truth at or past the threshold, 0 = an
// ignored one, -1 = none; a larger IoU wins inside a class and the HIGHER position wins an exact tie
__device__ inline bool better(int c1, float v1, int j1, int c0, float v0, int j0) {
  if (c1 != c0) return c1 > c0;
  if (c1 < 0) return false;
  if (v1 != v0) return v1 > v0;
  return j1 > j0;
}

__global__ void __launch_bounds__(kWave) match_kernel(MatchParams p, int32_t* __restrict__ det_match, uint8_t* __restrict__ det_ignore,
                                                      int32_t* __restrict__ gt_match) {
  const int g = blockIdx.x / p.n_thr, t = blockIdx.x - g * p.n_thr;
  const int lane = threadIdx.x;
  const int D = p.n_det[g], G = p.n_gt[g];
  const int64_t roff = p.row_off[g], doff = p.det_off[g], goff = p.gt_off[g];
  if (D < 0 || G < 0 || roff < 0 || doff < 0 || goff < 0 || roff + (int64_t)D * G > p.total_rows || doff + D > p.total_dets ||
      goff + G > p.total_gts)
    return;  // a group that leaves the tables touches nothing (uniform over the wavefront)
  const float thr = p.thr[t];
  const float* __restrict__ iou = p.iou + roff;
  const uint8_t* __restrict__ ig = p.gt_ignore + goff;
  int32_t* gm = gt_match + (int64_t)t * p.total_gts + goff;
  int32_t* dm = det_match + (int64_t)t * p.total_dets + doff;
  uint8_t* di = det_ignore + (int64_t)t * p.total_dets + doff;
  for (int j = lane; j < G; j += kWave) gm[j] = -1;  // lane j % 64 owns ground truth j from here on
  for (int d = 0; d < D; ++d) {
    int bc = -1, bj = -1;
    float bv = 0.f;
    for (int j = lane; j < G; j += kWave) {
      const float v = iou[(int64_t)d * G + j];
      if (gm[j] >= 0 || !(v >= thr)) continue;  // taken at this threshold, below it, or NaN
      const int c = ig[j] ? 0 : 1;
      if (better(c, v, j, bc, bv, bj)) bc = c, bv = v, bj = j;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const int oc = __shfl_xor(bc, off, kWave), oj = __shfl_xor(bj, off, kWave);
      const float ov = __shfl_xor(bv, off, kWave);
      if (better(oc, ov, oj, bc, bv, bj)) bc = oc, bv = ov, bj = oj;
    }
    if (bj >= 0 && lane == bj % kWave) gm[bj] = d;
    if (lane == 0) {
      dm[d] = bj;
      di[d] = (bj >= 0 && bc == 0) ? 1 : 0;
    }
  }
}

}  // namespace
}  // namespace hp

using namespace hp;

extern "C" int64_t hp_mask_pack_words(int h, int w) {
  if (h < 1 || w < 1 || (int64_t)h * w > kMaxPlane) return -1;
  return ((int64_t)h * w + 63) / 64;
}

extern "C" int hp_mask_pack(int n, int h, int w, const uint8_t* d_masks, uint64_t* d_words, int32_t* d_area, void* stream) {
  HP_REQUIRE(n >= 0, "hp_mask_pack: negative n");
  HP_REQUIRE(h >= 1 && w >= 1, "hp_mask_pack: h and w must be positive");
  HP_REQUIRE((int64_t)h * w <= kMaxPlane, "hp_mask_pack: more than 2^24 pixels per mask");
  if (n == 0) return HP_OK;
  HP_REQUIRE(d_masks && d_words && d_area, "hp_mask_pack: null pointer");
  HP_REQUIRE(aligned(d_words, 8), "hp_mask_pack: d_words must be 8-byte aligned");
  const int64_t P = (int64_t)h * w;
  const int w64 = (int)hp_mask_pack_words(h, w);
  hipStream_t st = (hipStream_t)stream;
  HP_CHECK_HIP(hipMemsetAsync(d_area, 0, (size_t)n * sizeof(int32_t), st));
  const dim3 grid((unsigned)n, (unsigned)((w64 + kChunkWords - 1) / kChunkWords));  // at most 2^18 / 128 chunks
  if (P % 8 == 0 && aligned(d_masks, 8))
    hipLaunchKernelGGL(pack_kernel<true>, grid, dim3(kThreads), 0, st, d_masks, P, w64, d_words, d_area);
  else
    hipLaunchKernelGGL(pack_kernel<false>, grid, dim3(kThreads), 0, st, d_masks, P, w64, d_words, d_area);
  return check_launch("hp_mask_pack");
}

extern "C" int hp_det_iou(int n_rows, const int32_t* d_pred_idx, const int32_t* d_gt_idx, int n_pred, int n_gt,
                          const float* d_boxes_pred, const float* d_boxes_gt, const uint64_t* d_words_pred,
                          const int32_t* d_area_pred, const uint64_t* d_words_gt, const int32_t* d_area_gt, int w64,
                          float* d_box_iou, int32_t* d_inter, int32_t* d_union, float* d_mask_iou, void* stream) {
  HP_REQUIRE(n_rows >= 0 && n_pred >= 0 && n_gt >= 0, "hp_det_iou: negative size");
  const bool boxes = d_boxes_pred || d_boxes_gt, masks = d_words_pred || d_words_gt;
  HP_REQUIRE(!boxes || (d_boxes_pred && d_boxes_gt), "hp_det_iou: boxes of one side only");
  HP_REQUIRE(!masks || (d_words_pred && d_words_gt && d_area_pred && d_area_gt), "hp_det_iou: packed masks need words and area of both sides");
  HP_REQUIRE(!masks || (w64 >= 1 && w64 <= (int)(kMaxPlane / 64)), "hp_det_iou: w64 outside 1..2^18");
  if (n_rows == 0) return HP_OK;
  HP_REQUIRE(d_pred_idx && d_gt_idx, "hp_det_iou: null index column");
  HP_REQUIRE(!boxes || d_box_iou, "hp_det_iou: boxes given without d_box_iou");
  HP_REQUIRE(!masks || (d_inter && d_union && d_mask_iou), "hp_det_iou: masks given without d_inter, d_union and d_mask_iou");
  HP_REQUIRE(!masks || (aligned(d_words_pred, 8) && aligned(d_words_gt, 8)), "hp_det_iou: packed masks must be 8-byte aligned");
  IouParams p;
  p.pred_idx = d_pred_idx, p.gt_idx = d_gt_idx, p.boxes_pred = d_boxes_pred, p.boxes_gt = d_boxes_gt;
  p.words_pred = d_words_pred, p.words_gt = d_words_gt, p.area_pred = d_area_pred, p.area_gt = d_area_gt;
  p.n_pred = n_pred, p.n_gt = n_gt, p.n_rows = n_rows, p.w64 = w64;
  hipStream_t st = (hipStream_t)stream;
  if (boxes) {
    hipLaunchKernelGGL(box_iou_kernel, dim3((unsigned)((n_rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, p, d_box_iou);
    if (int rc = check_launch("hp_det_iou (boxes)")) return rc;
  }
  if (masks) {
    hipLaunchKernelGGL(mask_iou_kernel, dim3((unsigned)n_rows), dim3(kThreads), 0, st, p, d_inter, d_union, d_mask_iou);  // rows in x
    if (int rc = check_launch("hp_det_iou (masks)")) return rc;
  }
  return HP_OK;
}

extern "C" int hp_det_match(int n_groups, const int32_t* d_n_det, const int32_t* d_n_gt, const int32_t* d_row_off,
                            const int32_t* d_det_off, const int32_t* d_gt_off, const float* d_iou, int64_t total_rows,
                            int64_t total_dets, int64_t total_gts, const uint8_t* d_gt_ignore, const float* d_thr, int n_thr,
                            int32_t* d_det_match, uint8_t* d_det_ignore, int32_t* d_gt_match, void* stream) {
  HP_REQUIRE(n_groups >= 0 && n_thr >= 0, "hp_det_match: negative size");
  HP_REQUIRE(total_rows >= 0 && total_dets >= 0 && total_gts >= 0, "hp_det_match: negative table size");
  HP_REQUIRE(total_rows < (int64_t(1) << 31) && total_dets < (int64_t(1) << 31) && total_gts < (int64_t(1) << 31),
             "hp_det_match: tables of 2^31 entries or more");
  HP_REQUIRE((int64_t)n_groups * n_thr < (int64_t(1) << 31), "hp_det_match: 2^31 (group, threshold) pairs or more");
  if (n_groups == 0 || n_thr == 0) return HP_OK;
  HP_REQUIRE(d_n_det && d_n_gt && d_row_off && d_det_off && d_gt_off && d_thr, "hp_det_match: null group table");
  HP_REQUIRE((d_iou || total_rows == 0) && (d_gt_ignore || total_gts == 0), "hp_det_match: null input");
  HP_REQUIRE((d_det_match && d_det_ignore) || total_dets == 0, "hp_det_match: null detection output");
  HP_REQUIRE(d_gt_match || total_gts == 0, "hp_det_match: null ground-truth output");
  MatchParams p;
  p.iou = d_iou, p.n_det = d_n_det, p.n_gt = d_n_gt, p.row_off = d_row_off, p.det_off = d_det_off, p.gt_off = d_gt_off;
  p.gt_ignore = d_gt_ignore, p.thr = d_thr, p.n_groups = n_groups, p.n_thr = n_thr;
  p.total_rows = total_rows, p.total_dets = total_dets, p.total_gts = total_gts;
  hipLaunchKernelGGL(match_kernel, dim3((unsigned)(n_groups * n_thr)), dim3(kWave), 0, (hipStream_t)stream, p, d_det_match,
                     d_det_ignore, d_gt_match);
  return check_launch("hp_det_match");
}
