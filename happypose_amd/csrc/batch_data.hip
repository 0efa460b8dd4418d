// Batch assembly of the training data sets (happypose_amd/datasets.py): what the reference's PoseDataset.make_data_from_obs +
// collate_fn and DetectionDataset.make_data_from_obs do between a scene observation and the trainers' steps, on frames that already
// live on the device.  Entry points and definitions are in include/happypose_amd.h (hp_pose_batch_select, hp_batch_gather_chw,
// hp_instance_masks).
//
//   select_kernel   a wavefront is one frame; lane l owns slots l, l + 64, l + 128, l + 192 (max_ids <= 256).  The valid flags of a
//                   chunk of 64 slots are one ballot, the number of valid slots the sum of four population counts, and the k-th
//                   valid slot is the lane whose flag is set with k flags set below it (a second ballot).  k is 0 (first) or
//                   mulhi32(x0, n_valid), x0 = word 0 of Philox4x32-10, key (seed lo, seed hi), counter (row lo, row hi, 0, 0),
//                   row = row_offset + b in 64 bits: the generator of philox.h, the key layout of csrc/train_hyp.hip.  Lanes 0 .. 15 then
//                   evaluate one entry each of inverse(TWC) @ TWO[chosen] in double from the float32 inputs, in the order written
//                   in the header, and round once.
//   scan_kernel     one workgroup: the exclusive scan of the valid flags over the frames, 256 frames per step (ballot, population
//                   count below the lane, the four wavefronts' totals through the LDS, a running carry), and the total.
//   gather_kernel   a workgroup is one tile of kTile pixels of one frame.  RGB: the tile's 3 kTile interleaved bytes are read as
//                   16-byte vectors on the 16-byte grid of the INPUT address and written into three planes in the LDS, plane c
//                   shifted by the misalignment of its OUTPUT address, so that the planes leave as 16-byte vectors on the 16-byte
//                   grid of the output.  A frame's byte ranges need not start or end on either grid (h w odd): the vectors that
//                   straddle an end of a range are moved byte by byte by the lanes that own them ("tail lanes"); everything between
//                   is a full vector.  Depth tiles (the workgroups after the RGB tiles) copy 32-bit words, four at a time when both
//                   addresses are 16-byte aligned.
//   masks_kernel    a workgroup is one tile of kTile pixels of one frame.  It reads the tile of the id map ONCE into the LDS and
//                   writes, for every kept slot of the frame, the tile of that slot's mask row: a lane compares 16 staged ids with
//                   the slot's id and stores the 16 bytes as one vector on the 16-byte grid of the row's address (tail lanes as
//                   above).  The staged ids are padded by one word per 16 (index i lives at i + i / 16), so that the 16-word
//                   strides of the lanes fall on distinct banks.
//
// Integers and copied bits only, except the pose product; no atomics; every output element has one writer: two calls give the same
// bits.  Every index that comes from device memory (count, dst, slot_row) is checked against the table it addresses before use.
#include "common.h"
#include "philox.h"
#include "wave.h"

namespace hp {
namespace {

#pragma clang fp contract(off)  // the pose product rounds in the order written

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxIds = 256;  // as hp_seg_boxes
constexpr int kTile = 4096;   // pixels per workgroup of gather_kernel and masks_kernel
constexpr int kPlane = kTile + 16;           // bytes of one LDS plane of gather_kernel: the tile and the largest shift, a multiple of 16
constexpr int kSegWords = kTile + kTile / 16;  // padded words of the staged id map

__device__ inline uint32_t philox_word0(uint64_t row, uint32_t k0, uint32_t k1) {
  uint32_t c[4] = {(uint32_t)row, (uint32_t)(row >> 32), 0u, 0u};
  philox4x32_10(c, k0, k1);
  return c[0];
}

__global__ void __launch_bounds__(kWave) select_kernel(int max_ids, const int32_t* __restrict__ n_px, const int32_t* __restrict__ boxes,
                                                       const int32_t* __restrict__ count, const uint8_t* __restrict__ keep, float min_area,
                                                       int first, uint32_t k0, uint32_t k1, uint64_t row_offset,
                                                       const float* __restrict__ TWC, const float* __restrict__ TWO,
                                                       int32_t* __restrict__ chosen_out, uint8_t* __restrict__ valid_out,
                                                       float* __restrict__ bbox, float* __restrict__ TCO) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int cnt = min(max(count[b], 0), max_ids);
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  uint64_t mask[kMaxIds / kWave];
  int n_valid = 0;
#pragma unroll
  for (int c = 0; c < kMaxIds / kWave; ++c) {
    const int slot = c * kWave + lane;
    bool v = false;
    if (slot < cnt) {
      const int64_t idx = (int64_t)b * max_ids + slot;
      v = n_px[idx] > 0;  // remove_invisible_objects and `unique_id in unique_ids_visible`
      if (v && min_area >= 0.f) {
        const int32_t* bx = boxes + 4 * idx;
        const int64_t area = ((int64_t)bx[3] - bx[1]) * ((int64_t)bx[2] - bx[0]);  // the inclusive box, no + 1: the reference's
        v = (double)area >= (double)min_area;
      }
      if (v && keep) v = keep[idx] != 0;
    }
    mask[c] = __ballot(v);
    n_valid += __popcll(mask[c]);
  }
  int chosen = -1;
  if (n_valid > 0) {  // uniform over the wavefront, and so is everything below but the lane's own flag
    const int k = first ? 0 : (int)__umulhi(philox_word0(row_offset + (uint64_t)b, k0, k1), (uint32_t)n_valid);
    int base = 0;
#pragma unroll
    for (int c = 0; c < kMaxIds / kWave; ++c) {
      const int pc = __popcll(mask[c]);
      if (chosen < 0 && k < base + pc) {
        const bool hit = ((mask[c] >> lane) & 1) && __popcll(mask[c] & below) == k - base;
        chosen = c * kWave + __ffsll((unsigned long long)__ballot(hit)) - 1;
      }
      base += pc;
    }
  }
  if (lane == 0) {
    chosen_out[b] = chosen;
    valid_out[b] = chosen >= 0;
  }
  const int64_t slot = (int64_t)b * max_ids + max(chosen, 0);
  if (lane < 4) bbox[4 * (int64_t)b + lane] = chosen >= 0 ? (float)boxes[4 * slot + lane] : 0.f;
  if (lane < 16) {
    float out = 0.f;
    if (chosen >= 0) {
      const float* __restrict__ A = TWC + 16 * (int64_t)b;
      const float* __restrict__ Bm = TWO + 16 * slot;
      const int i = lane >> 2, j = lane & 3;
      if (i == 3) {
        out = Bm[12 + j];  // the inverse's bottom row is (0, 0, 0, 1)
      } else {
        // row i of the rigid inverse: (R^T)[i][k] = R[k][i], and -(R^T t)[i]
        const double r0 = A[i], r1 = A[4 + i], r2 = A[8 + i];
        const double ti = -((r0 * (double)A[3] + r1 * (double)A[7]) + r2 * (double)A[11]);
        out = (float)((((r0 * (double)Bm[j] + r1 * (double)Bm[4 + j]) + r2 * (double)Bm[8 + j])) + ti * (double)Bm[12 + j]);
      }
    }
    TCO[16 * (int64_t)b + lane] = out;
  }
}

__global__ void __launch_bounds__(kThreads) scan_kernel(int B, const uint8_t* __restrict__ valid, int32_t* __restrict__ dst,
                                                        int32_t* __restrict__ n_valid) {
  __shared__ int s_total[kWaves];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  int carry = 0;
  for (int base = 0; base < B; base += kThreads) {
    const int b = base + tid;
    const bool v = b < B && valid[b] != 0;
    const uint64_t m = __ballot(v);
    if (lane == 0) s_total[wave] = __popcll(m);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) off += s_total[w];
      total += s_total[w];
    }
    if (b < B) dst[b] = carry + off + __popcll(m & (((uint64_t)1 << lane) - 1));
    carry += total;
    __syncthreads();
  }
  if (tid == 0) n_valid[0] = carry;
}

__device__ inline uint32_t byte_of(const uint32_t w[4], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xffu; }

__global__ void __launch_bounds__(kThreads) gather_kernel(int P, int tiles_rgb, int n_out, const uint8_t* __restrict__ rgb,
                                                          const uint32_t* __restrict__ depth, const uint8_t* __restrict__ valid,
                                                          const int32_t* __restrict__ dst, uint8_t* __restrict__ out_rgb,
                                                          uint32_t* __restrict__ out_depth) {
  __shared__ __align__(16) uint8_t s_plane[3 * kPlane];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (!valid[b]) return;  // uniform over the workgroup
  const int r = dst[b];
  if ((unsigned)r >= (unsigned)n_out) return;  // a row outside the output: nothing is written
  if ((int)blockIdx.x >= tiles_rgb) {  // a depth tile: 32-bit words, copied as bits
    const int p0 = ((int)blockIdx.x - tiles_rgb) * kTile, npix = min(kTile, P - p0);
    const uint32_t* __restrict__ src = depth + (int64_t)b * P + p0;
    uint32_t* __restrict__ out = out_depth + (int64_t)r * P + p0;
    if ((((uintptr_t)src | (uintptr_t)out) & 15) == 0) {
      for (int g = tid; 4 * g < npix; g += kThreads) {
        if (4 * g + 4 <= npix) {
          *(uint4*)(out + 4 * g) = *(const uint4*)(src + 4 * g);
        } else {
          for (int i = 4 * g; i < npix; ++i) out[i] = src[i];
        }
      }
    } else {
      for (int i = tid; i < npix; i += kThreads) out[i] = src[i];
    }
    return;
  }
  const int p0 = (int)blockIdx.x * kTile, npix = min(kTile, P - p0), nbytes = 3 * npix;
  const uint8_t* g0 = rgb + ((int64_t)b * P + p0) * 3;  // the tile's first byte
  const int head = (int)((uintptr_t)g0 & 15);
  const uint8_t* a0 = g0 - head;  // the 16-byte grid of the input
  uint8_t* o0[3];
  int shift[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o0[c] = out_rgb + ((int64_t)r * 3 + c) * P + p0;
    shift[c] = (int)((uintptr_t)o0[c] & 15);
  }
  const int off0 = shift[0], off1 = kPlane + shift[1], off2 = 2 * kPlane + shift[2];
  const int nvec = (head + nbytes + 15) >> 4;
  for (int v = tid; v < nvec; v += kThreads) {
    const int i0 = 16 * v - head;  // the stream index of the vector's byte 0 (negative in the head vector)
    const uint8_t* a = a0 + 16 * v;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    const bool full = i0 >= 0 && i0 + 16 <= nbytes;
    if (full) {
      const uint4 q = *(const uint4*)a;
      w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int i = i0 + j;
        if (i >= 0 && i < nbytes) w[j >> 2] |= (uint32_t)a[j] << (8 * (j & 3));
      }
    }
    int pix = (i0 + 48) / 3 - 16, c = (i0 + 48) % 3;  // i0 >= -15
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int i = i0 + j;
      if (full || (i >= 0 && i < nbytes)) s_plane[(c == 0 ? off0 : c == 1 ? off1 : off2) + pix] = (uint8_t)byte_of(w, j);
      if (++c == 3) c = 0, ++pix;
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint8_t* A0 = o0[c] - shift[c];  // the 16-byte grid of the output plane
    const int nv = (shift[c] + npix + 15) >> 4;  // <= kPlane / 16
    for (int v = tid; v < nv; v += kThreads) {
      const uint4 q = *(const uint4*)&s_plane[c * kPlane + 16 * v];
      const int q0 = 16 * v - shift[c];  // the tile pixel of the vector's byte 0
      uint8_t* a = A0 + 16 * v;
      if (q0 >= 0 && q0 + 16 <= npix) {
        *(uint4*)a = q;
      } else {
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (q0 + j >= 0 && q0 + j < npix) a[j] = (uint8_t)byte_of(w, j);
      }
    }
  }
}

__device__ inline int seg_pad(int i) { return i + (i >> 4); }

__global__ void __launch_bounds__(kThreads) masks_kernel(int P, int max_ids, int G, const int32_t* __restrict__ seg,
                                                         const int32_t* __restrict__ ids, const int32_t* __restrict__ count,
                                                         const int32_t* __restrict__ slot_row, uint8_t* __restrict__ masks) {
  __shared__ int32_t s_seg[kSegWords];
  __shared__ int32_t s_id[kMaxIds], s_row[kMaxIds];
  static_assert(kThreads == kMaxIds, "a thread per slot");
  const int b = blockIdx.y, tid = threadIdx.x;
  const int cnt = min(max(count[b], 0), max_ids);
  int row = -1;
  if (tid < cnt) {
    row = slot_row[(int64_t)b * max_ids + tid];
    if ((unsigned)row >= (unsigned)G) row = -1;  // not kept, or a row outside the output
    s_id[tid] = ids[(int64_t)b * max_ids + tid];
  }
  s_row[tid] = row;
  if (!__syncthreads_or(row >= 0)) return;  // a frame without kept slots
  const int p0 = (int)blockIdx.x * kTile, npix = min(kTile, P - p0);
  const int32_t* __restrict__ src = seg + (int64_t)b * P + p0;
  if (((uintptr_t)src & 15) == 0) {
    for (int g = tid; 4 * g < npix; g += kThreads) {
      if (4 * g + 4 <= npix) {
        const int4 q = *(const int4*)(src + 4 * g);
        const int at = seg_pad(4 * g);  // 4 g .. 4 g + 3 share one group of 16
        s_seg[at] = q.x, s_seg[at + 1] = q.y, s_seg[at + 2] = q.z, s_seg[at + 3] = q.w;
      } else {
        for (int i = 4 * g; i < npix; ++i) s_seg[seg_pad(i)] = src[i];
      }
    }
  } else {
    for (int i = tid; i < npix; i += kThreads) s_seg[seg_pad(i)] = src[i];
  }
  __syncthreads();
  for (int s = 0; s < cnt; ++s) {
    const int r = s_row[s];
    if (r < 0) continue;  // uniform
    const int32_t id = s_id[s];
    uint8_t* o0 = masks + (int64_t)r * P + p0;
    const int shift = (int)((uintptr_t)o0 & 15);
    uint8_t* A0 = o0 - shift;  // the 16-byte grid of the mask row
    const int nv = (shift + npix + 15) >> 4;
    for (int v = tid; v < nv; v += kThreads) {
      const int q0 = 16 * v - shift;  // the tile pixel of the vector's byte 0
      uint8_t* a = A0 + 16 * v;
      if (q0 >= 0 && q0 + 16 <= npix) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j >> 2] |= (uint32_t)(s_seg[seg_pad(q0 + j)] == id) << (8 * (j & 3));
        *(uint4*)a = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (q0 + j >= 0 && q0 + j < npix) a[j] = (uint8_t)(s_seg[seg_pad(q0 + j)] == id);
      }
    }
  }
}

inline bool frame_ok(int B, int h, int w) {
  return B <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w <= ((int64_t)1 << 28);
}

}  // namespace
}  // namespace hp

using namespace hp;

extern "C" int hp_pose_batch_select(int B, int max_ids, const int32_t* d_n_px, const int32_t* d_boxes, const int32_t* d_count,
                                    const uint8_t* d_keep, float min_area, int first, uint64_t seed, uint64_t row_offset, const float* d_TWC,
                                    const float* d_TWO, int32_t* d_chosen, uint8_t* d_valid, float* d_bbox, float* d_TCO, int32_t* d_dst,
                                    int32_t* d_n_valid, void* stream) {
  HP_REQUIRE(B >= 0, "hp_pose_batch_select: negative count");
  HP_REQUIRE(d_n_valid, "hp_pose_batch_select: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {
    HP_CHECK_HIP(hipMemsetAsync(d_n_valid, 0, sizeof(int32_t), st));
    return HP_OK;
  }
  HP_REQUIRE(max_ids >= 1 && max_ids <= kMaxIds, "hp_pose_batch_select: max_ids outside 1 .. 256");
  HP_REQUIRE(min_area == min_area, "hp_pose_batch_select: min_area is NaN (negative means none)");
  HP_REQUIRE(d_n_px && d_boxes && d_count && d_TWC && d_TWO && d_chosen && d_valid && d_bbox && d_TCO && d_dst,
             "hp_pose_batch_select: null pointer");
  hipLaunchKernelGGL(select_kernel, dim3(B), dim3(kWave), 0, st, max_ids, d_n_px, d_boxes, d_count, d_keep, min_area, first,
                     (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), row_offset, d_TWC, d_TWO, d_chosen, d_valid, d_bbox, d_TCO);
  if (int rc = check_launch("hp_pose_batch_select")) return rc;
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kThreads), 0, st, B, (const uint8_t*)d_valid, d_dst, d_n_valid);
  return check_launch("hp_pose_batch_select");
}

extern "C" int hp_batch_gather_chw(int B, int h, int w, const uint8_t* d_rgb, const float* d_depth, const uint8_t* d_valid,
                                   const int32_t* d_dst, int n_out, uint8_t* d_out_rgb, float* d_out_depth, void* stream) {
  HP_REQUIRE(B >= 0 && n_out >= 0, "hp_batch_gather_chw: negative count");
  if (B == 0 || n_out == 0) return HP_OK;
  HP_REQUIRE(frame_ok(B, h, w), "hp_batch_gather_chw: B > 65535, a side < 1 or more than 2^28 pixels per frame");
  HP_REQUIRE(d_rgb && d_valid && d_dst && d_out_rgb, "hp_batch_gather_chw: null pointer");
  HP_REQUIRE((d_depth == nullptr) == (d_out_depth == nullptr), "hp_batch_gather_chw: d_depth and d_out_depth go together");
  HP_REQUIRE((const void*)d_rgb != (const void*)d_out_rgb && (d_depth == nullptr || d_depth != d_out_depth),
             "hp_batch_gather_chw: the output must not alias the input");
  const int P = h * w, tiles = (P + kTile - 1) / kTile;
  hipLaunchKernelGGL(gather_kernel, dim3(d_depth ? 2 * tiles : tiles, B), dim3(kThreads), 0, (hipStream_t)stream, P, tiles, n_out, d_rgb,
                     (const uint32_t*)d_depth, d_valid, d_dst, d_out_rgb, (uint32_t*)d_out_depth);
  return check_launch("hp_batch_gather_chw");
}

extern "C" int hp_instance_masks(int B, int h, int w, const int32_t* d_segmentation, const int32_t* d_ids, const int32_t* d_count,
                                 const int32_t* d_slot_row, int max_ids, int G, uint8_t* d_masks, void* stream) {
  HP_REQUIRE(B >= 0 && G >= 0, "hp_instance_masks: negative count");
  if (B == 0 || G == 0) return HP_OK;
  HP_REQUIRE(frame_ok(B, h, w), "hp_instance_masks: B > 65535, a side < 1 or more than 2^28 pixels per frame");
  HP_REQUIRE(max_ids >= 1 && max_ids <= kMaxIds, "hp_instance_masks: max_ids outside 1 .. 256");
  HP_REQUIRE(d_segmentation && d_ids && d_count && d_slot_row && d_masks, "hp_instance_masks: null pointer");
  const int P = h * w, tiles = (P + kTile - 1) / kTile;
  hipLaunchKernelGGL(masks_kernel, dim3(tiles, B), dim3(kThreads), 0, (hipStream_t)stream, P, max_ids, G, d_segmentation, d_ids, d_count,
                     d_slot_row, d_masks);
  return check_launch("hp_instance_masks");
}
