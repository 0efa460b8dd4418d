// Area-uniform sampling of mesh surfaces: entry points and the definition are in include/happypose_amd.h (hp_mesh_sample_surface).
// Restates the documented algorithm of trimesh.sample.sample_surface (parity unpinned: trimesh is not a dependency): a face is
// picked with probability proportional to its area, the point is uniform in the face by the reflected-parallelogram rule.
//
//   area_scan_kernel   a workgroup of kScanThreads = kScanChunk threads is one object.  Chunks of kScanChunk faces in sequence, a
//                      thread is one face of the chunk: area_f = 0.5 |(v1 - v0) x (v2 - v0)| in fp64 from the fp32 vertices (no
//                      contraction: every product and difference rounds once, in the order written in face_area), an inclusive
//                      Hillis-Steele scan over the wavefront (shuffles), the wave totals through the LDS, the prefix carried from
//                      chunk to chunk:  cum[f] = carry + (wave_prefix + lane_inclusive),  wave_prefix = ((t_0 + t_1) + ...) over
//                      the earlier waves' totals,  carry' = carry + (sum of all wave totals in the same order).  Every addend is
//                      >= 0 and fp64 addition is monotone, so cum never decreases.  No atomics: bit-identical from run to run.
//                      A face with an index outside the object's vertices reads no vertex and marks the object.  total[o] (head
//                      of the workspace) = cum[F - 1], 0 without faces, NaN for a marked object or offsets that leave the tables.
//   sample_kernel      a thread is one (object, sample); objects in grid y.  Philox4x32-10 with key (seed lo, seed hi) and counter
//                      (i, o, 0, 0): stateless, so a sample depends on (seed, o, i) and the object's mesh alone.  Binary search of
//                      the first f with cum[f] > pick (strict: a zero-area face is never picked, except through the clamp to
//                      F - 1), integer reflection of the 24-bit (ia, ib), p = (v0 + a (v1 - v0)) + b (v2 - v0) in fp32 without
//                      contraction.  An object whose total is not a positive finite number gives NaN points and face_id -1.
#include "common.h"
#include "philox.h"
#include "wave.h"

namespace hp {
namespace {

constexpr int kScanChunk = 1024;  // faces per scan step = threads of the scan workgroup
constexpr int kScanThreads = kScanChunk;
constexpr int kScanWaves = kScanThreads / kWave;
constexpr int kSampleThreads = 256;

__device__ inline double face_area(const float* __restrict__ v, int i0, int i1, int i2) {
#pragma clang fp contract(off)
  const double x0 = v[3 * (int64_t)i0], y0 = v[3 * (int64_t)i0 + 1], z0 = v[3 * (int64_t)i0 + 2];
  const double ax = (double)v[3 * (int64_t)i1] - x0, ay = (double)v[3 * (int64_t)i1 + 1] - y0, az = (double)v[3 * (int64_t)i1 + 2] - z0;
  const double bx = (double)v[3 * (int64_t)i2] - x0, by = (double)v[3 * (int64_t)i2 + 1] - y0, bz = (double)v[3 * (int64_t)i2 + 2] - z0;
  const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  return 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

__global__ void __launch_bounds__(kScanThreads) area_scan_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                 const int32_t* __restrict__ vert_offset,
                                                                 const int32_t* __restrict__ face_offset, int64_t cap_faces,
                                                                 double* __restrict__ total_out, double* __restrict__ cum,
                                                                 double* __restrict__ area_out) {
  __shared__ double s_tot[2][kScanWaves];
  __shared__ int s_bad;
  const int o = blockIdx.x, tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int64_t v0 = vert_offset[o], v1 = vert_offset[o + 1], f0 = face_offset[o], f1 = face_offset[o + 1];
  const int64_t V = v1 - v0, F = f1 - f0;
  // everything below is uniform over the workgroup
  if (v0 < 0 || V < 0 || f0 < 0 || F < 0 || f1 > cap_faces) {  // offsets that leave the tables: nothing is read or written past them
    if (tid == 0) {
      total_out[o] = NAN;
      if (area_out) area_out[o] = NAN;
    }
    return;
  }
  if (tid == 0) s_bad = 0;
  __syncthreads();
  const float* __restrict__ vv = vertices + 3 * v0;
  const int32_t* __restrict__ ff = faces + 3 * f0;
  double* __restrict__ cc = cum + f0;
  double carry = 0.0;
  int bad = 0;
  for (int64_t c0 = 0, step = 0; c0 < F; c0 += kScanChunk, ++step) {
    const int64_t f = c0 + tid;
    double a = 0.0;
    if (f < F) {
      const int i0 = ff[3 * f], i1 = ff[3 * f + 1], i2 = ff[3 * f + 2];
      if ((uint64_t)i0 < (uint64_t)V && (uint64_t)i1 < (uint64_t)V && (uint64_t)i2 < (uint64_t)V)
        a = face_area(vv, i0, i1, i2);
      else
        bad = 1;
    }
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {  // inclusive scan over the wavefront
      const double t = __shfl_up(a, off, kWave);
      if (lane >= off) a += t;
    }
    const int buf = (int)(step & 1);
    if (lane == kWave - 1) s_tot[buf][wave] = a;
    __syncthreads();  // double-buffered: one barrier per chunk
    double prefix = 0.0, chunk = 0.0;
#pragma unroll
    for (int w = 0; w < kScanWaves; ++w) {
      if (w == wave) prefix = chunk;
      chunk += s_tot[buf][w];
    }
    if (f < F) cc[f] = carry + (prefix + a);
    carry = carry + chunk;
  }
  if (bad) s_bad = 1;  // every writer stores the same value
  __syncthreads();
  if (tid == 0) {
    const double total = s_bad ? (double)NAN : carry;
    total_out[o] = total;
    if (area_out) area_out[o] = total;
  }
}

__global__ void __launch_bounds__(kSampleThreads) sample_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                const int32_t* __restrict__ vert_offset,
                                                                const int32_t* __restrict__ face_offset, int n_samples, uint32_t key0,
                                                                uint32_t key1, const double* __restrict__ total_in,
                                                                const double* __restrict__ cum, float* __restrict__ points,
                                                                int32_t* __restrict__ face_id) {
#pragma clang fp contract(off)
  const int o = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x;
  if (i >= n_samples) return;
  const int64_t row = (int64_t)o * n_samples + i;
  float* __restrict__ p = points + 3 * row;
  const double total = total_in[o];  // uniform over the workgroup
  if (!(total > 0.0) || !(total < (double)INFINITY)) {  // no faces, zero or non-finite area, an index out of range: nothing else is read
    p[0] = NAN, p[1] = NAN, p[2] = NAN;
    if (face_id) face_id[row] = -1;
    return;
  }
  const int64_t f0 = face_offset[o];
  const int F = (int)(face_offset[o + 1] - f0);
  const double* __restrict__ cc = cum + f0;
  uint32_t r[4] = {(uint32_t)i, (uint32_t)o, 0u, 0u};
  philox4x32_10(r, key0, key1);
  const double u = (double)(((uint64_t)r[0] << 21) | (uint64_t)(r[1] >> 11)) * 0x1p-53;  // 53 bits: exact
  const double pick = u * total;
  int lo = 0, hi = F;  // the first f with cum[f] > pick lies in [lo, hi]; hi == F: none
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (cc[mid] > pick)
      hi = mid;
    else
      lo = mid + 1;
  }
  const int f = lo < F ? lo : F - 1;
  uint32_t ia = r[2] >> 8, ib = r[3] >> 8;
  if (ia + ib > (1u << 24)) ia = (1u << 24) - ia, ib = (1u << 24) - ib;  // on integers: a float a + b > 1 may round
  const float a = (float)ia * 0x1p-24f, b = (float)ib * 0x1p-24f;  // exact
  const int32_t* __restrict__ fi = faces + 3 * (f0 + f);
  const float* __restrict__ vv = vertices + 3 * (int64_t)vert_offset[o];
  const float* __restrict__ q0 = vv + 3 * (int64_t)fi[0];
  const float* __restrict__ q1 = vv + 3 * (int64_t)fi[1];
  const float* __restrict__ q2 = vv + 3 * (int64_t)fi[2];
#pragma unroll
  for (int d = 0; d < 3; ++d) p[d] = (q0[d] + a * (q1[d] - q0[d])) + b * (q2[d] - q0[d]);
  if (face_id) face_id[row] = f;
}

}  // namespace
}  // namespace hp

using namespace hp;

extern "C" int64_t hp_mesh_sample_workspace_bytes(int n_obj, int64_t total_faces) {
  if (n_obj < 0 || total_faces < 0 || total_faces >= (int64_t(1) << 31)) return -1;
  return ((int64_t)n_obj + total_faces) * (int64_t)sizeof(double);
}

extern "C" int hp_mesh_sample_surface(int n_obj, const float* d_vertices, const int32_t* d_faces, const int32_t* d_vert_offset,
                                      const int32_t* d_face_offset, int n_samples, uint64_t seed, float* d_points, int32_t* d_face_id,
                                      double* d_area, void* d_workspace, int64_t workspace_bytes, void* stream) {
  HP_REQUIRE(n_obj >= 0 && n_samples >= 0, "hp_mesh_sample_surface: negative size");
  HP_REQUIRE(n_obj <= 65535, "hp_mesh_sample_surface: more than 65535 objects");
  if (n_obj == 0 || n_samples == 0) return HP_OK;
  HP_REQUIRE(d_vert_offset && d_face_offset && d_points, "hp_mesh_sample_surface: null pointer");
  // the face capacity of the tables is what the workspace was sized for: offsets past it are guarded on the device
  const int64_t cap_faces = workspace_bytes / (int64_t)sizeof(double) - n_obj;
  HP_REQUIRE(d_workspace && cap_faces >= 0, "hp_mesh_sample_surface: workspace smaller than hp_mesh_sample_workspace_bytes(n_obj, total_faces)");
  HP_REQUIRE(aligned(d_workspace, 8), "hp_mesh_sample_surface: d_workspace must be 8-byte aligned");
  HP_REQUIRE(cap_faces == 0 || (d_vertices && d_faces), "hp_mesh_sample_surface: null mesh tables");
  hipStream_t st = (hipStream_t)stream;
  double* total = (double*)d_workspace;
  double* cum = total + n_obj;
  hipLaunchKernelGGL(area_scan_kernel, dim3((unsigned)n_obj), dim3(kScanThreads), 0, st, d_vertices, d_faces, d_vert_offset,
                     d_face_offset, cap_faces, total, cum, d_area);
  if (int rc = check_launch("hp_mesh_sample_surface (areas)")) return rc;
  const dim3 grid((unsigned)(((int64_t)n_samples + kSampleThreads - 1) / kSampleThreads), (unsigned)n_obj);
  hipLaunchKernelGGL(sample_kernel, grid, dim3(kSampleThreads), 0, st, d_vertices, d_faces, d_vert_offset, d_face_offset, n_samples,
                     (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), total, cum, d_points, d_face_id);
  return check_launch("hp_mesh_sample_surface (samples)");
}
