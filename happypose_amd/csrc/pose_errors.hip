// Pose-error metrics of the evaluation (ADD, ADD-S, ADD-SYM, MSSD, MSPD): entry points and the reference lines they replace are in
// include/happypose_amd.h.
//
// A row is a triple (predicted pose, ground-truth pose, object), gathered through int32 index columns.  Three kernels:
//   rows_kernel    ONE WAVEFRONT per row, lanes over the object's points (a loop: no size limit), symmetries walked serially.  It
//                  answers the guards, the translation errors of every row and all of ADD / ADD-SYM / MSSD / MSPD.
//   adds_kernel    ADD-S.  A workgroup is one (row, block of kGtBlock ground-truth points); every lane keeps kGtPerLane of them in
//                  registers.  The row's predicted points stream through LDS in tiles of kPredTile, transformed ONCE per tile,
//                  and are read back by same-address (broadcast) 16-byte reads.  The distance stays in the reference's difference
//                  form (subtract, then square): no |a|^2 + |b|^2 - 2ab.  Nothing of size P x P exists anywhere.
//   adds_finish    adds the per-block partial sums of a row IN BLOCK ORDER.
// No float atomics; every reduction is a fixed tree, so a row's outputs are a function of the row alone: the number of rows in the
// launch, their modes and the run cannot change a bit.
#include "common.h"
#include "rigid.h"
#include "wave.h"

namespace hp {
namespace {

constexpr int kRowsPerBlock = 4;                      // rows_kernel: 256 threads
constexpr int kPredTile = HP_POSE_ERR_PRED_TILE;      // predicted points per LDS tile (float4 each: 8 KB)
constexpr int kGtBlock = HP_POSE_ERR_GT_BLOCK;        // ground-truth points per workgroup
constexpr int kAddsThreads = 256;
constexpr int kGtPerLane = kGtBlock / kAddsThreads;   // 4
constexpr int kPartial = 8;                           // floats per (row, block): sum |d|, sum |dx| |dy| |dz|, max |d|, 3 unused
static_assert(kGtBlock % kAddsThreads == 0 && kPredTile % kAddsThreads == 0, "tile sizes are multiples of the workgroup");

struct Tables {
  const int32_t* pred_id;
  const int32_t* gt_id;
  const int32_t* obj_id;
  const int32_t* mode;
  const float* poses_pred;
  const float* poses_gt;
  const float* K;  // [n_rows][9] or nullptr
  const float* points;
  const float* symmetries;
  const int32_t* n_sym;
  const int32_t* n_pts;
  int n_pred, n_gt, n_obj, max_pts, s_max;
  int adds_enabled;  // 0: the caller declared that no row is ADD-S and the ADD-S kernels are not launched
};

struct Row {
  int pred, gt, obj, mode, n_sym, n_pts;
};

// an index outside its table, an n_sym outside 1..s_max, an n_pts outside 1..max_pts, an unknown mode, MSPD
// without K or an ADD-S row in a call declared to hold none make the row NaN; nothing of such a row is read past the index columns and the two count tables.
__device__ inline bool load_row(const Tables& t, int row, Row& r) {
  r.pred = t.pred_id[row];
  r.gt = t.gt_id[row];
  r.obj = t.obj_id[row];
  r.mode = t.mode[row];
  r.n_sym = r.n_pts = 0;
  if ((unsigned)r.pred >= (unsigned)t.n_pred || (unsigned)r.gt >= (unsigned)t.n_gt || (unsigned)r.obj >= (unsigned)t.n_obj) return false;
  if (r.mode < HP_POSE_ERR_ADD || r.mode > HP_POSE_ERR_MSPD || (r.mode == HP_POSE_ERR_MSPD && !t.K) ||
      (r.mode == HP_POSE_ERR_ADD_S && !t.adds_enabled))
    return false;
  r.n_sym = t.n_sym[r.obj];
  r.n_pts = t.n_pts[r.obj];
  return r.n_sym >= 1 && r.n_sym <= t.s_max && r.n_pts >= 1 && r.n_pts <= t.max_pts;
}

struct Outputs {
  float* norm_avg;
  float* xyz_avg;
  float* norm_max;
  int32_t* sym_id;
  float* TCO_xyz;
  float* TCO_norm;
  int32_t* assign;  // [n_rows][max_pts] or nullptr
};

__global__ void __launch_bounds__(kWave* kRowsPerBlock) rows_kernel(int n_rows, Tables t, Outputs o) {
  const int lane = threadIdx.x % kWave;
  const int row = blockIdx.x * kRowsPerBlock + threadIdx.x / kWave;
  if (row >= n_rows) return;  // whole wavefront
  Row r;
  const bool ok = load_row(t, row, r);
  int32_t* assign = o.assign ? o.assign + (int64_t)row * t.max_pts : nullptr;
  if (!ok) {
    if (lane == 0) {
      o.norm_avg[row] = o.norm_max[row] = o.TCO_norm[row] = NAN;
      o.sym_id[row] = -1;
    }
    if (lane < 3) o.xyz_avg[3 * (int64_t)row + lane] = o.TCO_xyz[3 * (int64_t)row + lane] = NAN;
    if (assign)
      for (int j = lane; j < t.max_pts; j += kWave) assign[j] = -1;
    return;
  }
  const T34 Tp = load_T(t.poses_pred + 16 * (int64_t)r.pred);
  const T34 Tg = load_T(t.poses_gt + 16 * (int64_t)r.gt);
  if (lane == 0) {  // PoseErrorMeter.compute_errors: |t_pred - t_gt| and its norm
    const float dx = Tp.m[3] - Tg.m[3], dy = Tp.m[7] - Tg.m[7], dz = Tp.m[11] - Tg.m[11];
    o.TCO_xyz[3 * (int64_t)row] = fabsf(dx);
    o.TCO_xyz[3 * (int64_t)row + 1] = fabsf(dy);
    o.TCO_xyz[3 * (int64_t)row + 2] = fabsf(dz);
    o.TCO_norm[row] = sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
  }
  if (r.mode == HP_POSE_ERR_ADD_S) return;  // adds_kernel / adds_finish write the rest of the row
  if (assign)
    for (int j = lane; j < t.max_pts; j += kWave) assign[j] = j < r.n_pts ? j : -1;
  const float* pts = t.points + 3 * (int64_t)r.obj * t.max_pts;
  const float* sym = t.symmetries + 16 * (int64_t)r.obj * t.s_max;
  const bool pixels = r.mode == HP_POSE_ERR_MSPD;
  const bool key_is_max = r.mode == HP_POSE_ERR_MSSD || pixels;
  const float* Kr = pixels ? t.K + 9 * (int64_t)row : nullptr;  // load_row: K is there for MSPD
  const T34 P = pixels ? camera_matrix(Kr, Tp) : Tp;
  const int ns = r.mode == HP_POSE_ERR_ADD ? 1 : r.n_sym;
  const float n = (float)r.n_pts;
  // a key that is NaN never wins: the chosen symmetry is always inside the table
  float best_key = INFINITY, b_norm = NAN, b_x = NAN, b_y = NAN, b_z = NAN, b_max = NAN;
  int best_s = 0;
  for (int s = 0; s < ns; ++s) {
    T34 M = r.mode == HP_POSE_ERR_ADD ? Tg : mul(Tg, load_T(sym + 16 * s));
    if (pixels) M = camera_matrix(Kr, M);
    float sn = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, mx = 0.f;
    for (int j = lane; j < r.n_pts; j += kWave) {
      const float x = pts[3 * j], y = pts[3 * j + 1], z = pts[3 * j + 2];
      float ax, ay, az, bx, by, bz;
      apply(M, x, y, z, ax, ay, az);
      apply(P, x, y, z, bx, by, bz);
      float dx, dy, dz;
      if (pixels) {  // project_points: suv / suv[2]
        dx = ax / az - bx / bz;
        dy = ay / az - by / bz;
        dz = 0.f;
      } else {
        dx = ax - bx;
        dy = ay - by;
        dz = az - bz;
      }
      const float d = sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
      sn += d;
      sx += fabsf(dx);
      sy += fabsf(dy);
      sz += fabsf(dz);
      mx = d > mx || d != d ? d : mx;  // a NaN distance stays visible in the maximum
    }
    sn = wave_sum(sn) / n;
    sx = wave_sum(sx) / n;
    sy = wave_sum(sy) / n;
    sz = wave_sum(sz) / n;
    const float any_nan = wave_max(mx != mx ? 1.f : 0.f);
    mx = any_nan > 0.f ? NAN : wave_max(mx);
    const float key = key_is_max ? mx : sn;
    if (key < best_key || (s == 0 && ns == 1)) {  // first strict minimum; a single candidate is the answer whatever its key
      best_key = key;
      best_s = s;
      b_norm = sn, b_x = sx, b_y = sy, b_z = sz, b_max = mx;
    }
  }
  if (lane == 0) {
    o.norm_avg[row] = b_norm;
    o.xyz_avg[3 * (int64_t)row] = b_x;
    o.xyz_avg[3 * (int64_t)row + 1] = b_y;
    o.xyz_avg[3 * (int64_t)row + 2] = b_z;
    o.norm_max[row] = b_max;
    o.sym_id[row] = r.mode == HP_POSE_ERR_ADD ? -1 : best_s;
  }
}

__global__ void __launch_bounds__(kAddsThreads) adds_kernel(Tables t, int32_t* __restrict__ assign_out, float* __restrict__ partials) {
  __shared__ float4 s_pred[kPredTile];
  __shared__ float s_red[kAddsThreads / kWave][5];
  const int row = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
  Row r;
  if (!load_row(t, row, r) || r.mode != HP_POSE_ERR_ADD_S) return;  // uniform over the workgroup
  const int j0 = blk * kGtBlock;
  if (assign_out)  // the padded tail of the row names no point
    for (int j = max(j0, r.n_pts) + tid; j < min(j0 + kGtBlock, t.max_pts); j += kAddsThreads) assign_out[(int64_t)row * t.max_pts + j] = -1;
  if (j0 >= r.n_pts) return;
  const T34 Tp = load_T(t.poses_pred + 16 * (int64_t)r.pred);
  const T34 Tg = load_T(t.poses_gt + 16 * (int64_t)r.gt);
  const float* pts = t.points + 3 * (int64_t)r.obj * t.max_pts;
  float gx[kGtPerLane], gy[kGtPerLane], gz[kGtPerLane], best[kGtPerLane];
  int best_i[kGtPerLane];
#pragma unroll
  for (int g = 0; g < kGtPerLane; ++g) {
    const int j = min(j0 + g * kAddsThreads + tid, r.n_pts - 1);  // lanes past the end repeat the last point and are not counted
    apply(Tg, pts[3 * j], pts[3 * j + 1], pts[3 * j + 2], gx[g], gy[g], gz[g]);
    best[g] = INFINITY;
    best_i[g] = 0;  // a distance that is NaN never wins: the index stays inside the table
  }
  for (int i0 = 0; i0 < r.n_pts; i0 += kPredTile) {
    const int tile_n = min(kPredTile, r.n_pts - i0);
    __syncthreads();  // the previous tile has been read
    for (int i = tid; i < tile_n; i += kAddsThreads) {
      const float* p = pts + 3 * (int64_t)(i0 + i);
      float4 q;
      apply(Tp, p[0], p[1], p[2], q.x, q.y, q.z);
      q.w = 0.f;
      s_pred[i] = q;
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < tile_n; ++i) {
      const float4 q = s_pred[i];  // one address for the wavefront: a broadcast read
#pragma unroll
      for (int g = 0; g < kGtPerLane; ++g) {
        const float dx = gx[g] - q.x, dy = gy[g] - q.y, dz = gz[g] - q.z;
        const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
        if (d2 < best[g]) {  // ascending i, strict <: the lowest index on an exact tie
          best[g] = d2;
          best_i[g] = i0 + i;
        }
      }
    }
  }
  float sn = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, mx = 0.f;
#pragma unroll
  for (int g = 0; g < kGtPerLane; ++g) {
    const int j = j0 + g * kAddsThreads + tid;
    if (j < r.n_pts) {
      const float* p = pts + 3 * (int64_t)best_i[g];
      float px, py, pz;
      apply(Tp, p[0], p[1], p[2], px, py, pz);  // the same arithmetic as the tile: the same bits
      const float dx = gx[g] - px, dy = gy[g] - py, dz = gz[g] - pz;
      const float d = sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
      sn += d;
      sx += fabsf(dx);
      sy += fabsf(dy);
      sz += fabsf(dz);
      mx = d > mx || d != d ? d : mx;
      if (assign_out) assign_out[(int64_t)row * t.max_pts + j] = best_i[g];
    }
  }
  sn = wave_sum(sn);
  sx = wave_sum(sx);
  sy = wave_sum(sy);
  sz = wave_sum(sz);
  const float any_nan = wave_max(mx != mx ? 1.f : 0.f);
  mx = any_nan > 0.f ? NAN : wave_max(mx);
  const int wave = tid / kWave;
  if (tid % kWave == 0) {
    s_red[wave][0] = sn;
    s_red[wave][1] = sx;
    s_red[wave][2] = sy;
    s_red[wave][3] = sz;
    s_red[wave][4] = mx;
  }
  __syncthreads();
  if (tid < 5) {
    float v = s_red[0][tid];
    for (int w = 1; w < kAddsThreads / kWave; ++w) {  // wavefront order
      const float u = s_red[w][tid];
      v = tid < 4 ? v + u : (u > v || u != u ? u : v);
    }
    partials[((int64_t)row * gridDim.x + blk) * kPartial + tid] = v;
  }
}

__global__ void __launch_bounds__(kWave) adds_finish_kernel(int n_rows, int n_blocks, Tables t, Outputs o, const float* __restrict__ partials) {
  const int row = blockIdx.x * kWave + threadIdx.x;
  if (row >= n_rows) return;
  Row r;
  if (!load_row(t, row, r) || r.mode != HP_POSE_ERR_ADD_S) return;
  const int used = (r.n_pts + kGtBlock - 1) / kGtBlock;  // <= n_blocks: n_pts <= max_pts
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < used; ++b) {  // block order
    const float* p = partials + ((int64_t)row * n_blocks + b) * kPartial;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += p[k];
    acc[4] = p[4] > acc[4] || p[4] != p[4] ? p[4] : acc[4];
  }
  const float n = (float)r.n_pts;
  o.norm_avg[row] = acc[0] / n;
  o.xyz_avg[3 * (int64_t)row] = acc[1] / n;
  o.xyz_avg[3 * (int64_t)row + 1] = acc[2] / n;
  o.xyz_avg[3 * (int64_t)row + 2] = acc[3] / n;
  o.norm_max[row] = acc[4];
  o.sym_id[row] = -1;
}

int adds_blocks(int max_pts) { return (max_pts + kGtBlock - 1) / kGtBlock; }

}  // namespace
}  // namespace hp

using namespace hp;

extern "C" int64_t hp_pose_errors_workspace_bytes(int n_rows, int max_pts) {
  if (n_rows < 0 || max_pts < 1) return -1;
  return (int64_t)n_rows * adds_blocks(max_pts) * kPartial * (int64_t)sizeof(float);
}

extern "C" int hp_pose_errors(int n_rows, const int32_t* d_pred_id, const int32_t* d_gt_id, const int32_t* d_obj_id,
                              const int32_t* d_mode, int n_add_s, const float* d_poses_pred, int n_pred, const float* d_poses_gt,
                              int n_gt, const float* d_K, const float* d_points, const float* d_symmetries, const int32_t* d_n_sym,
                              const int32_t* d_n_pts, int n_obj, int max_pts, int s_max, float* d_norm_avg, float* d_xyz_avg,
                              float* d_norm_max, int32_t* d_sym_id, float* d_TCO_xyz, float* d_TCO_norm, int32_t* d_assign,
                              void* d_workspace, int64_t workspace_bytes, void* stream) {
  HP_REQUIRE(n_rows >= 0 && n_pred >= 0 && n_gt >= 0, "hp_pose_errors: negative size");
  if (n_rows == 0) return HP_OK;
  HP_REQUIRE(d_points && d_symmetries && d_n_sym && d_n_pts, "hp_pose_errors: mesh tables missing");
  HP_REQUIRE(n_obj >= 1 && max_pts >= 1 && s_max >= 1, "hp_pose_errors: n_obj, max_pts and s_max must be positive");
  HP_REQUIRE((int64_t)n_obj * s_max < (int64_t(1) << 26) && (int64_t)n_obj * max_pts < (int64_t(1) << 28),
             "hp_pose_errors: mesh tables too large");
  HP_REQUIRE(d_pred_id && d_gt_id && d_obj_id && d_mode && d_poses_pred && d_poses_gt && d_norm_avg && d_xyz_avg && d_norm_max &&
                 d_sym_id && d_TCO_xyz && d_TCO_norm,
             "hp_pose_errors: null pointer");
  const int blocks = adds_blocks(max_pts);
  HP_REQUIRE(n_rows <= 65535 * kRowsPerBlock && n_rows <= 65535, "hp_pose_errors: more than 65535 rows in one call");
  HP_REQUIRE(!d_assign || (int64_t)n_rows * max_pts < (int64_t(1) << 31), "hp_pose_errors: d_assign of 2^31 entries or more");
  const bool adds = n_add_s != 0;  // negative: the caller does not know
  HP_REQUIRE(!adds || (d_workspace && workspace_bytes >= hp_pose_errors_workspace_bytes(n_rows, max_pts)),
             "hp_pose_errors: workspace smaller than hp_pose_errors_workspace_bytes(n_rows, max_pts)");
  const Tables t{d_pred_id, d_gt_id, d_obj_id, d_mode, d_poses_pred, d_poses_gt, d_K, d_points, d_symmetries, d_n_sym, d_n_pts,
                 n_pred, n_gt, n_obj, max_pts, s_max, adds ? 1 : 0};
  const Outputs o{d_norm_avg, d_xyz_avg, d_norm_max, d_sym_id, d_TCO_xyz, d_TCO_norm, d_assign};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rows_kernel, dim3((n_rows + kRowsPerBlock - 1) / kRowsPerBlock), dim3(kWave * kRowsPerBlock), 0, st, n_rows, t, o);
  if (int rc = check_launch("hp_pose_errors (rows)")) return rc;
  if (!adds) return HP_OK;
  hipLaunchKernelGGL(adds_kernel, dim3(blocks, n_rows), dim3(kAddsThreads), 0, st, t, d_assign, (float*)d_workspace);
  if (int rc = check_launch("hp_pose_errors (ADD-S blocks)")) return rc;
  hipLaunchKernelGGL(adds_finish_kernel, dim3((n_rows + kWave - 1) / kWave), dim3(kWave), 0, st, n_rows, blocks, t, o,
                     (const float*)d_workspace);
  return check_launch("hp_pose_errors (ADD-S sums)");
}
