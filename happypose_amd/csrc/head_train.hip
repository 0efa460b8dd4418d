// Training the linear heads of a pose network on a frozen backbone (happypose_amd/training.py: HeadTrainer): the weight gradient
// of the heads csrc/pool_head.hip evaluates, the same for the 512 x 512 fc in front of them, the gradient norm and the optimiser
// step.  Entry points and definitions are in include/happypose_amd.h (hp_head_backward, hp_fc_backward, hp_grad_sq_norm,
// hp_adamw_step).  All fp32, no floating-point atomics: every sum below has ONE order, a function of the sizes alone, so a result
// is bit-identical from run to run and does not depend on how many workgroups ran it.
//
//   head_bwd_partial   the heads have O = pose_dim + n_logits <= 32 output rows: the parallelism has to come from the batch.  Rows
//                      are cut into chunks of kRows = 64 in index order (a constant, not a launch parameter); a one-wave workgroup
//                      owns (chunk, 64 columns c).  It stages g[r][o] = w_b d_out[b][o] (one rounding; no product without w, 0 for
//                      a NULL logits part) in the LDS, then each lane walks the chunk's rows in index order with
//                      acc[o] = fma(g[r][o], feat[b][c], acc[o]) from acc = 0, and writes its partial to the workspace
//                      [chunk][o][c].  With d_feat it also writes d_feat[b][c] = fma chain over o = 0 .. O - 1 of g[r][o] W[o][c]
//                      from 0.  The workgroup of column block 0 sums db's partial: g[r][o] over r in index order.
//   head_bwd_combine   a thread owns one element of dW (or db): s = partial[0], s += partial[k] for k = 1 .. in index order, then
//                      dW = s or, with accumulate, dW = dW + s.
//   fc_bwd             the fc has 512 x 512 outputs: they supply the parallelism and the batch stays ONE fma chain in index
//                      order per element, so there are no partials at all.  A workgroup owns a 32 x 32 tile of dW, a thread
//                      2 x 2 of it; 32 rows of d_out and of the input are staged in the LDS at a time (rows past B as zeros:
//                      fma(0, 0, acc) == acc exactly).  Column-tile 0 also sums db (plain additions in index order).
//   sq_norm_partial    256 threads x 4 elements: lane t of workgroup k holds x_j = g[1024 k + t + 256 j] (0 past N) and
//                      s = (x0 x0 + x1 x1) + (x2 x2 + x3 x3), every product and sum rounded once; a 6-level butterfly over the
//                      wavefront; the four wavefronts as (s0 + s1) + (s2 + s3).
//   sq_norm_final      one workgroup: lane t adds partials t, t + 256, ... in index order, then the same butterfly and wave sum.
//   adamw_kernel       a thread is one element; the operation order is torch's _single_tensor_adam, each operation rounded once.
#include <cmath>

#include "common.h"

namespace hp {
namespace {

#pragma clang fp contract(off)  // every product and sum below rounds once, in the order written; fmaf() is explicit

constexpr int kRows = 64;       // rows per chunk of head_bwd_partial: part of the definition of the summation order
constexpr int kMaxHeadRows = 32;
constexpr int kTile = 32;       // fc_bwd: tile edge and rows staged per step
constexpr int kNormBlock = 1024;

template <int OT>
__global__ __launch_bounds__(64) void head_bwd_partial(int B, int C, int pose_dim, int n_logits, const float* __restrict__ feat,
                                                       const float* __restrict__ g_pose, const float* __restrict__ g_logit,
                                                       const float* __restrict__ w, const float* __restrict__ W,
                                                       float* __restrict__ ws_dW, float* __restrict__ ws_db, float* __restrict__ d_feat) {
  __shared__ float g[kRows][OT];
  const int O = pose_dim + n_logits;
  const int chunk = blockIdx.y, b0 = chunk * kRows, nb = B - b0 < kRows ? B - b0 : kRows;
  const int lane = threadIdx.x, c = blockIdx.x * 64 + lane;
  for (int i = lane; i < kRows * OT; i += 64) {
    const int r = i / OT, o = i - r * OT;
    float v = 0.f;
    if (r < nb && o < O) {
      const int64_t b = b0 + r;
      if (o < pose_dim) v = g_pose[b * pose_dim + o];
      else if (g_logit) v = g_logit[b * n_logits + (o - pose_dim)];
      if (w) v = w[b] * v;
    }
    g[r][o] = v;
  }
  __syncthreads();
  if (c < C) {
    float acc[OT], Wc[OT];
#pragma unroll
    for (int o = 0; o < OT; ++o) {
      acc[o] = 0.f;
      Wc[o] = (d_feat && o < O) ? W[(int64_t)o * C + c] : 0.f;
    }
    const float* f = feat + (int64_t)b0 * C + c;
#pragma unroll 4
    for (int r = 0; r < nb; ++r) {
      const float x = f[(int64_t)r * C];
#pragma unroll
      for (int o = 0; o < OT; ++o) acc[o] = fmaf(g[r][o], x, acc[o]);
      if (d_feat) {
        float s = 0.f;
#pragma unroll
        for (int o = 0; o < OT; ++o) s = fmaf(g[r][o], Wc[o], s);
        d_feat[(int64_t)(b0 + r) * C + c] = s;
      }
    }
#pragma unroll
    for (int o = 0; o < OT; ++o)
      if (o < O) ws_dW[((int64_t)chunk * O + o) * C + c] = acc[o];
  }
  if (blockIdx.x == 0 && lane < O) {
    float s = 0.f;
    for (int r = 0; r < nb; ++r) s += g[r][lane];
    ws_db[(int64_t)chunk * O + lane] = s;
  }
}

__global__ __launch_bounds__(256) void head_bwd_combine(int n_chunks, int64_t n_w, int O, const float* __restrict__ ws_dW,
                                                        const float* __restrict__ ws_db, int accumulate, float* dW, float* db) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_w + O) return;
  const bool is_w = i < n_w;
  const float* part = is_w ? ws_dW + i : ws_db + (i - n_w);
  const int64_t stride = is_w ? n_w : O;
  float* dst = is_w ? dW + i : db + (i - n_w);
  float s = part[0];
#pragma unroll 4
  for (int k = 1; k < n_chunks; ++k) s += part[k * stride];
  *dst = accumulate ? *dst + s : s;
}

__global__ __launch_bounds__(256) void fc_bwd(int B, int O, int C, const float* __restrict__ d_out, const float* __restrict__ x,
                                              int accumulate, float* dW, float* db) {
  __shared__ float sA[kTile][kTile + 1];  // [row of the step][o of the tile]
  __shared__ float sB[kTile][kTile + 1];  // [row of the step][c of the tile]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int o0 = blockIdx.y * kTile, c0 = blockIdx.x * kTile;
  const bool bias = blockIdx.x == 0 && tx == 0;
  float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, accb[2] = {0.f, 0.f};
  for (int k0 = 0; k0 < B; k0 += kTile) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = tid + 256 * j, r = idx >> 5, col = idx & 31;
      const int64_t b = k0 + r;
      sA[r][col] = (b < B && o0 + col < O) ? d_out[b * O + o0 + col] : 0.f;
      sB[r][col] = (b < B && c0 + col < C) ? x[b * C + c0 + col] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < kTile; ++k) {
      const float a0 = sA[k][ty], a1 = sA[k][ty + 16], v0 = sB[k][tx], v1 = sB[k][tx + 16];
      acc[0][0] = fmaf(a0, v0, acc[0][0]); acc[0][1] = fmaf(a0, v1, acc[0][1]);
      acc[1][0] = fmaf(a1, v0, acc[1][0]); acc[1][1] = fmaf(a1, v1, acc[1][1]);
      if (bias) { accb[0] += a0; accb[1] += a1; }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int o = o0 + ty + 16 * i;
    if (o >= O) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = c0 + tx + 16 * j;
      if (c >= C) continue;
      float* dst = dW + (int64_t)o * C + c;
      *dst = accumulate ? *dst + acc[i][j] : acc[i][j];
    }
    if (bias) db[o] = accumulate ? db[o] + accb[i] : accb[i];
  }
}

// sum over the 256 threads of a workgroup, the same value in every lane of wavefront 0: butterfly, then (s0 + s1) + (s2 + s3).
// Not wave.h's wave_sum: the offsets run 1, 2, ... 32 here, another rounding order, and the trained weights are pinned to it.
__device__ __forceinline__ float block_sum(float s, float* red) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void sq_norm_partial(int64_t N, const float* __restrict__ g, float* __restrict__ out) {
  __shared__ float red[4];
  const int64_t base = (int64_t)blockIdx.x * kNormBlock + threadIdx.x;
  float x[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = base + 256 * j < N ? g[base + 256 * j] : 0.f;
  const float s = block_sum((x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3]), red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void sq_norm_final(int64_t P, const float* __restrict__ part, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < P; i += 256) s += part[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

struct AdamScalars {
  float one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay, decay_factor, step_size, bc2_sqrt;
  int decoupled;
};

__global__ __launch_bounds__(256) void adamw_kernel(int64_t N, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, AdamScalars a, const float* __restrict__ sq_norm,
                                                    const float* __restrict__ max_norm) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  float grad = g[i], param = p[i];
  if (sq_norm && max_norm) {  // clip_grad_norm_: the factor is applied even when it is 1
    const float coef = fminf(max_norm[0] / (sqrtf(sq_norm[0]) + 1e-6f), 1.0f);
    grad = grad * coef;
  }
  if (a.weight_decay != 0.f) {
    if (a.decoupled) param = param * a.decay_factor;
    else grad = grad + a.weight_decay * param;
  }
  float mi = m[i], vi = v[i];
  mi = mi + a.one_minus_beta1 * (grad - mi);
  vi = vi * a.beta2;
  vi = vi + a.one_minus_beta2 * (grad * grad);
  const float denom = sqrtf(vi) / a.bc2_sqrt + a.eps;
  param = param + (-a.step_size) * (mi / denom);
  p[i] = param; m[i] = mi; v[i] = vi;
}

inline int64_t head_chunks(int B) { return ((int64_t)B + kRows - 1) / kRows; }

}  // namespace
}  // namespace hp

using namespace hp;

extern "C" int64_t hp_head_backward_ws_floats(int B, int C, int O) {
  if (B < 0 || C < 1 || O < 1) return HP_ERR_ARG;
  return head_chunks(B) * ((int64_t)O * C + O);
}

extern "C" int hp_head_backward(int B, int C, int pose_dim, int n_logits, const float* d_feat_in, const float* d_pose_grad,
                                const float* d_logit_grad, const float* d_w, const float* d_W, int accumulate, float* d_dW, float* d_db,
                                float* d_dfeat, float* d_ws, int64_t ws_floats, void* stream) {
  HP_REQUIRE(B >= 0 && C >= 1 && pose_dim >= 0 && n_logits >= 0, "hp_head_backward: negative size");
  const int O = pose_dim + n_logits;
  HP_REQUIRE(O >= 1 && O <= kMaxHeadRows, "hp_head_backward: pose_dim + n_logits must be 1 .. 32");
  HP_REQUIRE(d_dW && d_db, "hp_head_backward: null output");
  HP_REQUIRE(pose_dim == 0 || d_pose_grad || B == 0, "hp_head_backward: null pose gradient");
  HP_REQUIRE(!d_dfeat || d_W, "hp_head_backward: d_dfeat needs the head matrix d_W");
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {  // an empty sum: zeros, or nothing to add
    if (!accumulate) {
      HP_CHECK_HIP(hipMemsetAsync(d_dW, 0, (size_t)O * C * 4, st));
      HP_CHECK_HIP(hipMemsetAsync(d_db, 0, (size_t)O * 4, st));
    }
    return HP_OK;
  }
  HP_REQUIRE(d_feat_in, "hp_head_backward: null features");
  HP_REQUIRE(d_ws && ws_floats >= hp_head_backward_ws_floats(B, C, O), "hp_head_backward: workspace too small (hp_head_backward_ws_floats)");
  const int n_chunks = (int)head_chunks(B);
  HP_REQUIRE(n_chunks <= 65535, "hp_head_backward: more than 65535 * 64 rows");
  const int64_t n_w = (int64_t)O * C;
  float* ws_db = d_ws + (int64_t)n_chunks * n_w;
  const dim3 grid((C + 63) / 64, n_chunks);
  if (O <= 16)
    hipLaunchKernelGGL(head_bwd_partial<16>, grid, dim3(64), 0, st, B, C, pose_dim, n_logits, d_feat_in, d_pose_grad, d_logit_grad, d_w,
                       d_W, d_ws, ws_db, d_dfeat);
  else
    hipLaunchKernelGGL(head_bwd_partial<32>, grid, dim3(64), 0, st, B, C, pose_dim, n_logits, d_feat_in, d_pose_grad, d_logit_grad, d_w,
                       d_W, d_ws, ws_db, d_dfeat);
  int rc = check_launch("head_bwd_partial");
  if (rc) return rc;
  hipLaunchKernelGGL(head_bwd_combine, dim3((unsigned)((n_w + O + 255) / 256)), dim3(256), 0, st, n_chunks, n_w, O, d_ws, ws_db,
                     accumulate, d_dW, d_db);
  return check_launch("head_bwd_combine");
}

extern "C" int hp_fc_backward(int B, int O, int C, const float* d_dout, const float* d_in, int accumulate, float* d_dW, float* d_db,
                              void* stream) {
  HP_REQUIRE(B >= 0 && O >= 1 && C >= 1, "hp_fc_backward: bad size");
  HP_REQUIRE(d_dW && d_db && (B == 0 || (d_dout && d_in)), "hp_fc_backward: null pointer");
  HP_REQUIRE((O + kTile - 1) / kTile <= 65535, "hp_fc_backward: too many output rows");
  if (B == 0 && accumulate) return HP_OK;
  // B == 0 without accumulate: the kernel's loop is empty and it stores zeros
  hipLaunchKernelGGL(fc_bwd, dim3((C + kTile - 1) / kTile, (O + kTile - 1) / kTile), dim3(256), 0, (hipStream_t)stream, B, O, C, d_dout,
                     d_in, accumulate, d_dW, d_db);
  return check_launch("fc_bwd");
}

extern "C" int64_t hp_grad_sq_norm_ws_floats(int64_t N) {
  if (N < 0) return HP_ERR_ARG;
  return (N + kNormBlock - 1) / kNormBlock;
}

extern "C" int hp_grad_sq_norm(int64_t N, const float* d_g, float* d_sq_norm, float* d_ws, int64_t ws_floats, void* stream) {
  HP_REQUIRE(N >= 0 && N <= 0x7fffffff, "hp_grad_sq_norm: element count outside 0 .. 2^31 - 1");
  HP_REQUIRE(d_sq_norm && (N == 0 || d_g), "hp_grad_sq_norm: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t P = hp_grad_sq_norm_ws_floats(N);
  if (P <= 1) {  // one workgroup is the whole tree (N == 0: it reads nothing and writes 0)
    hipLaunchKernelGGL(sq_norm_partial, dim3(1), dim3(256), 0, st, N, d_g, d_sq_norm);
    return check_launch("sq_norm_partial");
  }
  HP_REQUIRE(d_ws && ws_floats >= P, "hp_grad_sq_norm: workspace too small (hp_grad_sq_norm_ws_floats)");
  hipLaunchKernelGGL(sq_norm_partial, dim3((unsigned)P), dim3(256), 0, st, N, d_g, d_ws);
  int rc = check_launch("sq_norm_partial");
  if (rc) return rc;
  hipLaunchKernelGGL(sq_norm_final, dim3(1), dim3(256), 0, st, P, d_ws, d_sq_norm);
  return check_launch("sq_norm_final");
}

extern "C" int hp_adamw_step(int64_t N, float* d_p, const float* d_g, float* d_m, float* d_v, double lr, double beta1, double beta2, double eps,
                             double weight_decay, int64_t step, int decoupled, const float* d_sq_norm, const float* d_max_norm, void* stream) {
  HP_REQUIRE(N >= 0 && N <= 0x7fffffff, "hp_adamw_step: element count outside 0 .. 2^31 - 1");
  HP_REQUIRE(step >= 1, "hp_adamw_step: step counts from 1");
  HP_REQUIRE(lr >= 0.0 && eps >= 0.0 && weight_decay >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
             "hp_adamw_step: lr, eps, weight_decay >= 0 and betas in [0, 1) (NaN is refused)");
  HP_REQUIRE((d_sq_norm == nullptr) == (d_max_norm == nullptr), "hp_adamw_step: the squared norm and max_norm come together or not at all");
  if (N == 0) return HP_OK;
  HP_REQUIRE(d_p && d_g && d_m && d_v, "hp_adamw_step: null pointer");
  // the host scalars as torch forms them: Python floats (double), rounded to float32 where an elementwise operation consumes them
  const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
  AdamScalars a;
  a.one_minus_beta1 = (float)(1.0 - beta1);
  a.beta2 = (float)beta2;
  a.one_minus_beta2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  a.weight_decay = (float)weight_decay;
  a.decay_factor = (float)(1.0 - lr * weight_decay);
  a.step_size = (float)(lr / bc1);
  a.bc2_sqrt = (float)std::sqrt(bc2);
  a.decoupled = decoupled ? 1 : 0;
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, d_p, d_g, d_m, d_v, a,
                     d_sq_norm, d_max_norm);
  return check_launch("adamw_kernel");
}
