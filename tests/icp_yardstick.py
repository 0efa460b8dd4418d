"""Yardsticks of the depth refiner's GPU tests: how far a float32 evaluation of the definition lies from the float64 reference
(tests/icp_ref.py).  Unlike the reference, this module knows the kernels' order of summation and where they round; nothing here
is compared with a kernel, it only sizes the bounds.  Every figure below is measured and asserted by tests/test_icp_reference.py
on the CPU; tests/test_gpu_icp_stages.py allows the kernels 4x."""

import numpy as np

import icp_ref as R


def kernel_order_sum(terms, pixels, HW):
    """The sums of ``terms [N, 32]`` float32 at the flat pixel indices ``pixels`` in the order of the accumulate and update
    kernels: 64 blocks of ``ceil(HW / 64)`` pixels, 256 lanes striding through a block, the butterfly over the 64 lanes of a
    wave, the 4 waves in turn (all float32), then the 64 blocks in float64."""
    terms = np.asarray(terms, np.float32)
    per = -(-HW // R.N_BLOCKS)
    trips = -(-per // 256)
    grid = np.zeros((R.N_BLOCKS, trips * 256, terms.shape[1]), np.float32)
    grid[pixels // per, pixels % per] = terms
    acc = np.zeros((R.N_BLOCKS, 256, terms.shape[1]), np.float32)
    for k in range(trips):
        acc = acc + grid[:, k * 256:(k + 1) * 256]
    s = acc.reshape(R.N_BLOCKS, 4, 64, -1)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lanes ^ off]
    w = s[:, :, 0]
    block = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    return block.astype(np.float64).sum(0)


def refine_f32(depth_rendered, depth_measured, mask, K, TCO, n_iterations, tolerance, depth_delta_thresh, tgt):
    """An accepted run evaluated as the kernels evaluate it: float32 per-pixel terms added in the kernels' order, the 64 partials,
    the solution and the composition in float64, the increment kept in float32, the pose product in float32.  Returns
    ``(pose [4, 4] float32, inliers, residual)``: the size of a float32 evaluation's error on a whole run."""
    HW = np.size(depth_rendered)
    args = (depth_rendered, depth_measured, mask, K, np.asarray(tgt, np.float32), tolerance, depth_delta_thresh)
    sums = lambda a: kernel_order_sum(a["terms"], a["pixels"], HW)  # noqa: E731
    s = sums(R.accumulate_terms(0, None, *args, dtype=np.float32))
    T = np.concatenate([np.eye(3), ((s[3:6] - s[0:3]) / s[27])[:, None]], 1).astype(np.float32)
    for _ in range(n_iterations):
        x = R.solve_increment(sums(R.accumulate_terms(1, T, *args, dtype=np.float32)))
        T = R.compose(T.astype(np.float64), x).astype(np.float32)
    s = sums(R.accumulate_terms(1, T, *args, dtype=np.float32))
    P, out = np.asarray(TCO, np.float32), np.eye(4, dtype=np.float32)
    for j in range(4):
        v = (T[:, 0] * P[0, j] + T[:, 1] * P[1, j]) + T[:, 2] * P[2, j]
        out[:3, j] = v + T[:, 3] if j == 3 else v
    return out, int(s[27]), float(np.float32(np.sqrt(s[28] / s[27])))


# Accumulators by the size of a float32 evaluation's error: sums of points and of J J' against those that hold the residual.
ACC_GROUPS = {"geometry": np.r_[0:21, 27], "residual": np.r_[21:27, 28]}
# |kernel_order_sum(float32 terms) - float64 sum| / sum|term|, worst over every case of icp_ref.accumulate_cases.
MEASURED_F32_ERROR = {"geometry": 9.1e-7, "residual": 1.17e-5}
# Full runs: refine_f32 (on the float32 table of oracle/icp.py and on the rounded float64 table) against icp_ref.refine, worst over
# the predictions: largest difference of a rotation entry, of a translation entry in metres, of the residual relative to it.
# At 37x53, 1 and 2 iterations, threshold and mask (oracle/icp.py, which rounds less, is within 1.4e-7, 6.0e-8, 1.5e-6):
MEASURED_F32_RUN = {"rotation": 5.6e-7, "translation": 7.8e-8, "residual": 2.9e-6}
# and on the five predictions of the large call of the workspace test (120x160, 2 iterations, threshold):
MEASURED_F32_RUN_LARGE = {"rotation": 9.4e-8, "translation": 7.4e-8, "residual": 6.5e-6}
# Largest angle (rad) between the normals of oracle/icp.py's float32 table and the reference's, over the 3 images x 3 shapes of
# the GPU table test.
NORMAL_ANGLE_F32 = 7.2e-5
# oracle/icp.py against icp_ref.refine on the plane case (37x53, 2 iterations): largest pose entry difference, residual relative.
PLANE_F32 = {"pose": 3.4e-8, "residual": 1.9e-6}
