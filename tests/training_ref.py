"""NumPy restatement of the hypothesis generation and the meter arithmetic of the trainers' forward-loss step, written from the
definitions in include/happypose_amd.h (hp_pose_add_noise, hp_tco_init_from_boxes) and the reference's two forward-loss
functions.  Test infrastructure: it imports nothing from happypose_amd.  The CPU tests (tests/test_training_reference.py) check
the restatement itself; the GPU tests (tests/test_gpu_training.py) compare the kernels with it.

Every function takes ``dtype``: float64 is the reference, float32 (every operation rounded once, in the order written) is the
yardstick -- the GPU tests allow the kernels ``MARGIN`` x the float32 evaluation's own distance from the float64 one on the inputs
they use.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from mesh_sample_ref import MASK32, philox4x32_10  # noqa: E402

MARGIN = 4.0


# ---- add_noise ----------------------------------------------------------------------------------------------------------------------
def euler2mat(angles, dtype=np.float64, axes="sxyz"):
    """``[n, 3]`` angles ``(ai, aj, ak)`` in radians -> ``[n, 3, 3]``.  ``sxyz`` (static axes, transforms3d's default):
    ``Rz(ak) Ry(aj) Rx(ai)``; ``rxyz`` (rotating axes, NOT what the reference uses): ``Rx(ai) Ry(aj) Rz(ak)``."""
    a = np.asarray(angles).astype(dtype).reshape(-1, 3)
    if axes == "rxyz":  # r-xyz(ai, aj, ak) == s-zyx(ak, aj, ai): the same formula with the first and last angle exchanged ...
        return np.ascontiguousarray(euler2mat(-a, dtype, "sxyz").transpose(0, 2, 1))  # ... here through (Rz(-ak) Ry(-aj) Rx(-ai))^T
    assert axes == "sxyz"
    cx, sx, cy, sy, cz, sz = np.cos(a[:, 0]), np.sin(a[:, 0]), np.cos(a[:, 1]), np.sin(a[:, 1]), np.cos(a[:, 2]), np.sin(a[:, 2])
    R = np.empty((len(a), 3, 3), dtype)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = -sy, sx * cy, cx * cy
    assert R.dtype == dtype
    return R


def add_noise(TCO, noise, repeat=1, dtype=np.float64, axes="sxyz"):
    """``TCO [m, 4, 4]`` float32, ``noise [m * repeat, 6]`` float32 (angles in radians, metres) -> ``[m * repeat, 4, 4]`` in
    ``dtype``: ``R R_noise``, ``t + dt``, bottom row copied."""
    T = np.repeat(np.asarray(TCO, np.float32), repeat, axis=0).astype(dtype)
    nz = np.asarray(noise, np.float32).astype(dtype)
    Rn = euler2mat(nz[:, :3], dtype, axes)
    out = T.copy()
    R = T[:, :3, :3]
    for c in range(3):  # (R[r, 0] Rn[0, c] + R[r, 1] Rn[1, c]) + R[r, 2] Rn[2, c]
        out[:, :3, c] = (R[:, :, 0] * Rn[:, None, 0, c] + R[:, :, 1] * Rn[:, None, 1, c]) + R[:, :, 2] * Rn[:, None, 2, c]
    out[:, :3, 3] = T[:, :3, 3] + nz[:, 3:]
    assert out.dtype == dtype
    return out


def noise_words(n, seed, row_offset=0):
    """The eight Philox words of rows ``row_offset .. row_offset + n - 1``: counters ``(row lo, row hi, j, 0)``, ``j = 0, 1``."""
    rows = (np.arange(n, dtype=np.uint64) + np.uint64(row_offset))
    words = []
    for j in range(2):
        c = np.zeros((n, 4), np.uint64)
        c[:, 0], c[:, 1], c[:, 2] = rows & np.uint64(MASK32), rows >> np.uint64(32), j
        words.append(philox4x32_10(c, (seed & MASK32, (seed >> 32) & MASK32)))
    return np.concatenate(words, axis=1)


def normals(n, seed, row_offset=0, dtype=np.float64):
    """The six standard normals of every row, ``[n, 6]``: Box-Muller pairs from the words ``(w[2 p], w[2 p + 1])``, ``p = 0, 1, 2``."""
    w = noise_words(n, seed, row_offset)
    z = np.empty((n, 6), dtype)
    two_pi = dtype(2.0 * np.pi)
    for p in range(3):
        u1 = (((w[:, 2 * p] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24).astype(dtype)  # exact in both types
        u2 = ((w[:, 2 * p + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(dtype)
        r, a = np.sqrt(dtype(-2.0) * np.log(u1)), two_pi * u2
        z[:, 2 * p], z[:, 2 * p + 1] = r * np.cos(a), r * np.sin(a)
    assert z.dtype == dtype
    return z


def draw_noise(n, seed, row_offset, euler_deg_std, trans_std, dtype=np.float64):
    """``[n, 6]``: the angles in radians and the translation.  The standard deviations are the float32 values the entry point takes."""
    z = normals(n, seed, row_offset, dtype)
    e = np.asarray(euler_deg_std, np.float32).astype(dtype) * dtype(np.pi / 180.0)
    t = np.asarray(trans_std, np.float32).astype(dtype)
    out = z * np.concatenate([e, t])[None]
    assert out.dtype == dtype
    return out


# ---- TCO_init_from_boxes ------------------------------------------------------------------------------------------------------------
def TCO_init_from_boxes(z_range, boxes, K, dtype=np.float64):
    boxes, K = np.asarray(boxes, np.float32).astype(dtype), np.asarray(K, np.float32).astype(dtype)
    zr = np.asarray(z_range, np.float32).astype(dtype)
    z = (zr[0] + zr[1]) / dtype(2)
    out = np.tile(np.eye(4, dtype=dtype), (len(boxes), 1, 1))
    out[:, 0, 3] = (((boxes[:, 0] + boxes[:, 2]) / dtype(2) - K[:, 0, 2]) * z) / K[:, 0, 0]
    out[:, 1, 3] = (((boxes[:, 1] + boxes[:, 3]) / dtype(2) - K[:, 1, 2]) * z) / K[:, 1, 1]
    out[:, 2, 3] = z
    return out


# ---- meters -------------------------------------------------------------------------------------------------------------------------
def megapose_meters(losses, parts, batch_size, n_hypotheses, alpha=1.0):
    """``losses``: per iteration ``[B * n_hypotheses]``, ``parts``: per iteration ``{loss_orn, loss_xy, loss_z: [B * n_hypotheses]}``
    -> ``({key: value}, loss_total)`` by the reference's formulas, float64."""
    m = {}
    per_iter = []
    for n, (l, p) in enumerate(zip(losses, parts)):
        l = np.asarray(l, np.float64).reshape(batch_size, n_hypotheses)
        m[f"loss_TCO-iter={n + 1}"] = l.mean()
        for key in ("loss_orn", "loss_xy", "loss_z"):
            m[f"loss_TCO-iter={n + 1}-{key}"] = np.asarray(p[key], np.float64).reshape(batch_size, n_hypotheses).mean()
        per_iter.append(l)
    losses_pose = np.stack(per_iter).transpose(1, 2, 0)  # [B, n_hypotheses, n_iterations]
    m["loss_TCO"] = losses_pose.mean(axis=(-1, -2)).mean()
    m["loss_total"] = (alpha * losses_pose).mean()
    return m, m["loss_total"]


def h_pose_meters(losses):
    m = {f"loss_TCO-iter={n + 1}": np.asarray(l, np.float64).mean() for n, l in enumerate(losses)}
    m["loss_TCO"] = m["loss_total"] = np.concatenate([np.asarray(l, np.float64) for l in losses]).mean()
    return m, m["loss_total"]


def megapose_meter_keys(n_iterations):
    keys = {"time_render", "loss_TCO", "loss_total"}
    for n in range(1, n_iterations + 1):
        keys |= {f"loss_TCO-iter={n}"} | {f"loss_TCO-iter={n}-{k}" for k in ("loss_orn", "loss_xy", "loss_z")}
    return keys


def h_pose_meter_keys(n_iterations):
    return {"loss_TCO", "loss_total"} | {f"loss_TCO-iter={n}" for n in range(1, n_iterations + 1)}


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------
SEED = 0x0123456789ABCDEF
EXPLICIT_CASES = ((1, 1), (63, 1), (64, 1), (65, 1), (257, 1), (195, 3))  # (n, repeat)
EULER_DEG_STD, TRANS_STD = (15.0, 15.0, 15.0), (0.01, 0.01, 0.05)
BIG_ANGLES = np.array([[1.0, -0.7, 2.0], [-2.5, 1.2, 0.4]], np.float32)  # rxyz and sxyz differ by O(1) here


def random_poses(rs, m):
    q = rs.normal(size=(m, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    T = np.tile(np.eye(4), (m, 1, 1))
    T[:, :3, :3] = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                             2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                             2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(m, 3, 3)
    T[:, :3, 3] = rs.uniform(-0.3, 0.3, (m, 3)) + np.array([0.0, 0.0, 0.8])
    return T.astype(np.float32)


def explicit_case(n, repeat):
    """Host-seeded poses ``[n / repeat, 4, 4]`` and noise ``[n, 6]`` (the reference's training magnitudes), float32."""
    rs = np.random.RandomState(1000 * n + repeat)
    TCO = random_poses(rs, n // repeat)
    noise = rs.normal(size=(n, 6)) * np.concatenate([np.deg2rad(EULER_DEG_STD), TRANS_STD])
    return TCO, noise.astype(np.float32)


def yardstick(f32, f64):
    """Largest distance of the float32 evaluation from the float64 one."""
    return float(np.abs(np.asarray(f32, np.float64) - f64).max())
