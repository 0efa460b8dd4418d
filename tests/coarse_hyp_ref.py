"""NumPy restatement of the coarse classifier's training inputs and loss, written from their definitions in
include/happypose_amd.h (hp_views_sphere26, hp_coarse_hypotheses, hp_loss_bce_logits): the 26 offsets, the look-at with the
library's degenerate rule, the in-plane quarter turns, the Philox draw and the BCE value and gradient.  Test infrastructure: it
imports nothing from happypose_amd.  tests/test_coarse_hyp_reference.py checks the restatement itself on the CPU,
tests/test_gpu_coarse_hyp.py and tests/test_gpu_coarse_training.py compare the kernels with it.

The look-at is float64, the tail ``invert_transform_matrices(TC0_CV) @ TCO`` float32 -- the arithmetic of
``oracle.geometry.make_TCO_multiview`` for the front views, so the bound of that comparison carries over.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from mesh_sample_ref import MASK32, philox4x32_10  # noqa: E402

N_VIEWS, N_CANDIDATES = 26, 104
DEGENERATE = 1e-9
UP = np.array([0.0, -1.0, 0.0])  # camera 0's up (Panda z) in OpenCV axes


def offsets() -> np.ndarray:
    """``[26, 3]`` camera positions in units of ``|tCR|`` (Panda frame of the re-aimed camera 0: x right, y forward, z up) in the
    reference's loop order, without ``(0, 1, 0)``, the reference point itself."""
    out = [(x, y, z) for y in (0, 1, 2) for x in (0, -1, 1) for z in (0, 1, -1) if (x, y, z) != (0, 1, 0)]
    assert len(out) == N_VIEWS
    return np.asarray(out, np.float64)


def look_at(pos, target, fallback_right=None):
    """Pose (camera -> camera 0, OpenCV axes) of a camera at ``pos`` whose +z passes through ``target``; ``(T, |f x up|)``.  Where
    ``|f x up| < 1e-9`` and a fallback is given, ``right`` is the fallback."""
    f = target - pos
    f = f / np.linalg.norm(f)
    right = np.cross(f, UP)
    n = float(np.linalg.norm(right))
    right = fallback_right if (fallback_right is not None and n < DEGENERATE) else right / n
    upp = np.cross(right, f)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = right, -upp, f, pos
    return T, n


def views_TC0_CV(tCR, return_cross=False):
    """``[26, 4, 4]`` float64: the candidate cameras of ONE pose with respect to camera 0.  A non-finite or zero ``tCR``: identities."""
    tCR = np.asarray(tCR, np.float64)
    radius = float(np.linalg.norm(tCR)) if np.isfinite(tCR).all() else 0.0
    if radius == 0.0:
        out = np.tile(np.eye(4), (N_VIEWS, 1, 1))
        return (out, np.ones(N_VIEWS)) if return_cross else out
    base, _ = look_at(np.zeros(3), tCR)
    views, cross = [], []
    for ox, oy, oz in offsets():
        pos = radius * (ox * base[:3, 0] + oy * base[:3, 2] - oz * base[:3, 1])
        T, n = look_at(pos, tCR, base[:3, 0])
        views.append(T)
        cross.append(n)
    return (np.stack(views), np.asarray(cross)) if return_cross else np.stack(views)


def cross_norms(TCO, tCR=None) -> np.ndarray:
    """``[B, 26]``: ``|f x up|`` of every candidate's look-at (1 where the pose takes the identity view)."""
    TCO = np.asarray(TCO, np.float32)
    tCR = TCO[:, :3, 3] if tCR is None else np.asarray(tCR, np.float32)
    ok = np.isfinite(TCO[:, :3].reshape(len(TCO), -1)).all(1)
    return np.stack([views_TC0_CV(tCR[b] if ok[b] else np.zeros(3), True)[1] for b in range(len(TCO))])


QUARTER_TURNS = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]],
                          [[-1, 0, 0], [0, -1, 0], [0, 0, 1]], [[0, 1, 0], [-1, 0, 0], [0, 0, 1]]], np.float64)  # Rz(rot pi / 2), exact


def views_sphere26(TCO, tCR=None, inplane_rotations=True) -> np.ndarray:
    """``[B, 104, 4, 4]`` (or ``[B, 26, 4, 4]``) float32: candidate ``view * 4 + rot``."""
    TCO = np.asarray(TCO, np.float32)
    B = len(TCO)
    tCR = TCO[:, :3, 3] if tCR is None else np.asarray(tCR, np.float32)
    ok = np.isfinite(TCO[:, :3].reshape(B, -1)).all(1)
    TC0_CV = np.stack([views_TC0_CV(tCR[b] if ok[b] else np.zeros(3)) for b in range(B)]).astype(np.float32)
    R, t = TC0_CV[..., :3, :3], TC0_CV[..., :3, 3]
    inv = np.zeros_like(TC0_CV)  # invert_transform_matrices: R^T, -R^T t
    inv[..., :3, :3] = np.swapaxes(R, -1, -2)
    inv[..., :3, 3] = -(np.swapaxes(R, -1, -2) @ t[..., None])[..., 0]
    inv[..., 3, 3] = 1
    with np.errstate(invalid="ignore"):
        TCV_O = (inv @ TCO[:, None]).astype(np.float32)
    TCV_O[:, :, 3] = TCO[:, None, 3]  # the definition copies the pose's bottom row (a product would spread a NaN of the pose into it)
    if not inplane_rotations:
        return TCV_O
    out = np.repeat(TCV_O[:, :, None], 4, axis=2)
    for rot in range(1, 4):
        with np.errstate(invalid="ignore"):
            out[:, :, rot, :3, :3] = QUARTER_TURNS[rot].astype(np.float32) @ TCV_O[:, :, :3, :3]
    return out.reshape(B, N_CANDIDATES, 4, 4)


# ---- the draw -------------------------------------------------------------------------------------------------------------------------
def hyp_words(n, seed, row_offset=0) -> np.ndarray:
    """``[n, 108]``: the Philox words of images ``row_offset .. row_offset + n - 1``, counters ``(row lo, row hi, j, 0)``, ``j = 0 .. 26``."""
    rows = np.arange(n, dtype=np.uint64) + np.uint64(row_offset)
    words = []
    for j in range(N_CANDIDATES // 4 + 1):
        c = np.zeros((n, 4), np.uint64)
        c[:, 0], c[:, 1], c[:, 2] = rows & np.uint64(MASK32), rows >> np.uint64(32), j
        words.append(philox4x32_10(c, (seed & MASK32, (seed >> 32) & MASK32)))
    return np.concatenate(words, axis=1)


def draw(n, n_hyp, seed, row_offset=0, n_rendered_views=1, p_force_positive=0.7):
    """``(view_ids [n, n_hyp] int32, is_positive [n, n_hyp] float32)``: partial Fisher-Yates over ``0 .. 103`` with
    ``k = i + floor(w[i] (104 - i) / 2^32)``; where id 0 is absent and ``w[104] > floor((1 - p) 2^32)``, slot
    ``floor(w[105] n_rendered_views / 2^32)`` becomes id 0."""
    assert 1 <= n_hyp <= N_CANDIDATES and 1 <= n_rendered_views <= n_hyp
    w = hyp_words(n, seed, row_offset)
    threshold = min(int((1.0 - p_force_positive) * 4294967296.0), MASK32)
    ids = np.empty((n, n_hyp), np.int32)
    for b in range(n):
        perm = list(range(N_CANDIDATES))
        for i in range(n_hyp):
            k = i + ((int(w[b, i]) * (N_CANDIDATES - i)) >> 32)
            perm[i], perm[k] = perm[k], perm[i]
        if 0 not in perm[:n_hyp] and int(w[b, N_CANDIDATES]) > threshold:
            perm[(int(w[b, N_CANDIDATES + 1]) * n_rendered_views) >> 32] = 0
        ids[b] = perm[:n_hyp]
    return ids, (ids == 0).astype(np.float32)


# ---- the loss -------------------------------------------------------------------------------------------------------------------------
def bce_logits(logits, y, temperature=1.0):
    """float64 ``(loss, d loss / d logits)`` of ``BCEWithLogitsLoss(reduction="none")(logits / temperature, y)``."""
    T = float(np.float32(temperature))
    x, y = np.asarray(logits, np.float64) / T, np.asarray(y, np.float64)
    e = np.exp(-np.abs(x))
    loss = np.maximum(x, 0.0) - x * y + np.log1p(e)
    sig = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return loss, (sig - y) / T


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
SEED = 0x0FEDCBA987654321


def rotation(rs) -> np.ndarray:
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    return q * np.sign(np.linalg.det(q))


def poses(B: int, seed: int = 0) -> np.ndarray:
    """``[B, 4, 4]`` float32 in front of the camera.  The first rows are the special ones: 0 has ``tCR_y`` exactly 0 (the degenerate
    look-at of offsets ``(0, 1, +-1)``), 1 lies on the optical axis (``tCR_y`` is 0 there too), 2 (when ``B > 2``) is non-finite."""
    rs = np.random.RandomState(seed)
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    for b in range(B):
        T[b, :3, :3] = rotation(rs)
        T[b, :3, 3] = [rs.uniform(-0.3, 0.3), rs.uniform(-0.25, 0.25), rs.uniform(0.5, 1.5)]
    T[0, 1, 3] = 0.0
    if B > 1:
        T[1, :2, 3] = 0.0
    if B > 2:
        T[2, 0, 1] = np.nan
    return T
