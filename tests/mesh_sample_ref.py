"""NumPy restatement of mesh surface resampling, written from its definition (include/happypose_amd.h, "Mesh surface
resampling"), and of the ModelNet meter's quantities in float64.  Test infrastructure: it imports nothing from happypose_amd.
The CPU tests (tests/test_mesh_sample_reference.py) check the restatement itself and measure its own float32-vs-float64 error;
the GPU tests (tests/test_gpu_mesh_sample.py) compare the kernels with it.
"""

from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # key increments
MASK32 = 0xFFFFFFFF
SCAN_CHUNK = 1024  # faces per step of the device's scan (csrc/mesh_sample.hip: kScanChunk): what the grid meshes straddle


# ---- random numbers ---------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 in uint64 arithmetic.  ``counter [n, 4]``, ``key (k0, k1)``; returns ``[n, 4]`` uint64 holding 32-bit words."""
    c = np.asarray(counter, dtype=np.uint64).reshape(-1, 4).copy()
    k0, k1 = np.uint64(key[0] & MASK32), np.uint64(key[1] & MASK32)
    mask, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[:, 0], np.uint64(M1) * c[:, 2]  # 32 x 32 bits: no overflow in 64
        c = np.stack([(p1 >> s32) ^ c[:, 1] ^ k0, p1 & mask, (p0 >> s32) ^ c[:, 3] ^ k1, p0 & mask], axis=1)
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return c


def sample_words(n_samples: int, seed: int, obj: int):
    """``r0..r3`` of samples ``0 .. n_samples - 1`` of object ``obj``: counter ``(i, obj, 0, 0)``, key ``(seed lo, seed hi)``."""
    counter = np.zeros((n_samples, 4), np.uint64)
    counter[:, 0] = np.arange(n_samples, dtype=np.uint64)
    counter[:, 1] = obj
    return philox4x32_10(counter, (seed & MASK32, (seed >> 32) & MASK32))


# ---- areas, CDF, face pick, point --------------------------------------------------------------------------------------------------
def face_areas(vertices, faces) -> np.ndarray:
    """``0.5 |(v1 - v0) x (v2 - v0)|`` in float64 from the float32 vertices, component order as in the header."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    a, b = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def cdf(areas) -> np.ndarray:
    """Inclusive prefix sum in float64, summed in sequence."""
    return np.cumsum(np.asarray(areas, np.float64))  # numpy's cumsum adds one term after the other


def reflect(ia, ib):
    """The integer reflection: where ``ia + ib > 2^24`` both become ``2^24 - i``."""
    ia, ib = np.asarray(ia, np.int64), np.asarray(ib, np.int64)
    over = ia + ib > (1 << 24)
    return np.where(over, (1 << 24) - ia, ia), np.where(over, (1 << 24) - ib, ib)


def points_from(vertices, faces, face_id, ia, ib, dtype):
    """``p = (v0 + a (v1 - v0)) + b (v2 - v0)`` evaluated in ``dtype`` (float64, or float32 with every operation rounded once)."""
    v = np.asarray(vertices, np.float32).astype(dtype)
    f = np.asarray(faces).reshape(-1, 3)[face_id]
    a = (np.asarray(ia, np.float64) * 2.0 ** -24).astype(dtype)[:, None]  # exact in both types
    b = (np.asarray(ib, np.float64) * 2.0 ** -24).astype(dtype)[:, None]
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    p = (v0 + a * (v1 - v0)) + b * (v2 - v0)
    assert p.dtype == dtype
    return p


def sample(vertices, faces, n_samples: int, seed: int = 0, obj: int = 0) -> dict:
    """The whole definition for one object.  ``face_id``, ``margin`` (``min |pick - cum boundary| / total`` per sample),
    ``ia`` / ``ib`` after the reflection, ``p64`` / ``p32`` and ``total``."""
    faces = np.asarray(faces).reshape(-1, 3)
    cum = cdf(face_areas(vertices, faces))
    total, F = cum[-1], len(cum)
    r = sample_words(n_samples, seed, obj)
    u = ((r[:, 0] << np.uint64(21)) | (r[:, 1] >> np.uint64(11))).astype(np.float64) * 2.0 ** -53  # 53 bits: exact
    pick = u * total
    first = np.searchsorted(cum, pick, side="right")  # the first f with cum[f] > pick
    face_id = np.minimum(first, F - 1)
    below, above = cum[np.maximum(first - 1, 0)], cum[np.minimum(first, F - 1)]
    margin = np.minimum(np.where(first > 0, np.abs(pick - below), np.inf), np.abs(above - pick)) / total
    ia, ib = reflect(r[:, 2] >> np.uint64(8), r[:, 3] >> np.uint64(8))
    return {"face_id": face_id.astype(np.int32), "margin": margin, "ia": ia, "ib": ib, "total": total, "cum": cum,
            "p64": points_from(vertices, faces, face_id, ia, ib, np.float64),
            "p32": points_from(vertices, faces, face_id, ia, ib, np.float32)}


def barycentric(vertices, faces, face_id, p):
    """``(a, b)`` with ``p = v0 + a (v1 - v0) + b (v2 - v0)`` in the least-squares sense, and the distance of ``p`` to that plane
    point; float64."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces).reshape(-1, 3)[face_id]
    e1, e2, d = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], np.asarray(p, np.float64) - v[f[:, 0]]
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (d * e1).sum(1), (d * e2).sum(1)
    det = g11 * g22 - g12 * g12
    a, b = (r1 * g22 - r2 * g12) / det, (r2 * g11 - r1 * g12) / det
    return a, b, np.linalg.norm(d - a[:, None] * e1 - b[:, None] * e2, axis=1)


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------
MARGIN_MIN = 1e-9          # a sample whose pick lies closer to a CDF boundary than this (relative to the total) is left out
EXCLUDED_SHARE_CAP = 1e-3  # at most 0.1 % of a case's samples may be left out
SEED = 0x5EED0123456789AB  # both key words in use
N_SAMPLES = (1, 63, 64, 65, 1000, 4096)
OBJECTS = (0, 1, 2)        # the object indices the GPU tests place a case at


def tetrahedron():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 3.0]], np.float32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)


def cube_with_zero_area_faces():
    """12 faces of a cube plus two zero-area faces (three collinear points; a repeated vertex), one of them last."""
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.25, 0.75) for z in (0.0, 1.5)] + [[-0.5, -0.25, 0.75]], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    f.insert(5, (0, 8, 1))  # vertex 8 is the midpoint of the edge 0 - 1
    f.append((0, 1, 0))
    return v, np.asarray(f, np.int32)


def single_triangle():
    return np.array([[0.25, -1.0, 2.0], [3.0, 0.5, 2.5], [-1.0, 4.0, 0.125]], np.float32), np.array([[0, 1, 2]], np.int32)


def grid(n_faces: int):
    """A bumpy strip of ``n_faces`` triangles of unequal area (widths and heights vary with periods 7 and 3)."""
    n_cols = (n_faces + 1) // 2
    x = np.cumsum(0.01 + 0.002 * (np.arange(n_cols + 1) % 7))
    v = np.zeros((2 * (n_cols + 1), 3))
    v[0::2, 0], v[1::2, 0] = x, x
    v[1::2, 1] = 0.05 + 0.01 * (np.arange(n_cols + 1) % 3)
    v[:, 2] = 0.003 * np.sin(np.arange(len(v)))
    f = []
    for c in range(n_cols):
        f += [(2 * c, 2 * c + 2, 2 * c + 1), (2 * c + 1, 2 * c + 2, 2 * c + 3)]
    return v.astype(np.float32), np.asarray(f[:n_faces], np.int32)


GRID_FACES = (SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 2 * SCAN_CHUNK + 1)  # around one and two chunks of the scan


def cases(golden_dir) -> dict:
    """name -> (vertices float32, faces int32) of every mesh the GPU tests sample."""
    out = {"tetrahedron": tetrahedron(), "cube": cube_with_zero_area_faces(), "triangle": single_triangle()}
    for n in GRID_FACES:
        out[f"grid{n}"] = grid(n)
    z = np.load(golden_dir / "obj_000001.npz")
    out["golden"] = (z["vertices"].astype(np.float32), z["faces"].astype(np.int32))
    return out


RAGGED = ("cube", "grid1025", "tetrahedron")  # the three objects of the one ragged call, at object indices 0, 1, 2


def point_error(vertices, faces, objects=OBJECTS, n_samples=max(N_SAMPLES), seed=SEED) -> float:
    """The restatement's own float32-vs-float64 difference of the points of one mesh: the largest ``|p32 - p64|`` over the
    samples the GPU tests draw (every object index in use)."""
    worst = 0.0
    for o in objects:
        s = sample(vertices, faces, n_samples, seed, o)
        worst = max(worst, float(np.linalg.norm(s["p32"].astype(np.float64) - s["p64"], axis=1).max()))
    return worst


# point_error() of every case, as measured by tests/test_mesh_sample_reference.py::test_point_yardstick (which asserts them).
# The GPU tests hold the kernel's points to POINT_MARGIN x these, with a floor of one float32 ulp of the mesh's largest coordinate.
POINT_MARGIN = 4.0
POINT_F32_ERROR = {
    "tetrahedron": 1.1920928955078125e-07, "cube": 1.1920928955078125e-07, "triangle": 3.7342202920143806e-07,
    "grid1023": 8.42044894482674e-07, "grid1024": 8.323367563265532e-07, "grid1025": 8.931695864350545e-07,
    "grid2049": 1.8875989669096765e-06, "golden": 8.134242927909705e-06,
}


def point_bound(name: str, vertices) -> float:
    big = np.float32(np.abs(vertices).max())
    return max(POINT_MARGIN * POINT_F32_ERROR[name], float(np.spacing(big)))


# ---- ModelNet quantities in float64 ------------------------------------------------------------------------------------------------
def quaternion(R) -> np.ndarray:
    """Unit quaternion ``(w, x, y, z)`` of a rotation matrix (largest component first computed: Shepperd's method)."""
    R = np.asarray(R, np.float64)
    t = np.trace(R)
    cand = np.array([t, R[0, 0], R[1, 1], R[2, 2]])
    k = int(np.argmax(cand))
    if k == 0:
        q = np.array([1.0 + t, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], 1.0 + 2 * R[0, 0] - t, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1.0 + 2 * R[1, 1] - t, R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 + 2 * R[2, 2] - t])
    return q / np.linalg.norm(q)


def modelnet_errors(T_pred, T_gt, K, points) -> dict:
    """``add``, ``diameter``, ``proj_error``, ``trans_dist`` and ``angular_dist`` (degrees) of one match, float64.  ``points``: the
    object's own points ``[n, 3]``."""
    T_pred, T_gt, K, pts = (np.asarray(a, np.float64) for a in (T_pred, T_gt, K, points))
    tr = lambda T: pts @ T[:3, :3].T + T[:3, 3]  # noqa: E731

    def project(T):
        suv = tr(T) @ K.T
        return suv[:, :2] / suv[:, 2:3]

    dot = abs(float(quaternion(T_gt[:3, :3]) @ quaternion(T_pred[:3, :3])))
    return {"add": np.linalg.norm(tr(T_gt) - tr(T_pred), axis=1).mean(),
            "diameter": np.linalg.norm(pts.max(0) - pts.min(0)),
            "proj_error": np.linalg.norm(project(T_pred) - project(T_gt), axis=1).mean(),
            "trans_dist": np.linalg.norm(T_gt[:3, 3] - T_pred[:3, 3]),
            "angular_dist": np.rad2deg(2.0 * np.arccos(min(dot, 1.0 - 1e-7)))}


def modelnet_summary(rows) -> dict:
    add = np.mean([r["add"] < 0.1 * r["diameter"] for r in rows])
    rot_trans = np.mean([r["trans_dist"] < 0.05 and r["angular_dist"] < 5 for r in rows])
    return {"add0.1d": add, "5deg_5cm": rot_trans, "proj2d_5px": np.mean([r["proj_error"] < 5 for r in rows])}
