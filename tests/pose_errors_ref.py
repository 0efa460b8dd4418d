"""float64 restatement of the pose-error metrics, written from their definitions (include/happypose_amd.h, "Pose-error
metrics"); numpy only.  Test infrastructure: the CPU tests measure the reference's float32 error against it, the GPU tests
compare the kernels with it.

Every function scores ONE row: ``T_pred`` / ``T_gt`` are 4 x 4, ``pts`` is ``[n, 3]`` (the points that count, already cut to the
object's ``n_pts``), ``syms`` is ``[n_sym, 4, 4]``.  All return a dict with ``norm_avg``, ``xyz_avg [3]``, ``norm_max``,
``sym_id``, ``dists [n, 3]`` and ``assign [n]``.
"""

from __future__ import annotations

import numpy as np

MODES = ("ADD", "ADD-S", "ADD-SYM", "MSSD", "MSPD")


def transform(T, pts):
    T, pts = np.asarray(T, np.float64), np.asarray(pts, np.float64)
    return pts @ T[:3, :3].T + T[:3, 3]


def project(K, T, pts):
    suv = transform(T, pts) @ np.asarray(K, np.float64).T
    return suv[:, :2] / suv[:, 2:3]


def _pack(dists, sym_id, assign):
    norms = np.linalg.norm(dists, axis=-1)
    return {"norm_avg": norms.mean(), "xyz_avg": np.abs(dists).mean(0), "norm_max": norms.max(), "sym_id": sym_id, "dists": dists,
            "assign": assign}


def add(T_pred, T_gt, pts):
    return _pack(transform(T_gt, pts) - transform(T_pred, pts), -1, np.arange(len(pts)))


def squared_distances(T_pred, T_gt, pts, chunk=256):
    """Rows: ground-truth points, columns: predicted points; generated in chunks of rows."""
    a, b = transform(T_gt, pts), transform(T_pred, pts)
    for j0 in range(0, len(a), chunk):
        d = a[j0:j0 + chunk, None] - b[None]
        yield j0, (d * d).sum(-1)


def nearest(T_pred, T_gt, pts):
    """(assign [n], min squared distance [n]) in float64, lowest index on a tie."""
    assign, best = np.zeros(len(pts), np.int64), np.zeros(len(pts))
    for j0, d2 in squared_distances(T_pred, T_gt, pts):
        assign[j0:j0 + len(d2)] = d2.argmin(1)
        best[j0:j0 + len(d2)] = d2.min(1)
    return assign, best


def add_s(T_pred, T_gt, pts, assign=None):
    """ADD-S; with ``assign`` given, the sums for THAT choice of neighbours."""
    if assign is None:
        assign, _ = nearest(T_pred, T_gt, pts)
    assign = np.asarray(assign, np.int64)
    return _pack(transform(T_gt, pts) - transform(T_pred, pts)[assign], -1, assign)


def neighbour_distance(T_pred, T_gt, pts, assign):
    """float64 distance from every ground-truth point to the predicted point ``assign`` names."""
    return np.linalg.norm(transform(T_gt, pts) - transform(T_pred, pts)[np.asarray(assign, np.int64)], axis=-1)


def _over_symmetries(T_pred, T_gt, pts, syms, key, K=None):
    best = None
    for s, S in enumerate(np.asarray(syms, np.float64)):
        M = np.asarray(T_gt, np.float64) @ S
        if K is None:
            d = transform(M, pts) - transform(T_pred, pts)
        else:
            d2 = project(K, M, pts) - project(K, T_pred, pts)
            d = np.concatenate([d2, np.zeros((len(d2), 1))], 1)
        r = _pack(d, s, np.arange(len(pts)))
        if best is None or r[key] < best[key]:  # first strict minimum
            best = r
    return best


def add_sym(T_pred, T_gt, pts, syms):
    return _over_symmetries(T_pred, T_gt, pts, syms, "norm_avg")


def mssd(T_pred, T_gt, pts, syms):
    return _over_symmetries(T_pred, T_gt, pts, syms, "norm_max")


def mspd(T_pred, T_gt, pts, syms, K):
    return _over_symmetries(T_pred, T_gt, pts, syms, "norm_max", K=K)


def row(mode, T_pred, T_gt, pts, syms=None, K=None):
    if mode == "ADD":
        return add(T_pred, T_gt, pts)
    if mode == "ADD-S":
        return add_s(T_pred, T_gt, pts)
    if mode == "ADD-SYM":
        return add_sym(T_pred, T_gt, pts, syms)
    if mode == "MSSD":
        return mssd(T_pred, T_gt, pts, syms)
    if mode == "MSPD":
        return mspd(T_pred, T_gt, pts, syms, K)
    raise ValueError(mode)


def errors_batch(modes, TXO_pred, TXO_gt, obj_ids, points, symmetries, n_sym, n_pts, K=None):
    """Rows of ``ops.pose_errors`` in float64: dict of stacked ``norm_avg``, ``xyz_avg``, ``norm_max``, ``sym_id``, ``TCO_xyz``,
    ``TCO_norm``."""
    out = {k: [] for k in ("norm_avg", "xyz_avg", "norm_max", "sym_id", "TCO_xyz", "TCO_norm")}
    for r, mode in enumerate(modes):
        o = int(obj_ids[r])
        res = row(mode, TXO_pred[r], TXO_gt[r], points[o][:int(n_pts[o])], symmetries[o][:int(n_sym[o])], None if K is None else K[r])
        for k in ("norm_avg", "xyz_avg", "norm_max", "sym_id"):
            out[k].append(res[k])
        dt = np.asarray(TXO_pred[r], np.float64)[:3, 3] - np.asarray(TXO_gt[r], np.float64)[:3, 3]
        out["TCO_xyz"].append(np.abs(dt))
        out["TCO_norm"].append(np.linalg.norm(dt))
    return {k: np.asarray(v) for k, v in out.items()}


# ---- the measured tolerances ("pose-error metrics") ----------------------------------------------------------
MARGIN = 4.0  # the project's standing margin over the reference's own float32 error: FMA contraction and another summation order
_CACHE = {}


def golden_rows(g, cloud):
    """(TXO_pred, TXO_gt, points) of the six rows of one cloud of G12."""
    return g[f"{cloud}/TXO_pred"], g[f"{cloud}/TXO_gt"], g[f"cloud_{cloud}"]


def reference_errors(g) -> dict:
    """Largest deviation of the REFERENCE's float32 run (G12) from this float64 restatement, per quantity.  ADD-S is compared
    under the reference's own neighbours where G12 stores them (``small``), so that a flipped near-tie does not count as
    rounding; the ``large`` ADD-S rows, which store no neighbours, are left out of the measurement."""
    if "errors" in _CACHE:
        return _CACHE["errors"]
    e = {"norm_avg": 0.0, "xyz_avg": 0.0, "norm_max": 0.0, "point": 0.0, "pixel": 0.0}

    def take(res, tag, r):
        e["norm_avg"] = max(e["norm_avg"], abs(float(g[f"{tag}norm_avg"][r]) - res["norm_avg"]))
        e["xyz_avg"] = max(e["xyz_avg"], np.abs(g[f"{tag}xyz_avg"][r].astype(np.float64) - res["xyz_avg"]).max())
        e["norm_max"] = max(e["norm_max"], abs(float(g[f"{tag}norm_max"][r]) - res["norm_max"]))

    for cloud in ("small", "large"):
        pred, gt, pts = golden_rows(g, cloud)
        for r in range(len(pred)):
            take(add(pred[r], gt[r], pts), f"{cloud}/add_", r)
    pred, gt, pts = golden_rows(g, "small")
    for r in range(len(pred)):
        res = add_s(pred[r], gt[r], pts, assign=g["small/adds_assign"][r])
        take(res, "small/adds_", r)
        e["point"] = max(e["point"], np.linalg.norm(g["small/adds_dists"][r].astype(np.float64) - res["dists"], axis=-1).max())
        pix = np.linalg.norm(project(g["K"], gt[r], pts) - project(g["K"], pred[r], pts), axis=-1)
        e["pixel"] = max(e["pixel"], np.abs(g["small/pixel_dists"][r].astype(np.float64) - pix).max())
    for r, o in enumerate(g["sym/obj_id"]):
        res = add_sym(g["sym/TXO_pred"][r], g["sym/TXO_gt"][r], g["sym/points"][o][:g["sym/n_points"][o]],
                      g["sym/symmetries"][o][:g["sym/n_sym"][o]])
        take(res, "sym/", r)
    # the same two means on the short cloud (63 points), kept apart: fewer terms average less rounding away
    pred, gt, pts = g["short/TXO_pred"], g["short/TXO_gt"], g["cloud_small"][:g["short/adds_assign"].shape[1]]
    long_rows = dict(e)
    for r in range(len(pred)):
        take(add(pred[r], gt[r], pts), "short/add_", r)
        take(add_s(pred[r], gt[r], pts, assign=g["short/adds_assign"][r]), "short/adds_", r)
    e["norm_avg_short"], e["xyz_avg_short"] = e["norm_avg"], e["xyz_avg"]  # not below the long rows' figure
    e["norm_avg"], e["xyz_avg"] = long_rows["norm_avg"], long_rows["xyz_avg"]
    e["norm_max"] = max(e["norm_max"], long_rows["norm_max"])
    _CACHE["errors"] = e
    return e


def bounds(g) -> dict:
    """What the kernels are held to: MARGIN x the measured reference error, per quantity (``point`` is the issue's delta)."""
    b = {k: MARGIN * v for k, v in reference_errors(g).items()}
    # the means were measured over rows of at least `min_points` points (`norm_avg`, `xyz_avg`) and of `short_points`
    # (`*_short`): a mean over fewer terms averages less rounding away
    b["min_points"] = int(min(g["sym/n_points"].min(), len(g["cloud_small"])))
    b["short_points"] = int(g["short/adds_assign"].shape[1])
    return b


def mean_bounds(b, n_points) -> dict:
    """Bounds of ``norm_avg`` / ``xyz_avg`` for a row of ``n_points`` distinct points: the ones measured on rows of
    ``min_points`` and more; from ``short_points`` on the ones measured on the short cloud; below that -- the tests go down to
    a single point, whose 'mean' IS one per-point distance -- the measured per-point bound."""
    if n_points >= b["min_points"]:
        return {"norm_avg": b["norm_avg"], "xyz_avg": b["xyz_avg"]}
    if n_points >= b["short_points"]:
        return {"norm_avg": b["norm_avg_short"], "xyz_avg": b["xyz_avg_short"]}
    return {"norm_avg": b["point"], "xyz_avg": b["point"]}
