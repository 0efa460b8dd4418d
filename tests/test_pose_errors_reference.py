"""The pose-error tolerances are MEASURED here: the reference's own float32 run (tests/golden/g12_pose_errors.npz) against the
float64 restatement (tests/pose_errors_ref.py), per quantity.  The kernels get 4 x these deviations (tests/test_gpu_pose_errors.py,
table in DESIGN.md section 2).  The mutation checks show that the bounds bite: each wrong reading of a definition misses them
by 10 x or more."""

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pose_errors_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def g12(golden_dir):
    return np.load(golden_dir / "g12_pose_errors.npz")


def test_measured_reference_errors(g12):
    """The measurement itself, printed; sanity limits only: a float32 evaluation of centimetre errors half a metre to 1.2 m from
    the camera cannot be better than a fraction of an ulp of the coordinates (6e-8 at 1 m) nor worse than a few hundred ulps."""
    e = R.reference_errors(g12)
    print("reference float32 deviation from float64:", {k: f"{v:.3e}" for k, v in e.items()})
    print("kernel bounds (x %g):" % R.MARGIN, {k: f"{v:.3e}" for k, v in R.bounds(g12).items()})
    for k in ("norm_avg", "xyz_avg", "norm_max", "point"):
        assert 1e-10 < e[k] < 2e-5, (k, e[k])
    assert 1e-7 < e["pixel"] < 1e-2, e["pixel"]  # pixels: coordinates of a few hundred, ulp 3e-5


def test_recorded_symmetry_choices(g12):
    for r, o in enumerate(g12["sym/obj_id"]):
        res = R.add_sym(g12["sym/TXO_pred"][r], g12["sym/TXO_gt"][r], g12["sym/points"][o][:g12["sym/n_points"][o]],
                        g12["sym/symmetries"][o][:g12["sym/n_sym"][o]])
        assert res["sym_id"] == g12["sym/sym_id"][r], r
    assert set(g12["sym/sym_id"].tolist()) > {0}  # a symmetry other than the identity is exercised


def test_reference_neighbours_are_nearest_within_delta(g12):
    """Check 1 of the nearest-neighbour choice, applied to the reference's own assignment: the float64 distance to the neighbour
    it chose is at most the float64 minimum plus delta, on every stored row, no point excluded."""
    delta = R.bounds(g12)["point"]
    pred, gt, pts = R.golden_rows(g12, "small")
    flips = 0
    for r in range(len(pred)):
        assign64, best2 = R.nearest(pred[r], gt[r], pts)
        d = R.neighbour_distance(pred[r], gt[r], pts, g12["small/adds_assign"][r])
        assert (d <= np.sqrt(best2) + delta).all(), (r, (d - np.sqrt(best2)).max(), delta)
        flips += int((assign64 != g12["small/adds_assign"][r]).sum())
    print("choices of the reference's float32 run that differ from float64:", flips, "of", pred.shape[0] * len(pts))


def test_large_cloud_and_chamfer_within_bound_plus_delta(g12):
    """Rows without stored neighbours: the pure float64 ADD-S agrees with the reference within the bound plus delta (a flipped
    near-tie moves a point's distance by at most delta)."""
    b = R.bounds(g12)
    pred, gt, pts = R.golden_rows(g12, "large")
    for r in range(len(pred)):
        assert abs(R.add_s(pred[r], gt[r], pts)["norm_avg"] - g12["large/adds_norm_avg"][r]) <= b["norm_avg"] + b["point"], r
    pad = g12["sym/points"]
    for r, o in enumerate(g12["sym/obj_id"]):  # chamfer_dist(T1 = gt, T2 = pred) walks the padded table: T1's points look for T2's
        ref = R.add_s(g12["sym/TXO_pred"][r], g12["sym/TXO_gt"][r], pad[o])["norm_avg"]
        assert abs(ref - g12["sym/chamfer"][r]) <= b["norm_avg"] + b["point"], r


# ---- mutations: each wrong reading of a definition misses the bound by 10 x or more -----------------------------------------------
def _rows(g12):
    pred, gt, pts = R.golden_rows(g12, "small")
    return [(pred[r], gt[r], pts, r) for r in range(len(pred) - 1)]  # the last row has pred == gt: every reading gives 0


def test_mutation_nearest_neighbour_from_the_wrong_side(g12):
    """Predicted points looking for ground-truth points.  The two directions of a chamfer distance can have nearly equal MEANS
    (row 2 of G12: 4e-6 apart, 9 x the bound plus delta that a comparison with G12 allows), so THAT comparison is held to 10 x on
    the worst row only.  On EVERY row the mutant misses two bounds by 10 x and more: check 1 (read as 'neighbour of ground-truth
    point j', its choices are off by far more than 10 delta) and check 2 (its mean against the float64 mean over its own
    neighbours, read the same way, within the norm_avg bound)."""
    b = R.bounds(g12)
    miss = []
    for pred, gt, pts, r in _rows(g12):
        wrong = R.add_s(gt, pred, pts)
        miss.append(abs(wrong["norm_avg"] - g12["small/adds_norm_avg"][r]))
        _, best2 = R.nearest(pred, gt, pts)
        excess = R.neighbour_distance(pred, gt, pts, wrong["assign"]) - np.sqrt(best2)
        print(f"row {r}: mean off by {miss[-1]:.2e}, worst neighbour {excess.max():.2e} beyond the nearest")
        assert excess.max() >= 10 * b["point"], r
        own = R.add_s(pred, gt, pts, assign=wrong["assign"])["norm_avg"]
        assert abs(wrong["norm_avg"] - own) >= 10 * b["norm_avg"], (r, abs(wrong["norm_avg"] - own))
    assert max(miss) >= 10 * (b["norm_avg"] + b["point"])


def test_mutation_mean_of_squares(g12):
    b = R.bounds(g12)
    for pred, gt, pts, r in _rows(g12):
        d = R.add(pred, gt, pts)["dists"]
        rms = np.sqrt((d * d).sum(-1).mean())
        assert abs(rms - g12["small/add_norm_avg"][r]) >= 10 * b["norm_avg"], r
        d = R.add_s(pred, gt, pts, assign=g12["small/adds_assign"][r])["dists"]
        rms = np.sqrt((d * d).sum(-1).mean())
        assert abs(rms - g12["small/adds_norm_avg"][r]) >= 10 * b["norm_avg"], r


def test_mutation_padding_counted_in_exact_mode(g12):
    from happypose_amd.mesh_store import pad_stack_points

    b = R.bounds(g12)
    padded = pad_stack_points([g12["cloud_small"], g12["cloud_large"]])[0]
    assert len(padded) > len(g12["cloud_small"])
    for pred, gt, pts, r in _rows(g12):
        wrong = R.add(pred, gt, padded)
        assert abs(wrong["norm_avg"] - g12["small/add_norm_avg"][r]) >= 10 * b["norm_avg"], r


def test_mutation_symmetry_on_the_wrong_side(g12):
    b = R.bounds(g12)
    checked = 0
    for r, o in enumerate(g12["sym/obj_id"]):
        n_sym = g12["sym/n_sym"][o]
        if g12["sym/sym_id"][r] == 0:  # where the identity wins, both readings agree
            continue
        syms, T_gt = g12["sym/symmetries"][o][:n_sym].astype(np.float64), g12["sym/TXO_gt"][r].astype(np.float64)
        conj = np.stack([np.linalg.inv(T_gt) @ S @ T_gt for S in syms])  # T_gt conj = S T_gt: the symmetry in the camera frame
        wrong = R.add_sym(g12["sym/TXO_pred"][r], T_gt, g12["sym/points"][o][:g12["sym/n_points"][o]], conj)
        assert abs(wrong["norm_avg"] - g12["sym/norm_avg"][r]) >= 10 * b["norm_avg"], r
        checked += 1
    assert checked >= 3
