"""The float64 reference of the depth refiner (tests/icp_ref.py) without a GPU: it agrees with the float32 restatement of the same
definition (oracle/icp.py) to that restatement's round-off, recovers a known motion, solves a well-conditioned system, and
the pixels whose decisions a float32 evaluation could make differently (the fragile ones, see icp_ref) are few.

Figures of these scenes (three shapes, threshold and mask variants), printed by the tests with ``-s``:

* condition number of the regularised 6x6 system at the first iteration: 3.4e3 .. 6.1e3 (rotations in radians against
  translations in metres at 0.8 m from the camera; float64 loses 4 of its 16 digits, the float32 sums 4 of their 7).
* fragile share of the source set: under 1 % in every accumulate case (expected: two axes x a 2e-3 px window = 0.4 %); the
  condition is 2 %.  A full run is freed of them by removing the fragile pixels of every pass, again and again (removing a
  source pixel moves the centroid start, hence every later increment): at 37x53 these seeds have none, at 64x64 and 120x160
  the removal ends after up to 13 rounds and 8 % of the source set, over the condition, so full runs are compared at 37x53.
* float32 evaluation of a whole run (icp_yardstick.refine_f32) against the float64 run at 37x53: 5.6e-7 on a rotation entry, 7.8e-8 m
  on a translation entry, 2.9e-6 of the residual (icp_yardstick.MEASURED_F32_RUN).
* float32 evaluation of the per-pixel terms, summed in the kernels' order, against the float64 sums, relative to sum|term|:
  9.1e-7 for the sums of points and of J J', 1.17e-5 for J r and r^2 (icp_yardstick.MEASURED_F32_ERROR).
"""

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import icp_ref as R  # noqa: E402
import icp_yardstick as Y  # noqa: E402

from oracle import icp as OI  # noqa: E402


def _angle_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1.0) / 2.0, -1.0, 1.0))))


@pytest.mark.parametrize("shape", R.SHAPES)
def test_target_table_agrees_with_the_float32_restatement(shape):
    """Same zero pattern; points to 2 ulp of float32 (two rounded operations); normals to the cancellation of the restatement's
    float32 differences of neighbouring points (1e-4 rad); the holes of the scene are where they should be."""
    images, _, tgt = R.batch(*shape)
    for b, im in enumerate(images):
        X, N = OI.target_table(im["measured"], im["K"])
        valid = im["measured"] > 0
        assert 0.15 < 1.0 - valid.mean() < 0.30
        assert ((tgt[b] != 0).any(-1) == valid).all() and ((tgt[b, ..., 3:] != 0).any(-1) == valid).all()
        assert ((N != 0).any(-1) == valid).all() and ((X != 0).any(-1) == valid).all()
        assert (np.abs(X - tgt[b, ..., :3]) <= 2 * np.spacing(np.abs(X).astype(np.float32))).all()
        cosang = np.clip((N * tgt[b, ..., 3:]).sum(-1)[valid], -1, 1)
        cross = np.linalg.norm(np.cross(N[valid].astype(np.float64), tgt[b, ..., 3:][valid]), axis=-1)
        assert (cosang > 0).all() and cross.max() < 1e-4, cross.max()
        np.testing.assert_allclose(np.linalg.norm(tgt[b, ..., 3:][valid], axis=-1), 1.0, atol=1e-14)
        # the fronto-parallel patch, the empty block and the lone pixel in its hole
        inner = im["patch_interior"] & valid
        assert inner.sum() >= 30 and (tgt[b][inner][:, 3:] == [0.0, 0.0, 1.0]).all()
        v0, u0 = im["empty_block"]
        assert not valid[v0:v0 + 7, u0:u0 + 7].any() and not tgt[b, v0:v0 + 7, u0:u0 + 7].any()
        v1, u1 = im["lone_pixel"]
        assert valid[v1, u1] and valid[v1 - 3:v1 + 4, u1 - 3:u1 + 4].sum() == 1 and (tgt[b, v1, u1, 3:] == [0.0, 0.0, 1.0]).all()


def test_normal_yardstick_of_the_gpu_table_test():
    """The three images per shape of the GPU table test (seeds 0..2, focal lengths up to 1.12x): the float32 restatement's normals
    are within icp_yardstick.NORMAL_ANGLE_F32 of the reference's."""
    worst = 0.0
    for H, W in R.SHAPES:
        for b in range(3):
            im = R.make_image(H, W, seed=b, scale=1.0 + 0.06 * b)
            ref, (_, N) = R.target_table(im["measured"], im["K"]), OI.target_table(im["measured"], im["K"])
            valid = im["measured"] > 0
            g, r = N[valid].astype(np.float64), ref[..., 3:][valid]
            worst = max(worst, float(np.arctan2(np.linalg.norm(np.cross(g, r), axis=-1), (g * r).sum(-1)).max()))
    print(f"normals: float32 restatement against float64, largest angle {worst:.3g} rad")
    assert worst <= Y.NORMAL_ANGLE_F32 * 1.0001


def test_pixel_table_truncates_toward_zero():
    """Left of a fractional principal point ``int16(u - cx)`` is not ``floor(u - cx)``: the scenes do exercise the difference."""
    for H, W in R.SHAPES:
        K = R.camera(H, W)
        u = np.arange(W, dtype=np.float32) - K[0, 2]
        assert (R.ipix(W, K[0, 2]) == np.trunc(u)).all() and (np.trunc(u) != np.floor(u)).sum() >= W // 2 - 1
        assert R.ipix(W, K[0, 2])[W // 2 - 1] == R.ipix(W, K[0, 2])[W // 2] == 0


@pytest.mark.parametrize("masked", [False, True], ids=["threshold", "mask"])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_accumulate_cases(shape, masked):
    """Few fragile pixels; every outcome of a source pixel occurs where it is meant to; the float32 evaluation of the same
    terms selects the same pixels once the fragile ones are gone, and its error against the float64 sums is what the GPU test's
    bound is derived from (printed)."""
    H, W = shape
    worst = {"geometry": 0.0, "residual": 0.0}
    for case in R.accumulate_cases(H, W, masked):
        assert case["fragile_share"] <= R.MAX_FRAGILE_SHARE, (case["name"], case["fragile_share"])
        images, preds, tgt = R.batch(H, W)
        for i, b in enumerate(R.IM_IDS):
            ref = case["refs"][i][1]
            assert not ref["fragile"].any()
            states = np.bincount(ref["state"], minlength=5) / len(ref["state"])
            if case["name"] == "far":
                assert states[0] > 0.04 and states[1] > 0.15 and states[2] > 0.3 and states[3] > 0.05, states
            else:
                assert states[0] > 0.7 and states[1] == 0 and states[3] > 0.05, states
            im = images[b]
            mask = case["masks"][b] if masked else None
            for mode in (0, 1):
                r64 = case["refs"][i][mode]
                r32 = R.accumulate_terms(mode, case["T"], case["rendered"][i], im["measured"], mask, im["K"], tgt[b].astype(np.float32),
                                         case["tolerance"], R.DELTA_THRESH, dtype=np.float32)
                assert np.array_equal(r32["pixels"], r64["pixels"])
                s32 = Y.kernel_order_sum(r32["terms"], r32["pixels"], H * W)
                assert s32[27] == r64["sums"][27] == len(r64["pixels"])
                nz = r64["abs_sums"] > 0
                assert (s32[~nz] == 0).all()
                ratio = np.where(nz, np.abs(s32 - r64["sums"]) / np.where(nz, r64["abs_sums"], 1.0), 0.0)
                for group, idx in Y.ACC_GROUPS.items():
                    worst[group] = max(worst[group], float(ratio[idx].max()))
    print(f"accumulate {shape} {'mask' if masked else 'threshold'}: float32 |sum - ref| / sum|term| <= {worst}")
    # the yardstick itself: sums of points and of J J' lose a few ulp; r = n.(q - p') is a difference of two points 0.8 m away that
    # lie millimetres apart, so J r and r^2 carry the float32 spacing of 0.8 m (6e-8) over |r| of 1e-3 .. 1e-2
    assert worst["residual"] <= Y.MEASURED_F32_ERROR["residual"] * 1.0001
    assert worst["geometry"] <= Y.MEASURED_F32_ERROR["geometry"] * 1.0001


@pytest.mark.parametrize("masked", [False, True], ids=["threshold", "mask"])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_refine_agrees_with_the_float32_restatement(shape, masked):
    """One iteration (a pixel associated differently is amplified by every further one: 1e-4 on a rotation entry after
    three, on the 120x160 mask scene): same decision, poses and residual within the float32 restatement's round-off -- which here
    includes the odd fragile pixel it associates differently (the scenes are as generated) --; the 6x6 system is well conditioned
    (3.4e3 .. 6.1e3); residual <= tolerance."""
    H, W = shape
    images, preds, tgt = R.batch(H, W)
    iters = 1
    dR = dt = dres = cond = 0.0
    for i, b in enumerate(R.IM_IDS):
        im, mask = images[b], preds[i]["mask"] if masked else None
        ref = R.refine(preds[i]["rendered"], im["measured"], mask, im["K"], preds[i]["TCO"], iters, 50, 0.05, R.DELTA_THRESH, tgt=tgt[b])
        assert ref["retval"] == 0 and min(ref["n_start"], ref["n_inliers"]) > 150 and 0 < ref["residual"] <= 0.05
        A, _ = R.normal_equations(ref["passes"][0]["sums"])
        cond = max(cond, float(np.linalg.cond(A)))
        pose, ret, res = OI.icp_refine(preds[i]["rendered"], im["measured"], im["K"], preds[i]["TCO"], mask=mask, n_iterations=iters,
                                       n_min_points=50, tolerance=0.05, depth_delta_thresh=R.DELTA_THRESH)
        assert ret == 0
        dR = max(dR, float(np.abs(pose[:3, :3] - ref["pose"][:3, :3]).max()))
        dt = max(dt, float(np.abs(pose[:3, 3] - ref["pose"][:3, 3]).max()))
        dres = max(dres, abs(res - ref["residual"]) / ref["residual"])
    print(f"refine {shape} {'mask' if masked else 'threshold'} {iters} it: |dR| {dR:.3g} |dt| {dt:.3g} m residual rel {dres:.3g}; cond {cond:.3g}")
    assert dR < 2e-5 and dt < 5e-6 and dres < 5e-3 and 1e3 < cond < 1e4  # dres: one re-associated pixel among a few hundred inliers


def test_full_runs_without_fragile_pixels():
    """Section c's scenes (37x53, 1 and 2 iterations, threshold and mask): removing the pixels that are fragile in any pass of the
    float64 run ends, with at most 2 % of the source set gone (on these seeds: none; at 64x64 and 120x160 it ends too, but takes
    up to 8 %, so the runs are compared at 37x53 only); thresholds stay well away from the counts; the float32 evaluation of the
    whole run (icp_yardstick.refine_f32) selects the same inliers, and its distance from the float64 run is the yardstick of the GPU test."""
    H, W = 37, 53
    images, preds, tgt = R.batch(H, W)
    worst = {"rotation": 0.0, "translation": 0.0, "residual": 0.0}
    for masked in (False, True):
        for iters in (1, 2):
            for i, (b, case) in enumerate(zip(R.IM_IDS, R.run_cases(H, W, masked, iters))):
                ref, im = case["ref"], images[b]
                assert case["fragile_share"] <= R.MAX_FRAGILE_SHARE and not ref["fragile"].any()
                assert ref["retval"] == 0 and min(ref["n_start"], ref["n_inliers"]) >= 250 and 0 < ref["residual"] <= 0.005  # against 50 and 0.05
                # the table as float32 evaluates it (oracle/icp.py), and the float64 one rounded: the worst of both counts
                for table in (np.concatenate(OI.target_table(im["measured"], im["K"]), -1), tgt[b]):
                    pose, n_inl, res = Y.refine_f32(case["rendered"], im["measured"], case["mask"], im["K"], preds[i]["TCO"], iters, 0.05, R.DELTA_THRESH, table)
                    assert n_inl == ref["n_inliers"]
                    worst["rotation"] = max(worst["rotation"], float(np.abs(pose[:3, :3] - ref["pose"][:3, :3]).max()))
                    worst["translation"] = max(worst["translation"], float(np.abs(pose[:3, 3] - ref["pose"][:3, 3]).max()))
                    worst["residual"] = max(worst["residual"], abs(res - ref["residual"]) / ref["residual"])
    print(f"full runs 37x53: float32 evaluation against float64 {worst}")
    for key, value in worst.items():
        assert value <= Y.MEASURED_F32_RUN[key] * 1.0001, (key, value)


def test_large_runs_without_fragile_pixels():
    """The large call of the workspace test (120x160, 5 predictions over 3 images, 2 iterations).  Freeing its runs of fragile
    pixels ends, but takes 1.7 % .. 8.0 % of a source set, over the 2 % of the stage tests (every removal moves the increment and
    makes other pixels fragile: up to 28 rounds); the condition here is 8 %, and thousands of inliers are left.  The float32
    evaluation of these runs selects the same inliers; its distance from the float64 runs is the GPU test's yardstick."""
    H, W = R.LARGE_SHAPE
    images, preds, tgt = R.batch(H, W, R.LARGE_IM_IDS, R.LARGE_N_IMAGES)
    worst = {"rotation": 0.0, "translation": 0.0, "residual": 0.0}
    shares = []
    for i, (b, case) in enumerate(zip(R.LARGE_IM_IDS, R.run_cases(H, W, False, 2, R.LARGE_IM_IDS, R.LARGE_N_IMAGES))):
        ref, im = case["ref"], images[b]
        shares.append(case["fragile_share"])
        assert case["fragile_share"] <= R.MAX_FRAGILE_SHARE_LARGE_RUN and not ref["fragile"].any()
        assert ref["retval"] == 0 and min(ref["n_start"], ref["n_inliers"]) >= 2000 and 0 < ref["residual"] <= 0.005
        for table in (np.concatenate(OI.target_table(im["measured"], im["K"]), -1), tgt[b]):
            pose, n_inl, res = Y.refine_f32(case["rendered"], im["measured"], None, im["K"], preds[i]["TCO"], 2, 0.05, R.DELTA_THRESH, table)
            assert n_inl == ref["n_inliers"]
            worst["rotation"] = max(worst["rotation"], float(np.abs(pose[:3, :3] - ref["pose"][:3, :3]).max()))
            worst["translation"] = max(worst["translation"], float(np.abs(pose[:3, 3] - ref["pose"][:3, 3]).max()))
            worst["residual"] = max(worst["residual"], abs(res - ref["residual"]) / ref["residual"])
    print(f"large runs 120x160: fragile shares {np.round(shares, 4)}; float32 evaluation against float64 {worst}")
    for key, value in worst.items():
        assert value <= Y.MEASURED_F32_RUN_LARGE[key] * 1.0001, (key, value)


def test_recovers_the_known_motion():
    """At 240x320 without background and holes in the way the refinement moves the pose toward the truth: from 0.52 degrees and
    1.6 mm off (the centroid start) to under a third of either in 10 iterations.  It does not reach zero; the cause of the rest
    (about 0.17 degrees) has not been established and nothing here depends on it."""
    H, W = 240, 320
    K = R.camera(H, W)
    image = dict(K=K, measured=R.ellipsoid_depth(H, W, K))
    pr = R.make_prediction(image, 0)
    ref = R.refine(pr["rendered"], image["measured"], None, K, pr["TCO"], 10, 1000, 0.05, R.DELTA_THRESH)
    assert ref["retval"] == 0
    M, c = pr["motion"], R.ELLIPSOID["center"]
    err = [(_angle_deg(T[:, :3], M[:, :3]), float(np.linalg.norm((T[:, :3] - M[:, :3]) @ c + T[:, 3] - M[:, 3]))) for T in ref["T"]]
    print("recovery: (degrees, metres at the centre) start", err[0], "end", err[-1])
    assert err[0][0] > 0.5 and err[0][1] > 1.5e-3
    assert err[-1][0] < err[0][0] / 3 and err[-1][1] < err[0][1] / 3
    # the refined pose places the model where the measured surface is
    got = ref["pose"]
    assert np.abs(got[:3, 3] - c).max() < err[0][1] / 3


def test_rejections_and_the_degenerate_plane():
    """``refine`` gives up where the definition says so, with the input pose and residual -1, and the restatement decides alike.
    A single fronto-parallel plane leaves rotation about z and translation in x, y unconstrained: the regularised system is
    still positive definite, the increment is zero in those directions and the prediction is accepted."""
    H, W = 37, 53
    images, preds, tgt = R.batch(H, W)
    im, pr = images[0], preds[1]
    args = (im["measured"], None, im["K"], pr["TCO"])
    few = np.zeros_like(pr["rendered"])
    vs, us = np.nonzero((pr["rendered"] > 0) & (im["measured"] > 0.2) & (np.abs(im["measured"] - pr["rendered"]) < 0.05))
    few[vs[:5], us[:5]] = pr["rendered"][vs[:5], us[:5]]
    for rendered, n_min, reason in ((pr["rendered"], 5000, "start"), (few, 3, "few")):
        ref = R.refine(rendered, *args, 2, n_min, 0.05, R.DELTA_THRESH)
        assert (ref["retval"], ref["residual"], ref["reason"]) == (-1, -1.0, reason) and np.array_equal(ref["pose"], pr["TCO"])
        pose, ret, res = OI.icp_refine(rendered, im["measured"], im["K"], pr["TCO"], n_iterations=2, n_min_points=n_min)
        assert (ret, res) == (-1, -1.0) and np.array_equal(pose, pr["TCO"])
    plane = R.plane_case(H, W)
    ref = R.refine(plane["rendered"], plane["measured"], None, plane["K"], plane["TCO"], 2, 50, 0.05, R.DELTA_THRESH)
    x = R.solve_increment(ref["passes"][0]["sums"])
    assert ref["retval"] == 0 and ref["n_inliers"] > 500 and (x[2:5] == 0).all() and (np.abs(x[:2]) > 1e-3).all(), x
    A, _ = R.normal_equations(ref["passes"][0]["sums"])
    assert np.linalg.cond(A) > 1e8
    # the float32 restatement on the plane: the yardstick of the GPU test of this case
    pose, ret, res = OI.icp_refine(plane["rendered"], plane["measured"], plane["K"], plane["TCO"], n_iterations=2, n_min_points=50,
                                   tolerance=0.05, depth_delta_thresh=R.DELTA_THRESH)
    d_pose, d_res = float(np.abs(pose - ref["pose"]).max()), abs(res - ref["residual"]) / ref["residual"]
    print(f"plane: float32 restatement against float64: pose {d_pose:.3g}, residual rel {d_res:.3g}")
    assert ret == 0 and d_pose <= Y.PLANE_F32["pose"] * 1.0001 and d_res <= Y.PLANE_F32["residual"] * 1.0001
