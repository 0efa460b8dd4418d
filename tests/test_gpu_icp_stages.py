"""The depth refiner's kernels (csrc/icp.hip) stage by stage against the float64 reference of their definition (tests/icp_ref.py),
on analytic scenes at the smallest shapes that reach every path: 37x53 (idle lanes, blocks past the end), 64x64 (a multiple
of 64), 120x160 (a second trip of the strided loop); fractional principal points; 3 predictions over 2 images, unsorted.

Bounds (none comes from a kernel's output; the float32 figures are measured on the CPU by tests/test_icp_reference.py):

* table points: 2 ulp of float32 (x = i z / f is two correctly rounded operations).
* table normals: the float32 restatement (oracle/icp.py) is up to 7.2e-5 rad off the float64 normals on these scenes (its
  differences of neighbouring points cancel 3 digits; icp_yardstick.NORMAL_ANGLE_F32); the kernel gets 4x: 2.9e-4 rad.
* sums: |sum - ref| <= 4 x e x sum|term| per accumulator, e = 9.1e-7 for the sums of points and of J J', 1.17e-5 for J r and r^2
  (icp_yardstick.MEASURED_F32_ERROR: float32 terms added in the kernels' order against the float64 sums); counts are exact, which
  the removal of the fragile pixels (icp_ref) makes possible.
* full runs (37x53, where the removal of the fragile pixels of every pass stays under 2 % of the source set; 1 and 2 iterations):
  the float32 evaluation of the whole run (icp_yardstick.refine_f32) is up to 5.6e-7 off the float64 run on a rotation entry, 7.8e-8 m
  on a translation entry and 2.9e-6 of the residual (icp_yardstick.MEASURED_F32_RUN); the kernels get 4x: 2.2e-6, 3.1e-7 m, 1.2e-5.
* the large call of the workspace test (120x160, 5 predictions over 3 images, 2 iterations; the removal takes 1.7 % .. 8.0 % of a
  source set there, over the 2 % of the stage tests): the float32 evaluation is up to 9.4e-8, 7.4e-8 m and 6.5e-6 off
  (icp_yardstick.MEASURED_F32_RUN_LARGE); the kernels get 4x: 3.8e-7, 3.0e-7 m, 2.6e-5.
* the plane: oracle/icp.py is 3.4e-8 off on a pose entry and 1.9e-6 of the residual (icp_yardstick.PLANE_F32); the kernels get 4x.
  The remaining full runs (rejections, 70 predictions) are compared bit for bit with other calls of the same kernels.
"""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import icp_ref as R  # noqa: E402
import icp_yardstick as Y  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


# ---- the C entry points on NumPy inputs ------------------------------------------------------------------------------

def _dev(dev, a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)


def _target_table(dev, depth, K):
    from happypose_amd._ffi import check, lib, ptr, stream_ptr

    B, H, W = depth.shape
    d_depth, d_K = _dev(dev, depth, np.float32), _dev(dev, np.reshape(K, (B, 9)), np.float32)
    out = torch.full((B, H, W, 6), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_icp_target_table(B, H, W, ptr(d_depth), ptr(d_K), ptr(out), stream_ptr(dev)), "hp_icp_target_table")
    return out.cpu().numpy()


def _accumulate(dev, rendered, measured, masks, im_ids, K, tgt, T, mode, tolerance):
    """``hp_icp_accumulate``: the 64 partials of every prediction added in float64, as the update kernel adds them: ``[n, 32]``."""
    from happypose_amd._ffi import check, lib, ptr, stream_ptr

    n, H, W = rendered.shape
    B = measured.shape[0]
    assert min(im_ids) >= 0 and max(im_ids) < B and tgt.shape == (B, H, W, 6) and T.shape == (n, 3, 4) and K.shape == (n, 3, 3)
    bufs = [_dev(dev, rendered, np.float32), _dev(dev, measured, np.float32), None if masks is None else _dev(dev, masks, np.uint8),
            _dev(dev, im_ids, np.int32), _dev(dev, K.reshape(n, 9), np.float32), _dev(dev, tgt, np.float32), _dev(dev, T.reshape(n, 12), np.float32)]
    partial = torch.full((n, R.N_BLOCKS, R.N_ACC), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_icp_accumulate(n, B, H, W, *[ptr(b) for b in bufs], mode, tolerance, R.DELTA_THRESH, ptr(partial), stream_ptr(dev)),
              "hp_icp_accumulate")
    return partial.cpu().numpy().astype(np.float64).sum(1)


def _refine(dev, rendered, measured, masks, im_ids, K, TCO, n_iterations, n_min_points, tolerance):
    from happypose_amd._ffi import check, lib, ptr, stream_ptr

    n, H, W = rendered.shape
    B = measured.shape[0]
    im_ids_h = np.ascontiguousarray(im_ids, dtype=np.int32)
    bufs = [_dev(dev, rendered, np.float32), _dev(dev, measured, np.float32), None if masks is None else _dev(dev, masks, np.uint8),
            _dev(dev, im_ids_h, np.int32)]
    d_K, d_TCO = _dev(dev, np.reshape(K, (n, 9)), np.float32), _dev(dev, TCO, np.float32)
    out = torch.full((n, 4, 4), float("nan"), dtype=torch.float32, device=dev)
    retval = torch.full((n,), 7, dtype=torch.int32, device=dev)
    residual = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    import ctypes as C
    with torch.cuda.device(dev):
        check(lib().hp_icp_refine(n, B, H, W, *[ptr(b) for b in bufs], im_ids_h.ctypes.data_as(C.c_void_p), ptr(d_K), ptr(d_TCO),
                                  n_iterations, n_min_points, tolerance, R.DELTA_THRESH, ptr(out), ptr(retval), ptr(residual),
                                  stream_ptr(dev)), "hp_icp_refine")
    return out.cpu().numpy(), retval.cpu().numpy(), residual.cpu().numpy()


def _call(dev, images, preds, im_ids, which, masked=False, n_iterations=2, n_min_points=50, tolerance=0.05, image_ids=None):
    """``hp_icp_refine`` on the predictions ``which`` of a batch; ``image_ids`` renumbers the images (default: all of them)."""
    image_ids = list(range(len(images))) if image_ids is None else image_ids
    measured = np.stack([images[b]["measured"] for b in image_ids])
    ids = [image_ids.index(im_ids[i]) for i in which]
    masks = None
    if masked:  # one mask per image: the union of its predictions' boxes
        masks = np.stack([np.max([preds[i]["mask"] for i in range(len(preds)) if im_ids[i] == b] or [np.zeros_like(preds[0]["mask"])], 0)
                          for b in image_ids])
    return _refine(dev, np.stack([preds[i]["rendered"] for i in which]), measured, masks, ids,
                   np.stack([images[im_ids[i]]["K"] for i in which]), np.stack([preds[i]["TCO"] for i in which]), n_iterations, n_min_points,
                   tolerance)


def _same(a, b):
    return all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


def _pick(res, idx):
    return tuple(x[idx] for x in res)


# ---- f. the workspace -------------------------------------------------------------------------------------------------------
# The workspace belongs to the process and only grows.  Alone, this module's first test starts it empty and the large call regrows
# all three buffers; in the whole suite an earlier module has made a 480x640 call, so the table (7.4 MB against 1.4 MB here) is
# already large enough and only the per-prediction buffer (n 3 -> 5) and the per-image one (B 1 -> 3) regrow.

def test_workspace_regrowth(dev):
    """A small call (37x53, n = 1, B = 1), a large one (120x160, n = 5, B = 3, without its fragile pixels), the small one again:
    the small results are identical bit for bit; every prediction of the large call is within 4x the float32 evaluation's distance
    from the float64 run (icp_yardstick.MEASURED_F32_RUN_LARGE: 9.4e-8 on a rotation entry, 7.4e-8 m, 6.5e-6 of the residual; the
    removal takes up to 8.0 % of a source set here, see tests/test_icp_reference.py) and equals its own n = 1, B = 1 call bit for bit."""
    images, preds = R.make_batch(37, 53, [0], 1)
    small = lambda: _call(dev, images, preds, [0], [0])  # noqa: E731
    first = small()
    (H, W), im_ids = R.LARGE_SHAPE, list(R.LARGE_IM_IDS)
    big_images, big_preds, _ = R.batch(H, W, R.LARGE_IM_IDS, R.LARGE_N_IMAGES)
    cases = R.run_cases(H, W, False, 2, R.LARGE_IM_IDS, R.LARGE_N_IMAGES)
    big_preds = [dict(p, rendered=c["rendered"]) for p, c in zip(big_preds, cases)]
    big = _call(dev, big_images, big_preds, im_ids, range(5))
    again = small()
    assert first[1][0] == 0 and _same(first, again)
    assert (big[1] == 0).all() and (big[2] > 0).all() and (big[2] <= 0.05).all()
    for i, case in enumerate(cases):
        ref = case["ref"]
        dR, dt = np.abs(big[0][i, :3, :3] - ref["pose"][:3, :3]).max(), np.abs(big[0][i, :3, 3] - ref["pose"][:3, 3]).max()
        dres = abs(big[2][i] - ref["residual"]) / ref["residual"]
        print(f"large call prediction {i}: |dR| {dR:.3g} |dt| {dt:.3g} m residual rel {dres:.3g}")
        assert ref["retval"] == 0
        assert dR <= 4 * Y.MEASURED_F32_RUN_LARGE["rotation"] and dt <= 4 * Y.MEASURED_F32_RUN_LARGE["translation"], (i, dR, dt)
        assert dres <= 4 * Y.MEASURED_F32_RUN_LARGE["residual"], (i, dres)
        alone = _call(dev, big_images, big_preds, im_ids, [i], image_ids=[im_ids[i]])
        assert _same(_pick(big, [i]), alone), i


# ---- a. the target table -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.SHAPES)
def test_target_table(dev, shape):
    H, W = shape
    images = [R.make_image(H, W, seed=b, scale=1.0 + 0.06 * b) for b in range(3)]
    got = _target_table(dev, np.stack([im["measured"] for im in images]), np.stack([im["K"] for im in images]))
    for b, im in enumerate(images):
        ref = R.target_table(im["measured"], im["K"])
        valid = im["measured"] > 0
        # the pattern: per component for the points (x = i z / f is zero where i or z is), per vector for the normals (a component
        # that is exactly zero in float64, as on the background plane, is a rounding error of 1e-5 in float32, not a zero)
        assert np.isfinite(got[b]).all() and np.array_equal(got[b, ..., :3] != 0, ref[..., :3] != 0)
        assert np.array_equal((got[b, ..., 3:] != 0).any(-1), (ref[..., 3:] != 0).any(-1))
        assert np.array_equal((got[b, ..., 3:] != 0).any(-1), valid)
        assert np.array_equal(got[b, ..., 2], im["measured"] * valid)
        ulp = np.spacing(np.abs(ref[..., :3]).astype(np.float32))
        assert (np.abs(got[b, ..., :3] - ref[..., :3]) <= 2 * ulp).all()
        g, r = got[b, ..., 3:][valid].astype(np.float64), ref[..., 3:][valid]
        angle = np.arctan2(np.linalg.norm(np.cross(g, r), axis=-1), (g * r).sum(-1))
        print(f"target table {shape} image {b}: largest normal angle {angle.max():.3g} rad")
        assert angle.max() <= 4 * Y.NORMAL_ANGLE_F32
        np.testing.assert_allclose(np.linalg.norm(g, axis=-1), 1.0, atol=3e-7)
        inner = im["patch_interior"] & valid
        assert (got[b][inner][:, 3:] == [0.0, 0.0, 1.0]).all()
        v, u = im["lone_pixel"]
        assert (got[b, v, u, 3:] == [0.0, 0.0, 1.0]).all()


# ---- b. one accumulate pass ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True], ids=["threshold", "mask"])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_accumulate(dev, shape, masked):
    H, W = shape
    images, preds, tgt = R.batch(H, W)
    measured = np.stack([im["measured"] for im in images])
    K = np.stack([images[b]["K"] for b in R.IM_IDS])
    for case in R.accumulate_cases(H, W, masked):
        masks = case["masks"]  # one per image: what the reference was given too
        T = np.stack([case["T"]] * len(R.IM_IDS))
        for mode in (0, 1):
            got = _accumulate(dev, case["rendered"], measured, masks, list(R.IM_IDS), K, tgt.astype(np.float32), T, mode, case["tolerance"])
            for i in range(len(R.IM_IDS)):
                ref = case["refs"][i][mode]
                assert got[i, 27] == ref["sums"][27] == len(ref["pixels"]), (case["name"], mode, i, got[i, 27], ref["sums"][27])
                for group, idx in Y.ACC_GROUPS.items():
                    err = np.abs(got[i, idx] - ref["sums"][idx])
                    bound = 4 * Y.MEASURED_F32_ERROR[group] * ref["abs_sums"][idx]
                    worst = float((err / np.where(ref["abs_sums"][idx] > 0, ref["abs_sums"][idx], 1.0)).max())
                    print(f"accumulate {shape} {case['name']} mode {mode} prediction {i} {group}: |sum - ref| / sum|term| <= {worst:.3g}")
                    assert (err <= bound).all(), (case["name"], mode, i, group, err / np.maximum(bound, 1e-300))
                assert (got[i, 29:] == 0).all()


# ---- c. short full runs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_iterations", [1, 2])
@pytest.mark.parametrize("masked", [False, True], ids=["threshold", "mask"])
def test_short_runs_against_the_reference(dev, masked, n_iterations):
    """3 predictions over 2 images without their fragile pixels: retval exact (n_min_points = 50 against 250 and more inliers,
    tolerance 0.05 against residuals of 2 mm), poses and residual within 4x the float32 evaluation's distance from the reference."""
    H, W = 37, 53
    images, preds, _ = R.batch(H, W)
    cases = R.run_cases(H, W, masked, n_iterations)
    masks = R.image_masks(preds) if masked else None
    pose, retval, residual = _refine(dev, np.stack([c["rendered"] for c in cases]), np.stack([im["measured"] for im in images]), masks,
                                     list(R.IM_IDS), np.stack([images[b]["K"] for b in R.IM_IDS]), np.stack([p["TCO"] for p in preds]),
                                     n_iterations, 50, 0.05)
    for i, case in enumerate(cases):
        ref = case["ref"]
        dR, dt = np.abs(pose[i, :3, :3] - ref["pose"][:3, :3]).max(), np.abs(pose[i, :3, 3] - ref["pose"][:3, 3]).max()
        dres = abs(residual[i] - ref["residual"]) / ref["residual"]
        print(f"run {'mask' if masked else 'threshold'} {n_iterations} it prediction {i}: |dR| {dR:.3g} |dt| {dt:.3g} m residual rel {dres:.3g}")
        assert retval[i] == ref["retval"] == 0 and 0 < residual[i] <= 0.05
        assert (pose[i, 3] == [0, 0, 0, 1]).all()
        assert dR <= 4 * Y.MEASURED_F32_RUN["rotation"] and dt <= 4 * Y.MEASURED_F32_RUN["translation"]
        assert dres <= 4 * Y.MEASURED_F32_RUN["residual"]


# ---- d. rejections -------------------------------------------------------------------------------------------------------

def test_rejections_leave_the_pose_and_the_neighbours_alone(dev):
    """Every rejected prediction: input pose bit for bit, retval -1, residual -1; its accepted neighbours: the results of the call
    without it, bit for bit, and residual <= tolerance.  An image without a prediction changes nothing either."""
    H, W = 37, 53
    im_ids = [2, 0, 2]  # image 1 has no prediction
    images, preds = R.make_batch(H, W, im_ids, 3)
    full = _call(dev, images, preds, im_ids, range(3))
    assert (full[1] == 0).all() and (full[2] > 0).all() and (full[2] <= 0.05).all()
    for i in range(3):
        assert _same(_pick(full, [i]), _call(dev, images, preds, im_ids, [i], image_ids=[im_ids[i]])), i
    vs, us = np.nonzero((preds[1]["rendered"] > 0) & (images[0]["measured"] > 0.2) & (np.abs(images[0]["measured"] - preds[1]["rendered"]) < 0.05))
    few = np.zeros_like(preds[1]["rendered"])
    few[vs[:5], us[:5]] = preds[1]["rendered"][vs[:5], us[:5]]
    starved = R.starved_prediction(images[0], 1)
    half = preds[1]["rendered"].copy()
    half[H // 2:] = 0
    for name, rendered, n_min, tol, reason in (("start set", half, 250, 0.05, "start"), ("fewer than 6", few, 3, 0.05, "few"),
                                               ("inliers", starved["rendered"], 150, 0.02, "inliers")):
        ref = R.refine(rendered, images[0]["measured"], None, images[0]["K"], preds[1]["TCO"], 2, n_min, tol, R.DELTA_THRESH)
        assert ref["reason"] == reason and (ref["n_start"] <= 0.7 * n_min if reason == "start" else ref["n_start"] >= 1.5 * n_min), (name, ref["reason"], ref["n_start"], ref["n_inliers"])
        assert reason != "inliers" or 6 <= ref["n_inliers"] <= 0.6 * n_min
        mixed = [preds[0], dict(preds[1], rendered=rendered), preds[2]]
        got = _call(dev, images, mixed, im_ids, range(3), n_min_points=n_min, tolerance=tol)
        without = _call(dev, images, mixed, im_ids, [0, 2], n_min_points=n_min, tolerance=tol)
        assert got[1].tolist() == [0, -1, 0] and got[2][1] == -1.0, (name, got[1], got[2])
        assert np.array_equal(got[0][1].view(np.uint32), preds[1]["TCO"].view(np.uint32)), name
        assert _same(_pick(got, [0, 2]), without), name
        assert (got[2][[0, 2]] > 0).all() and (got[2][[0, 2]] <= tol).all()


def test_degenerate_plane_is_solved(dev):
    """One fronto-parallel plane leaves rotation about z and translation in x, y unconstrained.  The definition adds
    1e-9 trace + 1e-12 to the diagonal, so the factorisation succeeds, the increment is zero in those directions and the
    prediction is ACCEPTED: retval 0 and the float64 reference's pose."""
    H, W = 37, 53
    pl = R.plane_case(H, W)
    ref = R.refine(pl["rendered"], pl["measured"], None, pl["K"], pl["TCO"], 2, 50, 0.05, R.DELTA_THRESH)
    assert ref["retval"] == 0
    pose, retval, residual = _refine(dev, pl["rendered"][None], pl["measured"][None], None, [0], pl["K"][None], pl["TCO"][None], 2, 50, 0.05)
    assert retval[0] == 0 and 0 <= residual[0] <= 0.05
    # every target has the same depth and normal, so which pixel a source point lands on changes neither r nor J: the run needs
    # no removal of fragile pixels.  oracle/icp.py (float32) is 3.4e-8 off the reference on this scene and 1.9e-6 of the residual
    # (icp_yardstick.PLANE_F32, asserted by tests/test_icp_reference.py); the kernels get 4x
    np.testing.assert_allclose(pose[0], ref["pose"], rtol=0, atol=4 * Y.PLANE_F32["pose"])
    assert abs(residual[0] - ref["residual"]) <= 4 * Y.PLANE_F32["residual"] * ref["residual"]


# ---- e. more predictions than one block of the update and finalize kernels holds ------------------------------------------

def test_seventy_predictions_equal_their_single_calls(dev):
    H, W = 37, 53
    im_ids = [i % 2 for i in range(70)]
    images, preds = R.make_batch(H, W, im_ids, 2)
    full = _call(dev, images, preds, im_ids, range(70))
    assert (full[1] == 0).all() and (full[2] <= 0.05).all()
    assert len({full[0][i].tobytes() for i in range(70)}) == 70
    for i in range(70):
        assert _same(_pick(full, [i]), _call(dev, images, preds, im_ids, [i], image_ids=[im_ids[i]])), i
