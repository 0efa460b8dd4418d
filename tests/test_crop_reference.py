"""CPU tests of the crop reference (tests/crop_ref.py), of the case table it shares with tests/test_gpu_crop_paths.py, and of the
float32 yardstick (tests/crop_yardstick.py).

Measured here and written into crop_yardstick.MEASURED_F32_ERROR (worst over the table, both orders of summation, relative to the
reference on |image|): colour 3.04e-7, depth 2.72e-7 / 3.19e-7 / 1.46e-7 / 2.07e-7 after modes 0-3, interpolated validity mask
1.2e-7 absolute.  The GPU tests allow the kernels 4x these figures and leave out depth pixels whose float64 mask lies within
4 x 1.2e-7 of 0.99; no case of the table has a single such pixel (asserted below: at most 0.5 %)."""

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import crop_ref as R  # noqa: E402
import crop_yardstick as Y  # noqa: E402

F = np.float32


def _one(img, box, out_size, g, im_id=0):
    return R.roi_align_ref(img, np.array([box], F), [im_id], out_size, g)[0]


def test_constant_image():
    img = np.full((2, 3, 37, 53), 0.625, F)
    out = _one(img, (3.3, 2.2, 48.9, 33.1), (24, 32), 4, 1)  # every sample inside the frame
    assert np.abs(out - 0.625).max() <= 2e-16
    # half outside: a pixel keeps the share of its samples that are valid
    out = _one(img, (-20, 2.2, 20, 33.1), (24, 32), 4)
    vx = R.axis_samples(F(-20), F(40) / F(32), 32, 53, 4)[0].mean(1)
    assert np.abs(out[0] - 0.625 * vx[None, :]).max() <= 2e-16 and 0 in vx and 1 in vx


@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_affine_ramp_is_exact(g):
    H, W = 37, 53
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = (0.25 * xx - 0.5 * yy + 3.0)[None, None]  # exact in float64 and float32
    box, out_size = (4.7, 3.1, 44.3, 30.9), (24, 32)
    out = _one(img, box, out_size, g)[0]
    x1, y1, bw, bh = R.box_bins(box, out_size)
    # the float32 sample coordinates of the definition, averaged in float64: the value of the ramp at the mean sample
    ys = ((y1 + np.arange(24, dtype=F)[:, None] * bh) + ((np.arange(g, dtype=F) + F(0.5)) * bh) / F(g)).astype(np.float64)
    xs = ((x1 + np.arange(32, dtype=F)[:, None] * bw) + ((np.arange(g, dtype=F) + F(0.5)) * bw) / F(g)).astype(np.float64)
    assert ys.min() >= 0 and ys.max() <= H - 1 and xs.min() >= 0 and xs.max() <= W - 1
    want = 0.25 * xs.mean(1)[None, :] - 0.5 * ys.mean(1)[:, None] + 3.0
    assert np.abs(out - want).max() <= 1e-13


def test_identity_box():
    img = R.make_frames("A")
    out = R.roi_align_ref(img, np.array([[0, 0, 53, 37]] * 2, F), [0, 1], (37, 53), 1)
    # aligned=False, g = 1: the sample of pixel p sits at p + 0.5, half-way to p + 1, so the box of the frame gives the mean of
    # the four neighbours; the same box moved by half a pixel puts the samples on the pixels and returns the frame itself
    out0 = R.roi_align_ref(img, np.array([[-0.5, -0.5, 52.5, 36.5]] * 2, F), [0, 1], (37, 53), 1)
    assert np.array_equal(out0, img.astype(np.float64))
    img = img.astype(np.float64)
    want = 0.25 * (img[:, :, :-1, :-1] + img[:, :, 1:, :-1] + img[:, :, :-1, 1:] + img[:, :, 1:, 1:])
    assert np.abs(out[:, :, :-1, :-1] - want).max() <= 1e-15


def test_boundary_rules_at_hand_placed_samples():
    size = 8
    img = np.arange(1.0, size + 1)[None, None, None, :] * np.ones((1, 1, 4, 1))  # value x + 1 at column x, 4 rows
    up, dn = np.nextafter(F(1), F(2)), np.nextafter(F(1), F(0))

    def at(x):  # one output column, g = 1, bin 1: the single sample sits at x1 + 0.5 = x
        x1 = F(x) - F(0.5)
        assert x1 + F(0.5) == F(x)
        return R.roi_align_ref(img, np.array([[x1, 0.5, x1 + F(1), 1.5]], F), [0], (1, 1), 1)[0, 0, 0, 0]

    assert at(-1.0) == 1.0                      # exactly -1: kept, clamped to 0
    assert at(F(-1.0) * up) == 0.0              # just below -1: dropped
    assert at(-0.5) == 1.0 and at(0.0) == 1.0   # (-1, 0]: clamped to 0
    assert at(0.25) == 1.25
    assert at(F(size)) == size                  # exactly size: kept, collapsed onto size - 1
    assert at(F(size) * up) == 0.0              # just above: dropped
    assert at(size - 1) == size and at(size - 0.5) == size and at(F(size) * dn) == size  # [size-1, size]: the last pixel
    assert at(size - 1.25) == size - 0.25
    v, lo, hi, l = R.axis_samples(F(-1.25), F(2), 2, 64, 4)  # the first samples of the case edge_low
    assert v[0].tolist() == [True] * 4 and lo[0].tolist() == [0, 0, 0, 0] and l[0].tolist() == [0, 0, 0, 0.5]
    v, lo, hi, l = R.axis_samples(F(0.75), F(2), 24, 48, 4)  # the last row of the case edge_high: 47, 47.5, 48, 48.5
    assert v[-1].tolist() == [True, True, True, False] and lo[-1].tolist() == hi[-1].tolist() == [47] * 4 and not l[-1].any()
    for start, size in ((41, 64), (9, 48)):  # the last samples of the case edge_high_slow: the fourth sits on size itself and is kept
        n = 3 if size == 64 else 5
        v, lo, hi, l = R.axis_samples(F(start), F(8), n, size, 4)
        assert v[-1].all() and lo[-1].tolist() == [size - 6, size - 4, size - 2, size - 1] and hi[-1][-1] == size - 1 and not l[-1].any()


def test_agrees_with_the_c_oracle():
    from oracle import native

    img = R.make_frames("B")
    out_size = (24, 32)
    for C in (3, 4):
        im = np.ascontiguousarray(img[:, :C])
        got = native.crop_images(im, R.ORACLE_BOXES, R.ORACLE_IDS, out_size)
        ref, mask = R.crop_ref(im, R.ORACLE_BOXES, R.ORACLE_IDS, out_size, 4)
        S = np.maximum(R.roi_align_ref(np.abs(im), R.ORACLE_BOXES, R.ORACLE_IDS, out_size, 4), Y.SCALE_FLOOR)
        err = np.abs(got - ref) / S
        if C == 4:
            keep = np.abs(mask - R.VALID_THRESHOLD) > Y.band_of_mask()
            assert keep.mean() >= 0.995
            assert (err[:, 3][keep] <= 4 * Y.MEASURED_F32_ERROR["depth0"]).all(), err[:, 3][keep].max()
        assert (err[:, :3] <= 4 * Y.MEASURED_F32_ERROR["colour"]).all(), err[:, :3].max()
        assert np.abs(got).max() > 0.5


def test_axis_spans_hand_counted():
    # bin 1, g = 4, start 0: samples p + 0.125 .. p + 0.875 touch p and p + 1; the last pixel collapses onto size - 1
    assert R.axis_spans(0, 1, 4, 4, 4).tolist() == [2, 2, 2, 1]
    # g = 1 never touches more than 2
    assert R.axis_spans(0.3, 9.7, 5, 100, 1).tolist() == [2] * 5
    # bin 2: samples at 0.25, 0.75, 1.25, 1.75 (+ 2 p) touch 2 p .. 2 p + 2
    assert R.axis_spans(0, 2, 3, 100, 4).tolist() == [3, 3, 3]
    assert R.axis_spans(0.5, 2, 3, 100, 4).tolist() == [4, 4, 4]  # 0.75 .. 2.25
    # bin 4 exactly: the outer samples lie 3 apart: 0.5 .. 3.5 touches 0 .. 4
    assert R.axis_spans(0, 4, 3, 100, 4).tolist() == [5, 5, 5]
    # span 6 first appears over bin 4: bin 4.5, samples 0.5625 + 1.125 k: 0.5625 .. 3.9375 -> 0 .. 4; from 4.5: 5.0625 .. 8.4375 -> 5 .. 9
    assert R.axis_spans(0, 4.5, 2, 100, 4).tolist() == [5, 5]
    assert R.axis_spans(0.2, 4.5, 2, 100, 4).tolist() == [6, 5]   # 0.7625 .. 4.1375 -> 0 .. 5: six | 5.2625 .. 8.6375 -> 5 .. 9: five
    for g, first_slow in ((2, 6.0), (3, 4.5), (4, 4.0)):
        assert R.axis_spans(0.37, first_slow, 200, 4000, g).max() <= 5 < R.axis_spans(0.37, first_slow * 1.02, 200, 4000, g).max()
    # outside: no valid sample
    assert R.axis_spans(-50, 1, 4, 20, 4).tolist() == [0] * 4 and R.axis_spans(20.5, 1, 4, 20, 4).tolist() == [0] * 4
    # partly outside: samples -1.5 (dropped), -1, -0.5 (clamped to 0: touch 0 and 1), 0
    assert R.axis_spans(-1.75, 2, 1, 48, 4).tolist() == [2]


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_case_reaches_its_paths(case):
    t = R.check_paths(case)
    oh, ow = case.out_size
    assert t["separable"].shape == (-(-oh // 32), -(-ow // 64))


def test_table_covers_the_tile_shapes_and_ratios():
    sizes = {c.out_size for c in R.CASES}
    assert {(24, 32), (33, 70), (64, 128), (5, 3)} <= sizes
    assert {c.frame for c in R.CASES} == set(R.FRAMES)
    assert any(ow % 64 and ow > 64 for _, ow in sizes) and any(oh % 32 and oh > 32 for oh, _ in sizes)
    # at sampling ratios 1-3 the ratio cases still reach both paths
    for g, slow_names in ((1, set()), (2, {"bin6.6_slow"}), (3, {"bin6.6_slow"}), (4, {"bin4.4_alternating", "bin6.6_slow"})):
        slow = {c.name for c in R.RATIO_CASES if not R.tile_paths(c.box, c.out_size, R.FRAMES[c.frame], g)["separable"].all()}
        assert slow == slow_names, (g, slow)


@pytest.mark.parametrize("case", R.DEPTH_CASES, ids=repr)
def test_depth_rule_has_both_outcomes_and_no_borderline_pixels(case):
    frames = R.make_frames(case.frame)
    boxes, ids, zs = Y.case_inputs(case)
    for g in ((1, 2, 3, 4) if case.ratios else (4,)):
        mask = R.crop_ref(frames, boxes, ids, case.out_size, g)[1]
        near = np.abs(mask - R.VALID_THRESHOLD) <= Y.band_of_mask()
        zeroed = mask < R.VALID_THRESHOLD
        assert near.mean() <= 0.005, (case, g, near.mean())
        assert zeroed.mean() >= 0.05 and (~zeroed).mean() >= 0.05, (case, g, zeroed.mean())


def test_depth_modes_reach_both_ends_of_their_clamps():
    case = R.CASE_BY_NAME["bin2.6"]
    frames = R.make_frames(case.frame)
    boxes, ids, zs = Y.case_inputs(case)
    d2 = R.crop_ref(frames, boxes, ids, case.out_size, 4, depth_norm_z=zs, depth_norm_mode=2)[0][:, 3]
    d3 = R.crop_ref(frames, boxes, ids, case.out_size, 4, depth_norm_z=zs, depth_norm_mode=3)[0][:, 3]
    assert d2.min() == -1.0 and d2.max() == 1.0 and ((d2 > -1) & (d2 < 1)).any()
    assert d3.min() == -2.0 and d3.max() == 2.0 and ((d3 > -2) & (d3 < 2)).any()
    d1 = R.crop_ref(frames, boxes, ids, case.out_size, 4, depth_norm_z=zs, depth_norm_mode=1)[0][:, 3]
    d0 = R.crop_ref(frames, boxes, ids, case.out_size, 4)[0][:, 3]
    assert np.array_equal(d1, d0 / zs.astype(np.float64)[:, None, None])


def test_yardstick_figures():
    worst = {k: 0.0 for k in Y.MEASURED_F32_ERROR}
    for case in R.CASES:
        for g in ((1, 2, 3, 4) if case.ratios else (4,)):
            m = Y.measure(case, g)
            assert m.pop("near") <= 0.005
            for k, v in m.items():
                worst[k] = max(worst[k], v)
    print("float32 evaluation against float64, worst over the table:", {k: f"{v:.3g}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= Y.MEASURED_F32_ERROR[k] * 1.0001, (k, v)
        assert v >= Y.MEASURED_F32_ERROR[k] * 0.9, (k, v)  # the constants are the measurement, not a generous round-up


def test_both_float32_orders_differ_only_in_rounding():
    case = R.CASE_BY_NAME["bin3.6_full_fold"]
    frame = R.make_frames(case.frame)[1]
    a = Y.literal_f32(frame, case.box, case.out_size, 4)
    b = Y.folded_f32(frame, case.box, case.out_size, 4)
    assert not np.array_equal(a, b) and np.abs(a - b).max() <= 16 * 4 * 1.3 * 2.0 ** -23
