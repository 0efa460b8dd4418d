"""CPU tests of the detector stages' reference (tests/detect_ref.py), of the case tables it shares with
tests/test_gpu_detect_stages.py, and of the float32 yardstick (tests/detect_yardstick.py); and the argument errors of the seven entry
points, which need no GPU.

Measured here and written into detect_yardstick.MEASURED_F32_ERROR (worst |f32 - f64| / S over the tables): rpn_boxes 9.7e-8, rpn_wh
1.5e-7, rpn_scores 8.55e-8, nms_iou 2.98e-8, roi_level_v 2.49e-7, roi_coord 2.55e-7, roi_values 1.36e-6, box_scores 7.73e-8, box_boxes
1.23e-7, paste_corner 6.91e-8, paste_masks 2.05e-6, preprocess 5.55e-8, resize 3.29e-7.  The GPU tests allow the kernels 4x these
figures.  No decision of the tables is fragile (margin below 4x the error of its deciding quantity) but those of the cases marked
exact, and there the float32 evaluation takes the reference's decision (asserted below)."""

import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import detect_ref as R  # noqa: E402
import detect_yardstick as Y  # noqa: E402

F = np.float32


# ------------------------------------------------------------------------------------------- the reference against closed forms
def test_base_anchors_are_the_products_and_the_oracles():
    from happypose_amd.detector import base_anchors
    from oracle import detector as od

    for s in R.ANCHOR_SCALES:
        np.testing.assert_array_equal(R.base_anchors(s), base_anchors(s))
        np.testing.assert_array_equal(R.base_anchors(s), od.base_anchors(s))
    np.testing.assert_array_equal(R.base_anchors(32), [[-23, -11, 23, 11], [-16, -16, 16, 16], [-11, -23, 11, 23]])


def test_zero_deltas_return_the_anchor():
    base = R.base_anchors(64)
    idx = np.arange(5 * 7 * 3, dtype=np.int32)
    out = R.ref_rpn_decode(np.zeros(105, F), idx, np.zeros((5, 7, 12), F), 7, 3, base, 16, 8, 1e6, 1e6, 1e-3)
    a = idx % 3
    y, x = idx // 3 // 7, idx // 3 % 7
    want = np.stack([8 * x + base[a, 0], 16 * y + base[a, 1], 8 * x + base[a, 2], 16 * y + base[a, 3]], 1)
    np.testing.assert_array_equal(out["raw"], want)  # the stride of the columns is stride_w and x runs fastest
    np.testing.assert_array_equal(out["boxes"], np.maximum(want, 0))
    assert np.all(out["scores"] == 0.5)


def test_constant_map_and_affine_ramp_pool_exactly():
    shapes = R.ROI_SHAPES
    const = [np.full((2, h, w, 4), 1.5 + l, F) for l, (h, w) in enumerate(shapes)]
    rois = np.array([[1, 8.3, 6.1, 70.2, 50.9], [0, 2.0, 3.0, 90.0, 60.0]], F)  # every sample inside the map
    out = R.ref_roi_align_levels(const, R.ROI_SCALES, 2, rois, 7, 2)
    assert np.abs(out["values"] - 1.5).max() <= 1e-15 and list(out["levels"]) == [0, 0]
    yy, xx = np.mgrid[0:16, 0:24].astype(np.float64)
    ramp = np.stack([0.25 * xx - 0.5 * yy + 3.0, 2.0 * yy + 1.0], -1)[None].repeat(2, 0)
    ramp[1] += 100.0  # the second image differs
    out = R.ref_roi_align_levels([ramp.astype(F)] + const[1:], R.ROI_SCALES, 2, rois, 7, 3)
    for k in range(2):
        ys, xs, _, _ = out["coords"][k]
        assert ys.min() >= 0 and ys.max() <= 15 and xs.min() >= 0 and xs.max() <= 23
        want0 = 0.25 * xs.mean(1)[None, :] - 0.5 * ys.mean(1)[:, None] + 3.0 + 100.0 * rois[k, 0]
        want1 = 2.0 * ys.mean(1)[:, None] + 1.0 + 100.0 * rois[k, 0] + 0 * xs.mean(1)[None, :]
        assert np.abs(out["values"][k, :, :, 0] - want0).max() <= 1e-12 and np.abs(out["values"][k, :, :, 1] - want1).max() <= 1e-12


def test_constant_mask_pastes_to_its_sigmoid_and_decays_through_the_ring():
    c = 0.75
    logits = R.interleave_masks(np.full((1, 2, 28, 28), c, F), 4)
    logits[..., 0] = -3.0  # another class: not looked at
    box = np.array([[10.0, 10.0, 70.0, 50.0]], F)  # expanded: 7.86 .. 72.14 x 8.57 .. 51.43 -> 7 .. 72 x 8 .. 51: 66 x 44 px
    out = R.ref_paste_masks(logits, 4, [1], box, 1, 64, 96)
    m, (x0, x1, y0, y1) = out["masks"][0], out["rect"][0]
    assert (x0, x1, y0, y1) == (7, 73, 8, 52)
    p = 1.0 / (1.0 + np.exp(-c))
    # source coordinate of column x: 30 / 66 (x - 7 + 0.5) - 0.5; between 1 and 28 all four neighbours are inside the mask
    sx, sy = 30 / 66 * (np.arange(7, 73) - 7 + 0.5) - 0.5, 30 / 44 * (np.arange(8, 52) - 8 + 0.5) - 0.5
    inner = m[8:52, 7:73][np.ix_((sy >= 1) & (sy <= 28), (sx >= 1) & (sx <= 28))]
    assert inner.size > 1000 and np.abs(inner - p).max() <= 1e-15
    # in the ring the mask is p times the weight of the neighbours inside: a product of two ramps
    wx = np.clip(np.minimum(np.maximum(sx, 0), 29 - np.maximum(sx, 0)), 0, 1)
    wy = np.clip(np.minimum(np.maximum(sy, 0), 29 - np.maximum(sy, 0)), 0, 1)
    assert np.abs(m[8:52, 7:73] - p * wy[:, None] * wx[None, :]).max() <= 1e-15 and wx[0] < 0.3 and wy[-1] < 0.3
    m[8:52, 7:73] = 0
    assert not m.any()


def test_identity_resize_returns_the_normalised_image():
    x = R.images_case(2, 9, 13)
    a = R.ref_preprocess(x, Y.MEAN32, Y.STD32)
    b = R.ref_preprocess_resize(x, 9, 13, 32, 32, Y.MEAN32, Y.STD32)
    assert np.array_equal(b[:, :9, :13], a) and not b[:, 9:].any() and not b[:, :, 13:].any() and not a[..., 3].any()
    want = (x[1, 2, 4, 5].astype(np.float64) - float(F(0.406))) / float(F(0.225))
    assert a[1, 4, 5, 2] == want


# -------------------------------------------------------------------------------------------------- the reference against the oracle
def test_reference_agrees_with_the_oracle_on_benign_inputs():
    import torch

    from oracle import detector as od

    t = torch.as_tensor
    # decode + clip: anchors of a 5 x 7 map with square strides (the oracle knows one stride per axis from the image size)
    case = R.rpn_case("benign", 64)
    ref = R.ref_rpn_decode(case.obj, case.idx, case.deltas, 7, 3, case.base, 16, 8, 75.0, 50.0, 1e-3)
    anchors = od.level_anchors((80, 56), (5, 7), 64)[t(case.idx.astype(np.int64))]
    np.testing.assert_allclose(ref["anchors"], anchors.numpy(), rtol=0, atol=0)
    d = t(case.deltas.reshape(-1, 4))[t(case.idx.astype(np.int64))]
    want = od.clip_boxes(od.decode(d, anchors, (1.0, 1.0, 1.0, 1.0)).view(-1, 4), (75, 50)).numpy()
    np.testing.assert_allclose(ref["boxes"], want, rtol=0, atol=2e-5)
    np.testing.assert_allclose(ref["scores"], torch.sigmoid(t(case.obj)).numpy(), rtol=0, atol=2e-7)
    # box post-processing (integer image: clip_boxes takes the size as it is)
    n, nc, ld, ldr = 52, 5, 8, 20
    lg, rg, props = R.box_case(n, nc, ld, ldr, pad=0.0)
    refb = R.ref_box_postprocess(lg, ld, rg, ldr, props, n, nc, 61, 83)
    want = od.clip_boxes(od.decode(t(rg), t(props), (10.0, 10.0, 5.0, 5.0)).reshape(n, -1, 4), (61, 83)).numpy()
    np.testing.assert_allclose(refb["boxes"], want, rtol=0, atol=1e-4)
    np.testing.assert_allclose(refb["scores"], torch.softmax(t(lg[:, :nc]), -1).numpy(), rtol=0, atol=2e-7)
    # NMS
    for name in ("cloud130", "chain", "identical"):
        c = R.nms_case(name)
        sc = np.linspace(1, 0, len(c.boxes)).astype(F)
        want = od.batched_nms(t(c.boxes), t(sc), t(c.group.astype(np.int64)), float(c.thr)).numpy()
        assert sorted(np.where(R.ref_nms(c.boxes, c.group, c.thr)["keep"])[0].tolist()) == sorted(want.tolist())
    # levels and RoIAlign: random rois inside the image, the oracle's order (image 0 first)
    rs = np.random.RandomState(3)
    ctr, wh = rs.uniform((20, 15), (76, 49), (12, 2)), rs.uniform(6, 30, (12, 2))
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(F)
    boxes[3], boxes[9] = (-100.7, -120.3, 180.2, 200.4), (-250.2, -280.6, 330.4, 350.1)
    rois = np.concatenate([(np.arange(12) >= 6).astype(F)[:, None], boxes], 1)
    maps = R.roi_maps(8)
    refr = R.ref_roi_align_levels(maps, R.ROI_SCALES, 2, rois, 7, 2)
    feats = [t(np.ascontiguousarray(m.transpose(0, 3, 1, 2))) for m in maps]
    want, lv = od.multiscale_roi_align(feats, [t(boxes[:6]), t(boxes[6:])], R.ROI_IMAGE, 7)
    assert list(lv.numpy()) == list(refr["levels"]) == list(od.map_levels(t(boxes)).numpy()) and len(set(refr["levels"])) >= 3
    np.testing.assert_allclose(refr["values"].transpose(0, 3, 1, 2), want.numpy(), rtol=0, atol=2e-5 * 4)
    # mask pasting
    pc = R.paste_case(pad=0.0)
    refp = R.ref_paste_masks(pc.logits, R.PASTE_LD, pc.labels, pc.boxes, len(pc.boxes), pc.H, pc.W)
    prob = torch.sigmoid(t(pc.nchw))[torch.arange(len(pc.boxes)), t(pc.labels.astype(np.int64))][:, None]
    want = od.paste_masks(prob, t(pc.boxes), (pc.H, pc.W)).numpy()[:, 0]
    np.testing.assert_allclose(refp["masks"], want, rtol=0, atol=2e-5)
    # the transform: 9 x 13 -> 6 x 8 (the size torchvision's scale rule gives) on a 32 x 32 canvas
    x = R.images_case(2, 9, 13)
    canvas, (hr, wr) = od.transform(t(x), 6, 9)
    assert (hr, wr) == (6, 8) and tuple(canvas.shape[-2:]) == (32, 32)
    got = R.ref_preprocess_resize(x, hr, wr, 32, 32, Y.MEAN32, Y.STD32)
    np.testing.assert_allclose(got[..., :3].transpose(0, 3, 1, 2), canvas.numpy(), rtol=0, atol=3e-6)


# ------------------------------------------------------------------------------------------------------------------- the yardstick
def test_yardstick_figures_and_decisions():
    w = Y.measure()
    for k, v in Y.MEASURED_F32_ERROR.items():
        assert w[k] <= v <= 1.01 * w[k], (k, v, w[k])  # the recorded figure is the measured one, rounded up
    assert w["decisions"] == 0  # the float32 evaluation takes every decision as the reference does, the exact cases included


def test_no_fragile_decision_outside_the_exact_cases():
    for g, s in R.RPN_CASES:
        case = R.rpn_case(g, s)
        fr = Y.rpn_fragile(case, R.rpn_ref(case))
        assert case.exact == bool(fr.any()), (case.name, int(fr.sum()))
    for name in R.NMS_CASES:
        case = R.nms_case(name)
        fr = Y.nms_fragile(R.ref_nms(case.boxes, case.group, case.thr))
        assert case.exact == bool(fr.any()), (name, int(fr.sum()))
    for name, maps, scales, shapes, rois, out, g in R.roi_calls():
        ref = R.ref_roi_align_levels(maps, scales, 2, rois, out, g)
        lv, sm = Y.roi_fragile(ref, rois, scales, shapes)
        assert not sm.any(), (name, np.argwhere(sm)[:4])
        # the exact octaves sit 1e-6 above their floor, a hair over the band of 4 x 2.49e-7: they are compared like every other
        exact = np.array([r[0] in R.ROI_EXACT for r in R.ROIS] if len(rois) == len(R.ROIS) else [False] * len(rois))
        assert not lv.any() and (ref["level_margin"][exact] < 1.001e-6).all() and (ref["level_margin"][~exact] > 0.1).all(), (name, lv)
    pc = R.paste_case()
    refp = R.ref_paste_masks(pc.logits, R.PASTE_LD, pc.labels, pc.boxes, len(pc.boxes), pc.H, pc.W)
    assert not Y.paste_fragile(pc, refp).any() and refp["trunc_margin"].min() > 0.01


# ------------------------------------------------------------------------------------------------- each case reaches its path
def test_rpn_cases_reach_their_paths():
    seen = set()
    for g, s in R.RPN_CASES:
        case = R.rpn_case(g, s)
        ref = R.rpn_ref(case)
        b, raw, cm = ref["boxes"], ref["raw"], ref["clamp_margin"]
        assert np.isfinite(raw).all() and (ref["scores"] >= 0).all() and (ref["scores"] <= 1).all()
        assert len(case.idx) == {"single": 1, "two_blocks": 257}.get(g, 105) and len(set(case.idx.tolist())) == len(case.idx)
        assert (case.stride_h, case.stride_w, case.im_h, case.im_w) == (16, 8, 75.0, 50.0)
        assert list(case.obj[:5]) == [-100, -1, 0, 1, 100][:len(case.obj)]
        if g == "benign":
            assert (b[:, 2] == 50).any() and (b[:, 3] == 75).any() and (b[:, 0] == 0).any() and (b[:, 1] == 0).any()  # clipping
            assert (raw[:, 2] > 50).any() and (raw[:, 3] > 75).any() and (case.idx[:-1] > case.idx[1:]).any()
            if s == 32:
                assert ref["valid"].any()
        if g == "clamped":
            assert (cm > 0).any() and (cm == 0).any() and (cm < 0).any() and float(cm.max()) > 45
            assert np.abs(ref["wh"][cm > 0] / (ref["anchors"][:, 2:] - ref["anchors"][:, :2])[cm > 0] - 62.5).max() < 1e-5
        if g == "collapsed":
            assert not ref["valid"].any() and (ref["wh"].min(1) < 1e-5).all()
        if g == "off_side":
            assert not ref["valid"].any()
            for side in ((b[:, 2] == 0), (b[:, 0] == 50), (b[:, 3] == 0), (b[:, 1] == 75)):
                assert side.sum() >= 20
        if g == "two_blocks":
            assert (case.gh, case.gw) == (9, 10)
        if g.startswith("exact"):
            at = (ref["valid_margin"] < 1e-5)
            assert at.sum() >= 3 and ref["valid"][at].all() == (g == "exact_at") and ref["valid"][at].any() == (g == "exact_at")
            assert np.array_equal(ref["boxes"], np.round(ref["boxes"])) and float(case.min_size) == (22.0 if g == "exact_at" else 22.000001907348633)
        seen.add(g)
    assert seen == set(R.RPN_GROUPS) | {"exact_at", "exact_above"}


def test_nms_cases_reach_their_paths():
    for name in R.NMS_CASES:
        case = R.nms_case(name)
        ref = R.ref_nms(case.boxes, case.group, case.thr)
        assert np.array_equal(case.boxes * 4, np.round(case.boxes * 4)) and np.abs(case.boxes).max() < 1024  # the 1/4-px grid
        assert np.array_equal(Y.iou_f32(case.boxes)[np.isfinite(ref["margin"])] > case.thr, (ref["iou"] > float(case.thr))[np.isfinite(ref["margin"])])
        for i, k in case.expect.items():
            assert bool(ref["keep"][i]) == k, (name, i)
        if len(case.boxes) >= 3:
            assert set(case.group[:3]) == {0, 1, 2}
        n = len(case.boxes)
        if name.startswith("cloud"):
            assert n == int(name[5:]) and (n < 60 or 0.2 < ref["keep"].mean() < 0.9)
            cross = (case.group[:, None] != case.group[None, :]) & (ref["iou"] > 0.5)
            assert n < 60 or cross.any()  # overlapping boxes of different groups are there, and they do not count
        else:
            rest = np.setdiff1d(np.arange(n), list(case.expect))
            assert ref["keep"][rest].all()
    c = R.nms_case("iou_half")
    assert R.ref_nms(c.boxes, c.group, c.thr)["iou"][3, 6] == 0.5 and float(R.nms_case("iou_half_below").thr) == 0.5 - 2.0 ** -25
    c = R.nms_case("chain")
    iou = R.ref_nms(c.boxes, c.group, c.thr)["iou"]
    assert iou[3, 66] > 0.5 and iou[66, 129] > 0.5 and iou[3, 129] < 0.5 and len({3 // 64, 66 // 64, 129 // 64}) == 3
    c = R.nms_case("zero_area")
    iou = R.ref_nms(c.boxes, c.group, c.thr)["iou"]
    assert np.isnan(iou[0, 3]) and iou[0, 6] == 0 and iou[6, 9] == 0 and c.group[0] == c.group[3] == c.group[6] == c.group[69]


def test_roi_cases_reach_their_paths():
    rois, names = R.roi_table(), [r[0] for r in R.ROIS]
    ref = R.ref_roi_align_levels(R.roi_maps(8), R.ROI_SCALES, 2, rois, 7, 2)
    lv, v = dict(zip(names, ref["levels"])), dict(zip(names, ref["v"]))
    assert [lv[f"level{i}"] for i in range(4)] == [0, 1, 2, 3] and all(2 + i < v[f"level{i}"] < 3 + i for i in range(4))
    assert v["below_clamp"] < 2 and lv["below_clamp"] == 0 and v["above_clamp"] > 6 and lv["above_clamp"] == 3
    assert v["zero_area"] == -np.inf and lv["zero_area"] == 0
    for name, k in (("octave_112", 1), ("octave_224", 2), ("octave_448", 3)):
        assert lv[name] == k and abs(v[name] - (k + 2) - 1e-6) < 1e-9 and np.floor(Y.level_v32(rois)[names.index(name)]) == k + 2
    assert ref["size_margin"][names.index("narrow"), 0] < 0 and (ref["size_margin"][names.index("zero_area")] < [0, 9]).all()
    img = rois[:, 0]
    assert set(img) == {0, 1} and (np.diff(img) > 0).any() and (np.diff(img) < 0).any()  # mixed, not sorted
    ys, xs, H, W = ref["coords"][names.index("x1_negative")]
    assert (xs < -1).any() and ((xs > -1) & (xs < 0)).any()
    ys, xs, H, W = ref["coords"][names.index("past_far_edge")]
    for c, n in ((ys, H), (xs, W)):
        assert ((c > n - 1) & (c < n)).any() and (c > n).any() and (c < n - 1).any()
    assert {(C, o, g) for C, o, g in R.ROI_CONFIGS} >= {(8, o, g) for o in (1, 7, 14) for g in (1, 2, 3)} | {(256, 7, 2), (256, 14, 2)}
    maps, scales, r, o, g = R.roi_big_case()
    assert maps[0].shape == (2, 2, 2, 4096) and list(r[:, 0]) == [1, 0] and not np.array_equal(maps[0][0], maps[0][1])
    for m in R.roi_maps(8):
        assert np.abs(m[0] - m[1]).min() > 0  # no element of the two images coincides


def test_box_and_paste_cases_reach_their_paths():
    seen = dict(clamp=0, equal=0, big=0, huge=0, zero_w=0, left=0, right=0, top=0, bottom=0, negative=0)
    for n, nc, ld, ldr in R.BOX_CASES:
        lg, rg, props = R.box_case(n, nc, ld, ldr)
        assert np.isnan(lg[:, nc:]).all() and np.isnan(rg[:, 4 * nc:]).all() and (ld > nc or n == 1)
        ref = R.ref_box_postprocess(lg, ld, rg, ldr, props, n, nc, *R.BOX_IMAGE)
        assert np.isfinite(ref["boxes"]).all() and np.abs(ref["scores"].sum(1) - 1).max() < 1e-12
        seen["clamp"] += int((ref["clamp_margin"] > 0).sum()); seen["negative"] += int((rg[:, :4 * nc] < -30).sum())
        seen["equal"] += int((np.ptp(lg[:, :nc], 1) == 0).sum()); seen["big"] += int((np.abs(lg[:, :nc]) == 80).all(1).sum()); seen["huge"] += int((np.abs(lg[:, :nc]) == 100).all(1).sum())
        seen["zero_w"] += int((props[:, 2] == props[:, 0]).sum())
        raw, b = ref["raw"], ref["boxes"]
        seen["left"] += int(((raw[..., 2] < 0) & (b[..., 2] == 0)).sum()); seen["right"] += int(((raw[..., 0] > 83.25) & (b[..., 0] == 83.25)).sum())
        seen["top"] += int(((raw[..., 3] < 0) & (b[..., 3] == 0)).sum()); seen["bottom"] += int(((raw[..., 1] > 61.5) & (b[..., 1] == 61.5)).sum())
    assert all(v > 0 for v in seen.values()), seen
    with np.errstate(over="ignore"):
        assert 52 * 5 > 256 and np.isinf(np.exp(F(100)))
    pc = R.paste_case()
    ref = R.ref_paste_masks(pc.logits, R.PASTE_LD, pc.labels, pc.boxes, len(pc.boxes), pc.H, pc.W)
    name = [b[0] for b in R.PASTE_BOXES]
    c, rect = dict(zip(name, ref["corners"])), dict(zip(name, ref["rect"].tolist()))
    assert (pc.H, pc.W) == (37, 300) and np.isnan(pc.logits[..., 5:]).all() and set(pc.labels) == {1, 2, 3, 4}
    assert -1 < c["negative_corner"][0] < -0.5 and -1 < c["negative_corner"][1] < 0 and rect["negative_corner"][0] == rect["negative_corner"][2] == 0
    assert rect["beyond_image"] == [0, 300, 0, 37] and c["beyond_image"][0] < -1 and c["beyond_image"][2] > 301
    assert rect["sub_pixel"] == [150, 151, 20, 21] and rect["zero_at_origin"] == [0, 1, 0, 1]
    assert rect["far_corner"][1] == 300 and rect["far_corner"][3] == 37 and c["far_corner"][2] > 300 and c["far_corner"][3] > 37
    assert rect["second_pass"][:2] == [250, 300] and rect["interior"][0] > 0 and rect["interior"][1] < 256
    assert ref["masks"][name.index("interior")].max() > 0.9
    for a in range(5):
        for b in range(a):
            assert np.abs(pc.nchw[:, a] - pc.nchw[:, b]).min() > 0  # the planes of two classes differ everywhere
    for n, h, w in R.PREPROCESS_CASES:
        assert (n * h * w) % 256 != 0 and n == 2
    assert 2 * 13 * 21 > 256 and not np.array_equal(*R.images_case(2, 5, 7))


# ----------------------------------------------------------------------------------------------- argument errors without a GPU
P = 4096  # stands for a device pointer: an argument error is reported before anything is dereferenced


def test_detector_stage_argument_errors_without_gpu():
    from happypose_amd import _ffi

    lib = _ffi.lib()
    f = C.c_float
    base = (f * 12)()
    ptrs, ints, flts = (C.c_void_p * 5)(*[P] * 5), (C.c_int * 5)(*[4] * 5), (f * 5)(*[0.25] * 5)

    def rpn(n=4, n_anchors=3, obj=P):
        return lib.hp_rpn_decode(obj, P, n, P, 7, n_anchors, base, 16, 8, f(75), f(50), f(1e-3), P, P, P, None)

    def roi(n_levels=4, Cn=8, K=2, rois=P):
        return lib.hp_roi_align_levels(ptrs, ints, ints, flts, n_levels, 2, Cn, rois, K, 7, 2, P, None, None)

    def box(n=3, nc=4, ld=4, ldr=16, lg=P):
        return lib.hp_box_postprocess(lg, ld, P, ldr, P, n, nc, f(60), f(80), P, P, None)

    def paste(n=2, ld=8, ml=P):
        return lib.hp_paste_masks(ml, ld, P, P, n, 37, 300, P, None)

    def nms(n=4, boxes=P):
        return lib.hp_nms(boxes, P, n, f(0.5), P, None)

    for call, name in ((lambda: nms(n=65537), b"hp_nms"), (lambda: nms(n=-1), b"hp_nms"), (lambda: rpn(n_anchors=2), b"hp_rpn_decode"),
                       (lambda: rpn(n_anchors=4), b"hp_rpn_decode"), (lambda: roi(Cn=6), b"hp_roi_align_levels"),
                       (lambda: roi(n_levels=5), b"hp_roi_align_levels"), (lambda: roi(Cn=4100), b"hp_roi_align_levels"),
                       (lambda: box(ld=3), b"hp_box_postprocess"), (lambda: box(ldr=15), b"hp_box_postprocess"),
                       (lambda: paste(ld=0), b"hp_paste_masks")):
        assert call() == -1 and name in lib.hp_last_error(), name
    # nothing to do: HP_OK, nothing launched, no pointer looked at
    assert nms(n=0, boxes=None) == 0 and rpn(n=0, obj=None) == 0 and roi(K=0, rois=None) == 0 and box(n=0, lg=None) == 0 and paste(n=0, ml=None) == 0
    mean, std = (f * 3)(*R.IMAGE_MEAN), (f * 3)(*R.IMAGE_STD)
    assert lib.hp_detector_preprocess(P, 0, 5, 7, mean, std, P, None) == 0
    assert lib.hp_detector_preprocess_resize(P, 0, 9, 13, 6, 9, 32, 32, mean, std, P, None) == 0
    assert lib.hp_detector_preprocess_resize(P, 1, 9, 13, 6, 9, 4, 32, mean, std, P, None) == -1 and b"hp_detector_preprocess_resize" in lib.hp_last_error()
