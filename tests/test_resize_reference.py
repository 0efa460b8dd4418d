"""tests/resize_ref.py and the host half of the resize (ops.resize_tables, the K of CropResizeToAspectTransform) against their
yardsticks, without a GPU: Pillow 12.2's recorded output (tests/golden/g15_resize.npz, tools/gen_golden_resize.py) in 0 bytes, the
oracle's get_K_crop_resize, and the reference's make_detections_from_segmentation restated literally."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(ROOT))
import resize_ref as R  # noqa: E402
from oracle.geometry import get_K_crop_resize  # noqa: E402

from happypose_amd import augmentations as A  # noqa: E402
from happypose_amd import ops  # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(golden_dir / "g15_resize.npz"))


def test_golden_file_is_the_case_table(golden, golden_dir):
    inputs = R.golden_inputs()
    for kind, table in inputs.items():
        for name, x in table.items():
            assert np.array_equal(golden[f"in|{kind}|{name}"].view(np.uint8), x.view(np.uint8)), (kind, name)
    want = {f"rgb|{c}|{f}" for c in R.GOLDEN_CASES for f in (*R.GOLDEN_FILTERS, "default")}
    want |= {f"{k}|{c}" for c, v in R.GOLDEN_CASES.items() if v[0] in inputs["i32"] for k in ("i32", "f32")}
    assert want == {k for k in golden if k.split("|")[0] in ("rgb", "i32", "f32")}
    assert str(golden["pillow_version"]).startswith("12.")
    assert (golden_dir / "g15_resize.npz").stat().st_size <= (golden_dir / "g14_augmentations.npz").stat().st_size


def _input(golden, kind, case):
    src, out, box, crop = R.GOLDEN_CASES[case]
    x = golden[f"in|{kind}|{src}"]
    return (x if crop is None else R.crop_pad(x, crop)), out, box


@pytest.mark.parametrize("case", sorted(R.GOLDEN_CASES))
def test_restatement_equals_pillow(golden, case):
    x, out, box = _input(golden, "rgb", case)
    for f in (*R.GOLDEN_FILTERS, "default"):  # Pillow's default filter is bicubic
        y = R.resize_rgb(x, out, R.BICUBIC if f == "default" else f, box)
        assert int((y != golden[f"rgb|{case}|{f}"]).sum()) == 0, f
    if f"i32|{case}" in golden:
        for kind in ("i32", "f32"):
            x, out, box = _input(golden, kind, case)
            y = R.resize_nearest(x, out, box)
            assert y.dtype == x.dtype and np.array_equal(y.view(np.uint32), golden[f"{kind}|{case}"].view(np.uint32)), kind


def test_golden_has_the_hard_pixels(golden):
    """Bicubic overshoot clipped at both ends, a NaN and a negative depth that survive, and the skipped passes."""
    y = golden["rgb|checker2_11x20_to_37x53|bicubic"]
    assert (y == 0).any() and (y == 255).any()
    assert not golden["rgb|zeros_37x53_to_11x20|bicubic"].any() and (golden["rgb|ones_37x53_to_11x20|bicubic"] == 255).all()
    d = golden["f32|11x20_to_37x53"]
    assert np.isnan(d).any() and (d < 0).any()
    assert np.array_equal(golden["rgb|13x17_same|bicubic"], golden["in|rgb|random_13x17"])


@pytest.mark.parametrize("case", sorted(R.GOLDEN_CASES))
def test_host_tables_equal_the_restatement(case):
    """ops.resize_tables (vectorised float64) gives the restatement's windows and fixed-point weights, in source pixels."""
    src, out, box, crop = R.GOLDEN_CASES[case]
    h, w = (int(v) for v in src.split("_")[1].split("x"))
    cx0, cy0, cx1, cy1 = (0, 0, w, h) if crop is None else crop
    x0, y0, x1, y1 = (0, 0, cx1 - cx0, cy1 - cy0) if box is None else box
    for f in R.GOLDEN_FILTERS:
        t = ops.resize_tables((h, w), out, box, f, crop)
        for axis, size, b0, b1, n_out, origin in (("x", cx1 - cx0, x0, x1, out[1], cx0), ("y", cy1 - cy0, y0, y1, out[0], cy0)):
            bounds, weights = t[f"{axis}bounds"], t[f"{axis}weights"]
            assert bounds.dtype == weights.dtype == np.int32
            for i, (lo, q) in enumerate(R.coefficients(size, b0, b1, n_out, f)):
                assert tuple(bounds[i]) == (lo + origin, len(q)) and list(weights[i, :len(q)]) == q and not weights[i, len(q):].any()
        assert t["skip_x"] == (case == "13x17_same" or case == "13x17_to_29x17")
        assert t["skip_y"] == (case == "13x17_same" or case == "13x17_to_13x40")
    assert ops.resize_tables((5, 1031), (3, 64))["band_x"] == 1031  # one tile's windows cover the whole line


def test_crop_rounds_as_pillow(golden):
    """The float box of the aspect crop and the size Image.crop gave it: 7.625 .. 32.375 -> 24 rows, 1.5 .. 31.5 -> 2 .. 32 (halves
    to the even integer: 30 rows, not 31 or 29), -5 .. 25 -> 30 rows, 5 of them padding on either side."""
    T = A.CropResizeToAspectTransform((24, 32))
    for (h, w), rect in (((40, 33), (0, 8, 33, 32)), ((33, 40), (0, 2, 40, 32)), ((20, 40), (0, -5, 40, 25))):
        rec = golden[f"crop_round|{h}x{w}"]
        box = T.crop_box(h, w)
        assert box == tuple(rec[:4]) == R.aspect_crop_box(h, w, (24, 32))
        assert R.pil_round_box(box) == rect and (rect[3] - rect[1], rect[2] - rect[0]) == tuple(rec[4:])
    assert T.crop_box(48, 64) is None and T.crop_box(480, 640) is None


def test_K_equals_two_calls_of_the_oracle():
    K = np.array([[[600.0, 0, 320.5], [0, 610.0, 239.25], [0, 0, 1]], [[300.0, 0, 17.0], [0, 310.0, 19.0], [0, 0, 1]]], np.float32)
    T = A.CropResizeToAspectTransform((24, 32))
    for h, w in ((40, 33), (33, 40), (20, 40), (48, 64), (1080, 1920)):
        box, got, want, (ch, cw) = T.crop_box(h, w), K, K, (h, w)
        if box is not None:
            sizes = (box[3] - box[1], box[2] - box[0])
            got = A.k_crop_resize(got, box, sizes)
            want = get_K_crop_resize(want, np.array([box, box], np.float32), (h, w), sizes)
            rect = R.pil_round_box(box)
            ch, cw = rect[3] - rect[1], rect[2] - rect[0]
        got = A.k_crop_resize(got, (0, 0, cw, ch), (24, 32))
        want = get_K_crop_resize(want, np.array([[0, 0, cw, ch]] * 2, np.float32), (ch, cw), (24, 32))
        assert got.dtype == np.float32 and np.array_equal(got, want), (h, w)
        assert np.array_equal(R.crop_resize_to_aspect(np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.int32), None, K[0], (24, 32),
                                                      get_K_crop_resize)[3], want[0])


def test_boxes_equal_make_detections_from_segmentation():
    rng = np.random.default_rng(4)
    for h, w in ((7, 11), (33, 65), (48, 64)):
        s = rng.integers(0, 6, (h, w)).astype(np.int32)
        s[s == 4] = 0          # id 4 is absent
        s[h // 2, w // 2] = 9  # one pixel
        dets = R.detections_from_segmentation(s)
        ids = [0, 1, 2, 3, 4, 5, 9]
        boxes, n_px = R.seg_boxes(s, ids)
        assert sorted(dets) == [i for i, n in zip(ids, n_px) if n]
        for k, i in enumerate(ids):
            if i in dets:
                assert np.array_equal(boxes[k], dets[i]) and n_px[k] == (s == i).sum()
        assert n_px[4] == 0 and n_px[6] == 1 and list(boxes[6]) == [w // 2, h // 2, w // 2, h // 2]
