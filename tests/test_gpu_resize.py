"""The frame-geometry kernels (csrc/resize.hip) on the device: byte equality with Pillow, no tolerance.

``resize_rgb`` / ``resize_nearest`` against every array of tests/golden/g15_resize.npz (Pillow 12.2's own output): all cases of
one (input size, output size) in ONE batch, each image with its own box and crop, both filters, rows with ``apply = 0`` left
untouched.  ``seg_boxes``, ``CropResizeToAspectTransform`` and ``ReplaceBackgroundTransform(resize_background=True)`` against
tests/resize_ref.py, which test_resize_reference.py pins to the same file.  Every result is computed twice: same bits.

Shapes: 1 x 1 .. 40 x 33 and the 5 x 1031 line (one tile's windows cover the whole line: the band is sized from the tables); out
widths below and above one tile of 256 only matter for the band, which 5 x 1031 -> 3 x 64 and 13 x 17 -> 3 x 300 cover."""

import sys
from collections import defaultdict
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import resize_ref as R  # noqa: E402

from happypose_amd import augmentations as A  # noqa: E402
from happypose_amd import ops  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle.geometry import get_K_crop_resize  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return torch.equal(bits(a), bits(b))


def twice(fn):
    """The call's result, after checking that a second call gives the same bits."""
    a, b = fn(), fn()
    assert same(a, b)
    return a


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(golden_dir / "g15_resize.npz"))


def _groups():
    """Cases that share input and output size: one batch each."""
    groups = defaultdict(list)
    for case, (src, out, box, crop) in R.GOLDEN_CASES.items():
        groups[(src.split("_")[1], out)].append(case)
    return dict(groups)


GROUPS = _groups()


def _batch(golden, kind, cases):
    """Inputs, boxes [B, 4] and crops [B, 4] of the cases (a missing box or crop spelled out, so that the rows differ)."""
    x, boxes, crops = [], [], []
    for case in cases:
        src, out, box, crop = R.GOLDEN_CASES[case]
        a = golden[f"in|{kind}|{src}"]
        h, w = a.shape[:2]
        crop = (0, 0, w, h) if crop is None else crop
        x.append(a), crops.append(crop), boxes.append((0, 0, crop[2] - crop[0], crop[3] - crop[1]) if box is None else box)
    return dev(np.stack(x)), np.array(boxes), np.array(crops)


@pytest.mark.parametrize("filt", ["bilinear", "bicubic", "default"])
@pytest.mark.parametrize("group", sorted(GROUPS), ids=lambda g: f"{g[0]}_to_{g[1][0]}x{g[1][1]}")
def test_resize_rgb_equals_pillow(golden, group, filt):
    cases = GROUPS[group]
    x, boxes, crops = _batch(golden, "rgb", cases)
    name = "bicubic" if filt == "default" else filt  # Pillow's default filter is bicubic
    y = twice(lambda: ops.resize_rgb(x, group[1], name, box=boxes, crop=crops))
    for i, case in enumerate(cases):
        want = golden[f"rgb|{case}|{filt}"]
        assert int((y[i].cpu().numpy() != want).sum()) == 0, case
    # without box and crop (None): the cases that have neither, through the other spelling
    plain = [i for i, c in enumerate(cases) if R.GOLDEN_CASES[c][2] is None and R.GOLDEN_CASES[c][3] is None]
    if plain:
        y2 = ops.resize_rgb(x[plain].contiguous(), group[1], name)
        assert torch.equal(y2, y[plain])
    # apply = 0: the image's output keeps what out held
    flags = np.arange(len(cases)) % 2 == 1
    out = torch.full_like(y, 7)
    y3 = ops.resize_rgb(x, group[1], name, box=boxes, crop=crops, apply=flags, out=out)
    assert y3 is out
    for i in range(len(cases)):
        assert torch.equal(y3[i], y[i] if flags[i] else torch.full_like(y[i], 7)), i


@pytest.mark.parametrize("group", sorted(GROUPS), ids=lambda g: f"{g[0]}_to_{g[1][0]}x{g[1][1]}")
def test_resize_nearest_equals_pillow(golden, group):
    cases = [c for c in GROUPS[group] if R.GOLDEN_CASES[c][0].startswith("random")]  # constant frames and checkerboards: RGB only
    assert cases
    for kind, dtype in (("i32", torch.int32), ("f32", torch.float32)):
        x, boxes, crops = _batch(golden, kind, cases)
        assert x.dtype == dtype
        y = twice(lambda: ops.resize_nearest(x, group[1], box=boxes, crop=crops))
        assert y.dtype == dtype
        for i, case in enumerate(cases):
            want = golden[f"{kind}|{case}"]
            assert np.array_equal(y[i].cpu().numpy().view(np.uint32), want.view(np.uint32)), (kind, case)
        flags = np.arange(len(cases)) % 2 == 0
        y3 = ops.resize_nearest(x, group[1], box=boxes, crop=crops, apply=flags)
        for i in range(len(cases)):
            assert same(y3[i], y[i] if flags[i] else torch.zeros_like(y[i])), i


def test_nearest_passes_nan_and_negative_depth(golden):
    """The 37 x 53 depth map holds a NaN and a -1.5; an upscale by 2 reaches every source pixel, so both arrive, as bits."""
    x = dev(golden["in|f32|random_37x53"][None])
    src = x[0].cpu().numpy()
    assert np.isnan(src).sum() == 1 and (src < 0).sum() == 1
    y = ops.resize_nearest(x, (74, 106))[0].cpu().numpy()
    want = R.resize_nearest(src, (74, 106))
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    assert np.isnan(y).sum() == 4 and (y == -1.5).sum() == 4


def test_band_is_sized_from_the_tables():
    """13 x 700 -> 3 x 300 has two tiles of output pixels (256 + 44); 5 x 1031 -> 3 x 64 (golden) has one whose windows cover the
    whole line.  A band beyond the maximum is an error before any launch."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (13, 700, 3), dtype=np.uint8)
    for filt in ("bilinear", "bicubic"):
        y = twice(lambda: ops.resize_rgb(dev(a[None]), (3, 300), filt))
        assert np.array_equal(y[0].cpu().numpy(), R.resize_rgb(a, (3, 300), filt))
    wide = torch.zeros((1, 1, 3 * ops.RESIZE_MAX_BAND, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="band"):
        ops.resize_rgb(wide, (1, 64), "bilinear")


SEG_SHAPES = [(7, 11), (33, 65), (48, 64)]


def _seg_maps(h, w):
    """Image 0: id 3 touches all four borders (a frame), id 5 is one pixel, id 9 is absent, a block of id 2 and id -4; image 1:
    background only; image 2: random ids 0 .. 15."""
    rng = np.random.default_rng(h * 100 + w)
    s = np.zeros((3, h, w), np.int32)
    s[0, 0, :], s[0, -1, :], s[0, :, 0], s[0, :, -1] = 3, 3, 3, 3
    s[0, h // 2, w // 3] = 5
    s[0, 2:h - 2, w // 2:w - 2] = 2
    s[0, 1, 1:3] = -4
    s[2] = rng.integers(0, 16, (h, w))
    return s


@pytest.mark.parametrize("h,w", SEG_SHAPES)
def test_seg_boxes_equals_reference(h, w):
    s = _seg_maps(h, w)
    ids = [[3, 5, 9, 2, -4, 0], [1, 2], list(range(16))]  # max_ids 16, ragged
    boxes, n_px = ops.seg_boxes(dev(s), ids)
    again = ops.seg_boxes(dev(s), ids)
    assert torch.equal(n_px, again[1]) and torch.equal(boxes[n_px > 0], again[0][again[1] > 0])  # two calls: same bits
    assert boxes.shape == (3, 16, 4) and n_px.shape == (3, 16) and boxes.dtype == n_px.dtype == torch.int32
    boxes, n_px = boxes.cpu().numpy(), n_px.cpu().numpy()
    for b in range(3):
        want_boxes, want_n = R.seg_boxes(s[b], ids[b])
        dets = R.detections_from_segmentation(s[b])
        assert np.array_equal(n_px[b, :len(ids[b])], want_n) and not n_px[b, len(ids[b]):].any()
        for k, i in enumerate(ids[b]):
            if want_n[k]:
                assert np.array_equal(boxes[b, k], want_boxes[k]) and np.array_equal(boxes[b, k], dets[i]), (b, i)
            else:
                assert i not in dets
    assert n_px[0, 1] == 1 and n_px[0, 2] == 0 and list(boxes[0, 0]) == [0, 0, w - 1, h - 1]  # one pixel, absent, all borders
    assert not n_px[1].any()  # background only, and 0 is not asked for
    # max_ids 1, as a device tensor with counts
    one = dev(np.array([[3], [0], [7]], np.int32))
    b1, n1 = ops.seg_boxes(dev(s), one)
    assert b1.shape == (3, 1, 4)
    for b, i in enumerate((3, 0, 7)):
        wb, wn = R.seg_boxes(s[b], [i])
        assert int(n1[b, 0]) == wn[0] and np.array_equal(b1[b, 0].cpu().numpy(), wb[0])
    _, n0 = ops.seg_boxes(dev(s), one, count=[1, 0, 1])
    assert int(n0[1, 0]) == 0 and int(n0[0, 0]) == int(n1[0, 0])


def _frames(h, w, n, seed):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    seg = rng.integers(0, 4, (n, h, w)).astype(np.int32)
    seg[:, h // 2, w // 2] = 9  # one pixel
    depth = rng.uniform(0.3, 2.0, (n, h, w)).astype(np.float32)
    depth[:, 0, 0], depth[:, h // 2, w // 2] = np.nan, -0.5
    K = np.tile(np.array([[600.0, 0, w / 2 - 0.25], [0, 610.0, h / 2 + 0.5], [0, 0, 1]], np.float32), (n, 1, 1))
    K[1:, 0, 0] += 17.0
    return rgb, seg, depth, K


@pytest.mark.parametrize("h,w", [(40, 33), (33, 40), (20, 40), (24, 32)])
def test_crop_resize_to_aspect_end_to_end(h, w):
    """Two frames per size: 40 x 33 (crop box 7.625 .. 32.375), 33 x 40 (1.5 .. 31.5: halves round to even), 20 x 40 (too wide:
    padded) and 24 x 32, the no-op."""
    rgb, seg, depth, K = _frames(h, w, 2, h * w)
    ids = [[1, 2, 9, 7], [3, 0]]
    batch = A.ObservationBatch(rgb=dev(rgb), segmentation=dev(seg), depth=dev(depth), K=torch.from_numpy(K), object_ids=ids)
    T = A.CropResizeToAspectTransform((24, 32))
    out = T(batch, np.random.default_rng(0))
    if (h, w) == (24, 32):
        assert out is batch
        return
    out2 = T(batch, np.random.default_rng(1))
    assert same(out.rgb, out2.rgb) and same(out.segmentation, out2.segmentation) and same(out.depth, out2.depth)
    assert out.rgb.shape == (2, 24, 32, 3) and out.depth.dtype == torch.float32 and out.segmentation.dtype == torch.int32
    assert out.K.device == batch.K.device and out.K.dtype == torch.float32
    for b in range(2):
        r_rgb, r_seg, r_depth, r_K, dets = R.crop_resize_to_aspect(rgb[b], seg[b], depth[b], K[b], (24, 32), get_K_crop_resize)
        assert np.array_equal(out.rgb[b].cpu().numpy(), r_rgb)
        assert np.array_equal(out.segmentation[b].cpu().numpy(), r_seg)
        assert np.array_equal(out.depth[b].cpu().numpy().view(np.uint32), r_depth.view(np.uint32))
        assert np.array_equal(out.K[b].numpy(), r_K)
        for k, i in enumerate(ids[b]):
            assert bool(out.visible[b, k]) == (i in dets), (b, i)
            if i in dets:
                assert np.array_equal(out.boxes_modal[b, k].cpu().numpy(), dets[i]), (b, i)
        assert not out.visible[b, len(ids[b]):].any()


def test_replace_background_with_resize(golden):
    """A 37 x 53 background under 11 x 20 frames, and an 11 x 20 one under 37 x 53 frames: Pillow's default resize (the golden
    file's ``default`` arrays), then the existing paste."""
    for src, case in (("random_37x53", "37x53_to_11x20"), ("random_11x20", "11x20_to_37x53")):
        bg = golden[f"in|rgb|{src}"]
        want_bg = golden[f"rgb|{case}|default"]
        h, w = want_bg.shape[:2]
        rgb, seg, _, _ = _frames(h, w, 2, 5)
        batch = A.ObservationBatch(rgb=dev(rgb), segmentation=dev(seg), background=dev(np.stack([bg, bg[::-1]])))
        out = twice(lambda: A.ReplaceBackgroundTransform(resize_background=True)(batch, np.random.default_rng(0)).rgb).cpu().numpy()
        for b, flip in enumerate((False, True)):
            wb = want_bg if not flip else R.resize_rgb(np.ascontiguousarray(bg[::-1]), (h, w), R.BICUBIC)
            assert np.array_equal(out[b], np.where((seg[b] == 0)[..., None], wb, rgb[b]))
        with pytest.raises(ValueError, match="already"):
            A.ReplaceBackgroundTransform()(batch, np.random.default_rng(0))
