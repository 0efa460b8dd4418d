"""NumPy restatement of the three definitions behind ``happypose_amd.ops.resize_rgb`` / ``resize_nearest`` / ``seg_boxes`` and of
``CropResizeToAspectTransform``, written from Pillow's documented behaviour (``Image.resize(size, resample, box)``,
``Image.crop(box)``) and pinned to Pillow 12.2 by ``tests/golden/g15_resize.npz`` (test_resize_reference.py: 0 bytes differ).

Antialiased resample of an 8-bit image (BILINEAR: support 1, BICUBIC: support 2, a = -0.5), one axis at a time, columns first:
  scale = (box1 - box0) / out, fscale = max(scale, 1), support = filter support * fscale;
  for output index i: centre = box0 + (i + 0.5) scale, lo = max(int(centre - support + 0.5), 0),
  hi = min(int(centre + support + 0.5), in); weight of source j in [lo, hi) = filter((j - centre + 0.5) / fscale), normalised to sum 1,
  then rounded to 22 fractional bits: int(w 2^22 + 0.5) (- 0.5 below zero);  out = clip((sum w_j in_j + 2^21) >> 22, 0, 255).
  An axis whose size is unchanged and whose box is the whole axis is skipped.  The columns pass writes a uint8 intermediate.
NEAREST (modes I and F): source x of output i is int(t_i), t_0 = box0 + scale / 2, t_{i + 1} = t_i + scale: a running double sum.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

BILINEAR, BICUBIC = "bilinear", "bicubic"
PRECISION_BITS = 32 - 8 - 2


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {BILINEAR: (_bilinear, 1.0), BICUBIC: (_bicubic, 2.0)}


def coefficients(in_size: int, box0: float, box1: float, out_size: int, filt: str) -> List[Tuple[int, List[int]]]:
    """Per output index: (first source index, integer weights)."""
    fn, support = FILTERS[filt]
    scale = (box1 - box0) / out_size
    fscale = max(scale, 1.0)
    support = support * fscale
    rows = []
    for i in range(out_size):
        centre = box0 + (i + 0.5) * scale
        lo = max(int(centre - support + 0.5), 0)
        hi = min(int(centre + support + 0.5), in_size)
        w = [fn((j - centre + 0.5) * (1.0 / fscale)) for j in range(lo, hi)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        q = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
        rows.append((lo, q))
    return rows


def _pass(img: np.ndarray, coeffs, axis: int) -> np.ndarray:
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(coeffs),) + src.shape[1:], np.uint8)
    for i, (lo, q) in enumerate(coeffs):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for k, wk in enumerate(q):
            acc += src[lo + k] * wk
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_rgb(img: np.ndarray, out_hw: Tuple[int, int], filt: str, box: Optional[Sequence[int]] = None) -> np.ndarray:
    """``img [h, w, 3]`` uint8 -> ``[oh, ow, 3]``; ``box = (x0, y0, x1, y1)`` in source pixels (default: everything)."""
    h, w = img.shape[:2]
    oh, ow = out_hw
    x0, y0, x1, y1 = (0, 0, w, h) if box is None else box
    if ow != w or x0 != 0 or x1 != w:
        img = _pass(img, coefficients(w, x0, x1, ow, filt), 1)
    if oh != h or y0 != 0 or y1 != h:
        img = _pass(img, coefficients(h, y0, y1, oh, filt), 0)
    return np.ascontiguousarray(img)


def nearest_index(in_size: int, box0: float, box1: float, out_size: int) -> np.ndarray:
    """Source index per output index, -1 = outside the image (the pixel stays 0)."""
    step = (box1 - box0) / out_size
    t = box0 + step * 0.5
    idx = np.empty(out_size, np.int64)
    for i in range(out_size):
        j = -1 if t < 0.0 else int(t)
        idx[i] = j if 0 <= j < in_size else -1
        t += step
    return idx


def resize_nearest(img: np.ndarray, out_hw: Tuple[int, int], box: Optional[Sequence[int]] = None) -> np.ndarray:
    """``img [h, w]`` of a 4-byte type: a copy of bits, whatever they mean."""
    h, w = img.shape
    oh, ow = out_hw
    x0, y0, x1, y1 = (0, 0, w, h) if box is None else box
    xi, yi = nearest_index(w, x0, x1, ow), nearest_index(h, y0, y1, oh)
    bits = img.view(np.uint32)
    out = bits[np.clip(yi, 0, None)][:, np.clip(xi, 0, None)].copy()
    out[yi < 0, :] = 0
    out[:, xi < 0] = 0
    return out.view(img.dtype)


def seg_boxes(seg: np.ndarray, ids: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """``(boxes [n, 4] (x1, y1, x2, y2) inclusive, n_px [n])`` of ``ids`` in ``seg [h, w]``; an absent id has n_px 0 and box 0."""
    boxes, n_px = np.zeros((len(ids), 4), np.int32), np.zeros(len(ids), np.int32)
    for k, i in enumerate(ids):
        rows, cols = np.nonzero(seg == i)
        n_px[k] = rows.size
        if rows.size:
            boxes[k] = cols.min(), rows.min(), cols.max(), rows.max()
    return boxes, n_px


def detections_from_segmentation(seg: np.ndarray) -> Dict[int, np.ndarray]:
    """The reference's ``make_detections_from_segmentation`` for one image, step by step: every value of the map, background
    included, with the inclusive min / max of its columns and rows."""
    dets = {}
    for unique_id in np.unique(seg):
        where = np.where(seg == unique_id)
        dets[int(unique_id)] = np.array([np.min(where[1]), np.min(where[0]), np.max(where[1]), np.max(where[0])])
    return dets


# ---- CropResizeToAspectTransform ----------------------------------------------------------------------------------------------------
def crop_pad(img: np.ndarray, rect: Sequence[int]) -> np.ndarray:
    """``Image.crop`` with an integer rectangle: pixels outside the image are 0."""
    x0, y0, x1, y1 = rect
    out = np.zeros((y1 - y0, x1 - x0) + img.shape[2:], img.dtype)
    h, w = img.shape[:2]
    sx0, sy0, sx1, sy1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
    if sx1 > sx0 and sy1 > sy0:
        out[sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = img[sy0:sy1, sx0:sx1]
    return out


def aspect_crop_box(h: int, w: int, resize: Tuple[int, int]) -> Optional[Tuple[float, float, float, float]]:
    """The float box the reference crops to (None: the aspect is already right)."""
    aspect = max(resize) / min(resize)
    if np.isclose(w / h, aspect):
        return None
    crop_h = w * 1 / aspect
    crop_h, crop_w = min(crop_h, w), max(crop_h, w)
    return (w / 2 - crop_w / 2, h / 2 - crop_h / 2, w / 2 + crop_w / 2, h / 2 + crop_h / 2)


def pil_round_box(box: Sequence[float]) -> Tuple[int, int, int, int]:
    """``Image.crop`` rounds each edge with Python's ``round``: halves go to the even integer."""
    return tuple(int(round(v)) for v in box)


def crop_resize_to_aspect(rgb, seg, depth, K, resize, get_K_crop_resize):
    """One frame through the reference's ``CropResizeToAspectTransform``; ``get_K_crop_resize`` is the oracle's restatement.
    Returns ``(rgb, seg, depth, K, detections)``."""
    assert resize[1] >= resize[0]
    h, w = rgb.shape[:2]
    if (h, w) == tuple(resize):
        return rgb, seg, depth, K, None
    K = np.asarray(K, np.float32)
    box = aspect_crop_box(h, w, resize)
    if box is not None:
        rect = pil_round_box(box)
        rgb, seg = crop_pad(rgb, rect), crop_pad(seg, rect)
        depth = None if depth is None else crop_pad(depth, rect)
        crop_h, crop_w = box[3] - box[1], box[2] - box[0]
        K = get_K_crop_resize(K[None], np.array([box], np.float32), (h, w), (min(crop_h, crop_w), max(crop_h, crop_w)))[0]
    h, w = rgb.shape[:2]
    out_hw = (min(resize), max(resize))
    rgb = resize_rgb(rgb, out_hw, BILINEAR)
    seg = resize_nearest(seg, out_hw)
    depth = None if depth is None else resize_nearest(depth, out_hw)
    K = get_K_crop_resize(K[None], np.array([[0, 0, w, h]], np.float32), (h, w), out_hw)[0]
    return rgb, seg, depth, K, detections_from_segmentation(seg)


# ---- the cases of tests/golden/g15_resize.npz (tools/gen_golden_resize.py records Pillow on them) ---------------------------------------
# name -> (input, (out_h, out_w), box (x0, y0, x1, y1) or None, crop rectangle applied first (Image.crop) or None)
GOLDEN_CASES = {
    "1x1_to_3x2": ("random_1x1", (3, 2), None, None),
    "2x9_to_9x2": ("random_2x9", (9, 2), None, None),
    "13x17_same": ("random_13x17", (13, 17), None, None),
    "13x17_to_13x40": ("random_13x17", (13, 40), None, None),
    "13x17_to_29x17": ("random_13x17", (29, 17), None, None),
    "13x17_same_box": ("random_13x17", (13, 17), (2, 1, 15, 12), None),
    "37x53_to_11x20": ("random_37x53", (11, 20), None, None),
    "37x53_to_11x20_box": ("random_37x53", (11, 20), (5, 3, 45, 30), None),
    "11x20_to_37x53": ("random_11x20", (37, 53), None, None),
    "11x20_to_37x53_box": ("random_11x20", (37, 53), (3, 2, 17, 9), None),
    "40x33_aspect": ("random_40x33", (24, 32), None, (0, 8, 33, 32)),
    "33x40_aspect": ("random_33x40", (24, 32), None, (0, 2, 40, 32)),       # box edges 1.5 and 31.5: halves go to even
    "20x40_aspect_pad": ("random_20x40", (24, 32), None, (0, -5, 40, 25)),  # too wide: the crop pads with zeros
    "5x1031_to_3x64": ("random_5x1031", (3, 64), None, None),
    "zeros_37x53_to_11x20": ("zeros_37x53", (11, 20), None, None),
    "ones_37x53_to_11x20": ("ones_37x53", (11, 20), None, None),
    "checker_37x53_to_11x20": ("checker_37x53", (11, 20), None, None),
    "checker_11x20_to_37x53": ("checker_11x20", (37, 53), None, None),
    "checker2_11x20_to_37x53": ("checker2_11x20", (37, 53), None, None),
}
GOLDEN_FILTERS = (BILINEAR, BICUBIC)


def golden_inputs() -> Dict[str, Dict[str, np.ndarray]]:
    """``{"rgb" | "i32" | "f32": {input name: array}}``: seeded; every depth map with room has a NaN and a negative pixel, every
    id map an id of one pixel, a negative id and 2^31 - 1."""
    rng = np.random.default_rng(15)
    rgb, i32, f32 = {}, {}, {}
    for name in sorted({c[0] for c in GOLDEN_CASES.values()}):
        kind, size = name.split("_")
        h, w = (int(v) for v in size.split("x"))
        if kind == "random":
            x = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        elif kind == "zeros":
            x = np.zeros((h, w, 3), np.uint8)
        elif kind == "ones":
            x = np.full((h, w, 3), 255, np.uint8)
        else:  # checker: cells of 1 pixel; checker2: cells of 2 pixels (overshoot survives the upscale)
            c = 1 if kind == "checker" else 2
            yy, xx = np.meshgrid(np.arange(h) // c, np.arange(w) // c, indexing="ij")
            x = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
        rgb[name] = x
        if kind != "random":
            continue
        s = rng.integers(0, 6, (h, w)).astype(np.int32)
        d = rng.uniform(0.2, 3.0, (h, w)).astype(np.float32)
        d[rng.random((h, w)) < 0.2] = 0
        if h * w >= 6:
            flat = rng.permutation(h * w)[:5]
            s.reshape(-1)[flat[0]], s.reshape(-1)[flat[1]], s.reshape(-1)[flat[2]] = 77, -7, 2 ** 31 - 1
            d.reshape(-1)[flat[3]], d.reshape(-1)[flat[4]] = np.nan, -1.5
        i32[name], f32[name] = s, d
    return {"rgb": rgb, "i32": i32, "f32": f32}
