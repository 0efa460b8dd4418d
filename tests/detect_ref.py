"""Reference of the detector's stages that are not convolutions (csrc/detect.hip and the two pre-processing kernels of
csrc/pool_head.hip), written from include/happypose_amd.h and the torchvision 0.14.1 rules it cites -- anchor_utils.py, _utils.py
(BoxCoder), rpn.py (filter_proposals), ops/boxes.py (nms, batched_nms), ops/poolers.py (LevelMapper, MultiScaleRoIAlign),
ops/csrc/cpu/roi_align_common.h, roi_heads.py (postprocess_detections, maskrcnn_inference, paste_masks_in_image), transform.py --
in float64 NumPy on the CPU.  ``ref_name`` restates entry point ``hp_name``.  Nothing here is translated from a kernel and nothing
needs torch.

The inputs are float32 arrays and therefore exact; every operation on them is float64.  Two constants belong to the DEFINITION as
float32 values, because torchvision applies them to float32 tensors: the ``log(1000 / 16)`` clamp of BoxCoder.decode and the
``1e-6`` of LevelMapper.

Every discrete decision comes back with its float64 MARGIN, the distance of the deciding quantity from its threshold: the small-box
flag (``valid_margin``, px), IoU against the NMS threshold (``margin``), the level floor (``level_margin``), the validity of a
sample at ``-1`` and at the map's size (``sample_margin``, feature px), the truncation of the expanded mask box (``trunc_margin``,
px) and the clamps (``clamp_margin``).  The GPU tests leave a decision out of the comparison when its margin is below the band of
tests/detect_yardstick.py; the tables at the end of this file are chosen so that no decision is, except in the cases marked
``exact``, whose float32 evaluation is exact step by step (each says why).  The clamps are minima and maxima: continuous, so a clamp
that falls the other way moves the output by no more than its own margin and never makes an output fragile; their margins prove
that the "clamped" cases reach the clamp.  The same holds for the truncations inside the bilinear interpolations."""

import functools
from types import SimpleNamespace

import numpy as np

F = np.float32
D = np.float64
XFORM_CLIP = float(F(np.log(1000.0 / 16.0)))  # BoxCoder.bbox_xform_clip, applied to a float32 tensor
LEVEL_EPS = float(F(1e-6))                    # LevelMapper.eps as a float32 tensor
ASPECT_RATIOS = (0.5, 1.0, 2.0)
ANCHOR_SCALES = (32, 64, 128, 256, 512)
IMAGE_MEAN = (0.485, 0.456, 0.406)
IMAGE_STD = (0.229, 0.224, 0.225)


def base_anchors(size):
    """AnchorGenerator.generate_anchors for one scale and the ratios (0.5, 1, 2): float32 ``[3, 4]``.  torchvision forms them in
    float32 and rounds half to even; the rounding is part of the definition."""
    hr = np.sqrt(np.asarray(ASPECT_RATIOS, F))
    wr = (F(1) / hr).astype(F)
    ws, hs = (wr * F(size)).astype(F), (hr * F(size)).astype(F)
    return np.round(np.stack([-ws, -hs, ws, hs], 1) / F(2)).astype(F)


def _sigmoid(x):
    x = np.asarray(x, D)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _decode(boxes, deltas, weights):
    """BoxCoder.decode_single on ``boxes [..., 4]`` and ``deltas [..., 4]`` -> ``(decoded [..., 4], clamp_margin [..., 2], wh [..., 2])``;
    clamp_margin = ``delta / weight - clip`` (positive: the clamp is active), wh = the decoded width and height."""
    boxes, deltas = np.asarray(boxes, D), np.asarray(deltas, D)
    wx, wy, ww, wh = weights
    w, h = boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]
    cx, cy = boxes[..., 0] + 0.5 * w, boxes[..., 1] + 0.5 * h
    dx, dy, dw, dh = deltas[..., 0] / wx, deltas[..., 1] / wy, deltas[..., 2] / ww, deltas[..., 3] / wh
    margin = np.stack([dw - XFORM_CLIP, dh - XFORM_CLIP], -1)
    dw, dh = np.minimum(dw, XFORM_CLIP), np.minimum(dh, XFORM_CLIP)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = np.exp(dw) * w, np.exp(dh) * h
    out = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], -1)
    return out, margin, np.stack([pw, ph], -1)


def _clip(boxes, im_h, im_w):
    b = np.array(boxes, D)
    b[..., 0::2] = np.clip(b[..., 0::2], 0.0, float(im_w))
    b[..., 1::2] = np.clip(b[..., 1::2], 0.0, float(im_h))
    return b


def grid_anchors(anchor_idx, map_w, n_anchors, h_base_anchors, stride_h, stride_w):
    """AnchorGenerator.grid_anchors for the selected anchors: index = (y * map_w + x) * n_anchors + a -> float64 ``[n, 4]``."""
    idx = np.asarray(anchor_idx, np.int64)
    a, pos = idx % n_anchors, idx // n_anchors
    y, x = pos // map_w, pos % map_w
    shift = np.stack([x * stride_w, y * stride_h, x * stride_w, y * stride_h], 1).astype(D)
    return shift + np.asarray(h_base_anchors, D).reshape(n_anchors, 4)[a], pos, a


def ref_rpn_decode(objectness, anchor_idx, deltas_map, map_w, n_anchors, h_base_anchors, stride_h, stride_w, im_h, im_w, min_size):
    """``deltas_map [h][map_w][4 n_anchors]`` of one image -> ``dict(boxes [n,4], scores [n], valid [n], valid_margin [n],
    clamp_margin [n,2], anchors [n,4], wh [n,2])``.  valid_margin: the smaller of ``|w - min_size|`` and ``|h - min_size|``."""
    anchors, pos, a = grid_anchors(anchor_idx, map_w, n_anchors, h_base_anchors, stride_h, stride_w)
    d = np.asarray(deltas_map, D).reshape(-1, n_anchors, 4)[pos, a]
    dec, clamp_margin, wh = _decode(anchors, d, (1.0, 1.0, 1.0, 1.0))
    boxes = _clip(dec, im_h, im_w)
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    ms = float(min_size)
    return dict(boxes=boxes, scores=_sigmoid(objectness), valid=(w >= ms) & (h >= ms),
                valid_margin=np.minimum(np.abs(w - ms), np.abs(h - ms)), clamp_margin=clamp_margin, anchors=anchors, wh=wh, raw=dec)


def pair_iou(boxes):
    """float64 IoU of every pair, ``0 / 0`` (two boxes without area) = NaN, which is not above any threshold."""
    b = np.asarray(boxes, D)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.maximum(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), 0.0)
    ih = np.maximum(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), 0.0)
    inter = iw * ih
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area[:, None] + area[None, :] - inter)


def ref_nms(boxes, group, iou_threshold):
    """Greedy suppression inside each group, the boxes in their order (decreasing score): ``dict(keep [n] bool in input order,
    iou [n,n], margin [n,n])``; margin = ``|IoU - threshold|`` of the pairs of one group, inf elsewhere and where IoU is NaN."""
    group = np.asarray(group)
    n = len(group)
    iou = pair_iou(boxes)
    thr = float(F(iou_threshold))
    same = group[:, None] == group[None, :]
    with np.errstate(invalid="ignore"):
        over = same & (iou > thr)
    keep = np.ones(n, bool)
    for i in range(n):
        if keep[i]:
            keep[i + 1:] &= ~over[i, i + 1:]
    margin = np.where(same & ~np.isnan(iou) & ~np.eye(n, dtype=bool), np.abs(iou - thr), np.inf)
    return dict(keep=keep, iou=iou, margin=margin)


def map_level(rois, k_min, n_levels):
    """LevelMapper: ``(level index [K], level_margin [K], v [K])``, v = ``4 + log2(sqrt(area) / 224) + eps`` before the floor;
    the margin is the distance of v from the nearest integer that separates two levels of the pyramid."""
    r = np.asarray(rois, D)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = 4.0 + np.log2(np.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])) / 224.0) + LEVEL_EPS
    lv = np.clip(np.floor(v), k_min, k_min + n_levels - 1)
    lv = np.where(np.isnan(lv), k_min, lv).astype(np.int64) - k_min  # torch.clamp of NaN stays NaN; no case has a negative area
    cuts = np.arange(k_min + 1, k_min + n_levels, dtype=D)
    margin = np.abs(v[:, None] - cuts[None, :]).min(1) if len(cuts) else np.full(len(r), np.inf)
    return lv, margin, v


def _axis(start, bin_size, n, size, g):
    """Samples of one axis, roi_align with aligned=False: coordinates ``[n, g]``, validity (outside ``[-1, size]`` a sample is 0),
    its margin, the two neighbours and the upper weight (bilinear_interpolate of roi_align_common.h)."""
    p, s = np.arange(n, dtype=D)[:, None], np.arange(g, dtype=D)[None, :]
    y = start + p * bin_size + (s + 0.5) * bin_size / g
    valid = ~((y < -1.0) | (y > size))
    margin = np.minimum(np.abs(y + 1.0), np.abs(y - size))
    yc = np.maximum(y, 0.0)
    lo = np.floor(yc).astype(np.int64)
    top = lo >= size - 1
    lo = np.where(top, size - 1, lo)
    hi = np.where(top, size - 1, lo + 1)
    yc = np.where(top, lo.astype(D), yc)
    return y, valid, margin, lo, hi, yc - lo


def ref_roi_align_levels(maps, scales, k_min, rois, out_size, sampling_ratio):
    """``maps``: per level NHWC ``[n_img][h][w][C]``; ``rois [K][5]`` = image index, x1, y1, x2, y2 in image coordinates ->
    ``dict(values [K][out][out][C], levels [K], level_margin [K], sample_margin [K][out][out], size_margin [K][2], coords)``.
    sample_margin: the least distance of a sample of the bin from ``-1`` or the map's size, along either axis; size_margin: the
    roi's width and height on the map minus 1 (negative: the ``max(., 1)`` of aligned=False is active)."""
    rois = np.asarray(rois, D)
    K, C, g = len(rois), maps[0].shape[-1], int(sampling_ratio)
    levels, level_margin, v = map_level(rois, k_min, len(maps))
    values = np.zeros((K, out_size, out_size, C), D)
    sample_margin = np.zeros((K, out_size, out_size), D)
    size_margin = np.zeros((K, 2), D)
    coords = []
    for k in range(K):
        f = np.asarray(maps[levels[k]][int(rois[k, 0])], D)
        H, W = f.shape[:2]
        sc = float(scales[levels[k]])
        x1, y1, x2, y2 = rois[k, 1:] * sc
        size_margin[k] = (x2 - x1 - 1.0, y2 - y1 - 1.0)
        rw, rh = max(x2 - x1, 1.0), max(y2 - y1, 1.0)
        ys, vy, my, ylo, yhi, ly = _axis(y1, rh / out_size, out_size, H, g)
        xs, vx, mx, xlo, xhi, lx = _axis(x1, rw / out_size, out_size, W, g)
        coords.append((ys, xs, H, W))
        sample_margin[k] = np.minimum(my.min(1)[:, None], mx.min(1)[None, :])
        acc = np.zeros((out_size, out_size, C), D)
        for iy in range(g):
            for ix in range(g):
                ok = (vy[:, iy][:, None] & vx[:, ix][None, :])[..., None]
                a, b = (1.0 - ly[:, iy])[:, None, None], ly[:, iy][:, None, None]
                c, d = (1.0 - lx[:, ix])[None, :, None], lx[:, ix][None, :, None]
                yl, yh, xl, xh = ylo[:, iy][:, None], yhi[:, iy][:, None], xlo[:, ix][None, :], xhi[:, ix][None, :]
                acc += np.where(ok, a * c * f[yl, xl] + a * d * f[yl, xh] + b * c * f[yh, xl] + b * d * f[yh, xh], 0.0)
        values[k] = acc / (g * g)
    return dict(values=values, levels=levels, level_margin=level_margin, sample_margin=sample_margin, size_margin=size_margin,
                coords=coords, v=v)


def ref_box_postprocess(class_logits, ld_logits, box_regression, ld_regression, proposals, n, n_classes, im_h, im_w):
    """Rows of ``ld_logits`` / ``ld_regression`` floats, of which the first ``n_classes`` / ``4 n_classes`` count ->
    ``dict(scores [n][n_classes], boxes [n][n_classes][4], clamp_margin [n][n_classes][2], wh)``."""
    lg = np.asarray(class_logits, F).reshape(n, ld_logits)[:, :n_classes].astype(D)
    rg = np.asarray(box_regression, F).reshape(n, ld_regression)[:, :4 * n_classes].astype(D).reshape(n, n_classes, 4)
    e = np.exp(lg - lg.max(1, keepdims=True))
    dec, clamp_margin, wh = _decode(np.asarray(proposals, D).reshape(n, 1, 4), rg, (10.0, 10.0, 5.0, 5.0))
    return dict(scores=e / e.sum(1, keepdims=True), boxes=_clip(dec, im_h, im_w), clamp_margin=clamp_margin, wh=wh, raw=dec)


def _trunc_margin(v):
    """Distance of ``v`` from the nearest value at which the conversion to an integer (towards zero) changes: the integers but 0."""
    v = np.asarray(v, D)
    near = np.where(np.abs(v) < 1.0, 1.0 - np.abs(v), np.minimum(v - np.floor(v), np.ceil(v) - v))
    return np.where((np.abs(v) >= 1.0) & (v == np.round(v)), 0.0, near)


def expand_boxes(boxes, M=28, padding=1):
    """expand_boxes of roi_heads.py with scale (M + 2 padding) / M -> float64 corners ``[n, 4]`` before ``.to(int64)``."""
    b = np.asarray(boxes, D)
    scale = float(M + 2 * padding) / M
    wh, hh = (b[:, 2] - b[:, 0]) * 0.5 * scale, (b[:, 3] - b[:, 1]) * 0.5 * scale
    xc, yc = (b[:, 2] + b[:, 0]) * 0.5, (b[:, 3] + b[:, 1]) * 0.5
    return np.stack([xc - wh, yc - hh, xc + wh, yc + hh], 1)


def _resize_axis(n_out, n_in):
    """F.interpolate(bilinear, align_corners=False) along one axis: ``(lo, hi, upper weight)`` per output index."""
    src = np.maximum((n_in / n_out) * (np.arange(n_out, dtype=D) + 0.5) - 0.5, 0.0)
    lo = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    hi = np.minimum(lo + 1, n_in - 1)
    return lo, hi, src - lo


def ref_paste_masks(mask_logits, ld, labels, boxes, n, H, W):
    """``mask_logits [n][14][14][2][2][ld]``: element ``(k, i, j, a, b, c)`` is the logit of class c at row ``2 i + a`` and column
    ``2 j + b`` of the 28 x 28 mask of detection k -> ``dict(masks [n][H][W], rect [n][4] = x0, x1, y0, y1 of the pasted rectangle,
    trunc_margin [n], corners [n][4])``; outside the rectangle the mask is 0."""
    ml = np.asarray(mask_logits, F).reshape(n, 14, 14, 2, 2, ld)
    M, P = 28, 1
    corners = expand_boxes(boxes, M, P)
    be = np.trunc(corners).astype(np.int64)
    out = np.zeros((n, H, W), D)
    rect = np.zeros((n, 4), np.int64)
    for k in range(n):
        plane = np.zeros((M, M), D)
        for py in range(M):
            for px in range(M):
                plane[py, px] = ml[k, py // 2, px // 2, py % 2, px % 2, int(labels[k])]
        padded = np.zeros((M + 2 * P, M + 2 * P), D)
        padded[P:-P, P:-P] = _sigmoid(plane)
        w, h = max(int(be[k, 2] - be[k, 0] + 1), 1), max(int(be[k, 3] - be[k, 1] + 1), 1)
        ylo, yhi, ly = _resize_axis(h, M + 2 * P)
        xlo, xhi, lx = _resize_axis(w, M + 2 * P)
        ly, lx = ly[:, None], lx[None, :]
        mm = (1 - ly) * ((1 - lx) * padded[ylo][:, xlo] + lx * padded[ylo][:, xhi]) + ly * ((1 - lx) * padded[yhi][:, xlo] + lx * padded[yhi][:, xhi])
        x0, x1, y0, y1 = max(int(be[k, 0]), 0), min(int(be[k, 2]) + 1, W), max(int(be[k, 1]), 0), min(int(be[k, 3]) + 1, H)
        rect[k] = (x0, x1, y0, y1)
        if y1 > y0 and x1 > x0:
            out[k, y0:y1, x0:x1] = mm[y0 - be[k, 1]:y1 - be[k, 1], x0 - be[k, 0]:x1 - be[k, 0]]
    return dict(masks=out, rect=rect, trunc_margin=_trunc_margin(corners).min(1), corners=corners)


def ref_preprocess(images, mean3, std3):
    """GeneralizedRCNNTransform.normalize + NCHW ``[n][3][h][w]`` -> NHWC ``[n][h][w][4]``, channel 3 zero."""
    x = np.asarray(images, D)
    m, s = np.asarray(mean3, F).astype(D), np.asarray(std3, F).astype(D)
    out = np.zeros(x.shape[:1] + x.shape[2:] + (4,), D)
    out[..., :3] = ((x - m[None, :, None, None]) / s[None, :, None, None]).transpose(0, 2, 3, 1)
    return out


def ref_preprocess_resize(images, h_out, w_out, h_pad, w_pad, mean3, std3):
    """The same behind a bilinear resize (align_corners=False, scale = input / output size) to ``[h_out][w_out]`` in the top-left
    corner of a zero canvas ``[n][h_pad][w_pad][4]``.  The kernel interpolates first and normalises after; so does this."""
    x = np.asarray(images, D)
    n, _, hi, wi = x.shape
    ylo, yhi, ly = _resize_axis(h_out, hi)
    xlo, xhi, lx = _resize_axis(w_out, wi)
    ly, lx = ly[:, None], lx[None, :]
    r = (1 - ly) * ((1 - lx) * x[:, :, ylo][..., xlo] + lx * x[:, :, ylo][..., xhi]) + ly * ((1 - lx) * x[:, :, yhi][..., xlo] + lx * x[:, :, yhi][..., xhi])
    out = np.zeros((n, h_pad, w_pad, 4), D)
    out[:, :h_out, :w_out] = ref_preprocess(r, mean3, std3)
    return out


# ================================================================================================================ the case tables
# Shared by tests/test_detect_reference.py (CPU) and tests/test_gpu_detect_stages.py.  Everything is generated from seeds.
def interleave_masks(nchw, ld, fill=np.nan):
    """``[n][C][28][28]`` -> the mask head's ``[n][14][14][2][2][ld]``; the channels past C hold ``fill``."""
    n, C = nchw.shape[:2]
    out = np.full((n, 14, 14, 2, 2, ld), fill, F)
    out[..., :C] = np.asarray(nchw, F).reshape(n, C, 14, 2, 14, 2).transpose(0, 2, 4, 3, 5, 1)
    return out


# ---- hp_rpn_decode: a 5 x 7 map with strides 16 (rows) and 8 (columns) under a 75 x 50 image, so that neither the map nor the
# strides survive a swap of x and y, and the image is smaller than the 80 x 56 canvas: every box near the far sides is clipped
RPN_IMAGE = (75.0, 50.0)
RPN_OBJECTNESS = np.array([-100, -1, 0, 1, 100], F)
RPN_GROUPS = ("benign", "clamped", "collapsed", "off_side", "single", "two_blocks")


def rpn_case(group, scale):
    """One call of hp_rpn_decode as a namespace: ``name, gh, gw, stride_h, stride_w, im_h, im_w, base, idx, obj, deltas, min_size,
    exact``."""
    rs = np.random.RandomState(100 * (RPN_GROUPS.index(group) if group in RPN_GROUPS else 0) + ANCHOR_SCALES.index(scale))
    gh, gw = (9, 10) if group == "two_blocks" else (5, 7)
    n_all = gh * gw * 3
    deltas = np.concatenate([rs.normal(0, 0.3, (gh, gw, 3, 2)), rs.normal(0, 0.4, (gh, gw, 3, 2))], -1).astype(F)
    idx = rs.permutation(n_all).astype(np.int32)
    # min_size: the product passes 1e-3; 0.25 here, because the band of the flag grows with the decoded size (1e-3 px at 1700 px)
    # and a box clipped to no width at all, 1e-3 under the product's threshold, would count as fragile
    min_size, exact = F(0.25), False
    if group == "clamped":  # dw, dh over the clamp, at it (the float32 nearest log(1000 / 16)), and just under: nothing overflows
        vals = np.array([4.0, F(np.log(1000.0 / 16.0)), 5.0, 50.0], F)
        pick = np.arange(gh * gw * 3).reshape(gh, gw, 3)
        deltas[..., 2], deltas[..., 3] = vals[pick % 4], vals[(pick // 4) % 4]
    elif group == "collapsed":  # exp(-20) of the anchor: a width (or height) of 1e-7 px, under min_size
        pick = np.arange(gh * gw * 3).reshape(gh, gw, 3)
        deltas[..., 2] = np.where(pick % 2 == 0, -20.0, deltas[..., 2])
        deltas[..., 3] = np.where(pick % 2 == 1, -20.0, deltas[..., 3])
    elif group == "off_side":  # six anchor sizes to the left, right, top, bottom: beyond the image from every position
        pick = np.arange(gh * gw * 3).reshape(gh, gw, 3) % 4
        deltas[..., 2:] *= 0.25
        deltas[..., 0] = np.where(pick == 0, -6.0, np.where(pick == 1, 6.0, deltas[..., 0]))
        deltas[..., 1] = np.where(pick == 2, -6.0, np.where(pick == 3, 6.0, deltas[..., 1]))
    elif group == "single":
        idx = idx[:1]
    elif group == "two_blocks":
        idx = idx[:257]
    elif group.startswith("exact"):
        # zero deltas return the anchor, clipped: every coordinate is an integer below 2^24 and expf(0) = 1, so the float32
        # evaluation is exact step by step.  The 46 x 22 anchor fits the image at x = 3, y = 1..3: its height is 22
        assert scale == 32
        deltas[:] = 0
        min_size, exact = (F(22.0) if group == "exact_at" else np.nextafter(F(22.0), F(np.inf))), True
    else:
        assert group == "benign"
    obj = np.concatenate([RPN_OBJECTNESS, rs.normal(0, 3, max(len(idx) - 5, 0)).astype(F)])[:len(idx)]
    return SimpleNamespace(name=f"{group}-{scale}", group=group, scale=scale, gh=gh, gw=gw, stride_h=16, stride_w=8, im_h=RPN_IMAGE[0],
                           im_w=RPN_IMAGE[1], base=base_anchors(scale), idx=idx, obj=obj, deltas=deltas.reshape(gh, gw, 12),
                           min_size=min_size, exact=exact)


RPN_CASES = [(g, s) for s in ANCHOR_SCALES for g in RPN_GROUPS] + [("exact_at", 32), ("exact_above", 32)]


def rpn_ref(case):
    return ref_rpn_decode(case.obj, case.idx, case.deltas, case.gw, 3, case.base, case.stride_h, case.stride_w, case.im_h, case.im_w,
                          case.min_size)


# ---- hp_nms: coordinates on a grid of 1/4 px below 2^10, so that the areas, the intersection and the union are exact in float32
# and the one rounding is that of the quotient: float32 IoU = the float64 IoU rounded, and it lies on the same side of a float32
# threshold unless the float64 IoU is within half an ulp of it
def _filler(n, rs):
    """n disjoint boxes of about 10 px on a 20-px lattice from (200, 200): they suppress nothing."""
    k = np.arange(n)
    x, y = 200.0 + 20.0 * (k % 16), 200.0 + 20.0 * (k // 16)
    wh = rs.randint(20, 60, (n, 2)) / 4.0
    return np.stack([x, y, x + wh[:, 0], y + wh[:, 1]], 1)


def nms_case(name):
    """``name, boxes [n,4] float32, group [n] int32, thr float32, exact``.  Three groups interleaved wherever n allows."""
    rs = np.random.RandomState(sum(map(ord, name)))
    thr, exact, expect = F(0.5), False, {}
    if name.startswith("cloud"):
        n = int(name[5:])
        ctr, wh = rs.randint(80, 400, (n, 2)) / 4.0, rs.randint(40, 240, (n, 2)) / 4.0
        boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1)
        boxes = np.round(boxes * 4) / 4
        group = np.arange(n) % 3
    else:
        n = 130
        boxes, group = _filler(n, rs), np.arange(n) % 3
        if name in ("iou_half", "iou_half_below"):
            # [0,0,4,2] inside [0,0,4,4]: intersection 8, union 16, IoU = 0.5 in either format.  Not above 0.5: both stay; above
            # the float32 just below 0.5: the second goes.  Exact: powers of two all the way
            boxes[3], boxes[6], exact = (0, 0, 4, 2), (0, 0, 4, 4), True
            boxes[4] = (0, 0, 4, 4)  # the same box in another group: untouched
            if name == "iou_half_below":
                thr = np.nextafter(F(0.5), F(0))
            expect = {3: True, 6: name == "iou_half", 4: True}
        elif name == "identical":
            boxes[0] = boxes[3] = boxes[66] = boxes[129] = boxes[1] = (10, 10, 30.25, 25.5)  # 0, 3, 66, 129: group 0; 1: group 1
            expect = {0: True, 3: False, 66: False, 129: False, 1: True}
        elif name == "zero_area":
            # 0 / 0 between two of them and 0 / area against the box round them: kept, and they suppress nothing
            boxes[0], boxes[3], boxes[6], boxes[9], boxes[69] = (5, 5, 5, 9), (5, 5, 5, 9), (0, 0, 20, 20), (7, 7, 7, 7), (5, 6, 9, 6)
            expect = {0: True, 3: True, 6: True, 9: True, 69: True}
        elif name == "cross_word":
            boxes[0], boxes[129] = (10, 10, 30, 30), (10.25, 10, 30, 30.5)  # both group 0 (129 = 3 * 43), words 0 and 2
            expect = {0: True, 129: False}
        elif name == "chain":
            # A (3) removes B (66), B would remove C (129), A does not reach C: C stays because B is gone.  Words 0, 1, 2
            boxes[3], boxes[66], boxes[129] = (0, 0, 8, 8), (2, 0, 10, 8), (4, 0, 12, 8)
            expect = {3: True, 66: False, 129: True}
        else:
            raise KeyError(name)
    return SimpleNamespace(name=name, boxes=boxes.astype(F), group=group.astype(np.int32), thr=thr, exact=exact, expect=expect)


NMS_CASES = ["cloud1", "cloud63", "cloud64", "cloud65", "cloud130", "iou_half", "iou_half_below", "identical", "zero_area", "cross_word",
             "chain"]


# ---- hp_roi_align_levels: two images of 64 x 96, four levels at 1/4 .. 1/32, k_min = 2
ROI_IMAGE = (64, 96)
ROI_SHAPES = ((16, 24), (8, 12), (4, 6), (2, 3))
ROI_SCALES = (0.25, 0.125, 0.0625, 0.03125)
# name, image, x1, y1, x2, y2.  Boxes of 224 px do not fit the image: the level rule is exercised with rois that reach beyond
# it, which the validity rule of the samples handles and the reference defines
ROIS = [
    ("level0", 1, 5.5, 3.3, 85.4, 63.1),              # sqrt(area) 69
    ("level1", 0, -20.6, -40.3, 110.2, 130.5),        # 149
    ("level2", 1, -100.7, -120.3, 180.2, 200.4),      # 300
    ("level3", 0, -250.2, -280.6, 330.4, 350.1),      # 605
    ("below_clamp", 1, 10.3, 8.2, 50.7, 40.9),        # 36: v = 1.4, under k_min
    ("above_clamp", 1, -1000.3, -900.1, 1100.6, 1200.2),  # 2100: v = 7.2, over k_min + 3
    ("zero_area", 0, 20.3, 30.1, 20.3, 50.6),         # log2(0) = -inf -> level 0; no width: the max(., 1) clamp
    # the exact octaves: w = h = 112, 224, 448, so the product, its root, the quotient by 224 and log2 of 1/2, 1, 2 are exact in
    # float32 and v = 3, 4, 5 + 1e-6, which 4 ulp(3) = 9.5e-7 does not swallow: the floor is 3, 4, 5 in either format
    ("octave_112", 0, -30.5, -21.5, 81.5, 90.5),
    ("octave_224", 1, -60.5, -70.5, 163.5, 153.5),
    ("octave_448", 0, -200.5, -190.5, 247.5, 257.5),
    ("narrow", 1, 40.2, 10.1, 41.9, 50.3),            # 0.43 feature px wide: rw < 1
    ("x1_negative", 0, -6.6, 4.1, 30.3, 44.6),        # samples under -1 and in (-1, 0)
    ("past_far_edge", 1, 60.5, 40.3, 130.6, 90.7),    # samples in (W - 1, W), (H - 1, H) and beyond
]
ROI_EXACT = ("octave_112", "octave_224", "octave_448")
ROI_CONFIGS = [(8, o, g) for o in (1, 7, 14) for g in (1, 2, 3)] + [(256, 7, 2), (256, 14, 2), (256, 1, 3)]


@functools.lru_cache(maxsize=None)
def roi_maps(C, shapes=ROI_SHAPES):
    """Per level ``[2][h][w][C]`` float32: the two images differ."""
    rs = np.random.RandomState(C)
    maps = [rs.normal(0, 1 + l, (2, h, w, C)).astype(F) for l, (h, w) in enumerate(shapes)]
    for m in maps:
        m.setflags(write=False)
    return maps


def roi_table():
    return np.array([r[1:] for r in ROIS], F)


def roi_big_case():
    """C = 4096, the most the entry point admits (1024 threads): one level of 2 x 2, two rois, out 2."""
    maps = roi_maps(4096, ((2, 2),))
    rois = np.array([[1, 0.6, 0.9, 6.7, 7.2], [0, 1.3, -0.7, 5.1, 6.9]], F)
    return maps, (0.25,), rois, 2, 2


def roi_calls():
    """Every call of the table: ``(name, maps, scales, shapes, rois, out_size, sampling_ratio)``."""
    calls = [(f"C{C}-out{o}-g{g}", roi_maps(C), ROI_SCALES, ROI_SHAPES, roi_table(), o, g) for C, o, g in ROI_CONFIGS]
    maps, scales, rois, o, g = roi_big_case()
    return calls + [("C4096-out2-g2", maps, scales, ((2, 2),), rois, o, g)]


# ---- hp_box_postprocess: (n, n_classes, ld_logits, ld_regression); non-integer image, clipping on all four sides
BOX_IMAGE = (61.5, 83.25)
BOX_CASES = [(1, 2, 2, 8), (3, 5, 8, 24), (52, 5, 8, 20)]


def box_case(n, nc, ld, ldr, pad=np.nan):
    rs = np.random.RandomState(n)
    logits, reg = np.full((n, ld), pad, F), np.full((n, ldr), pad, F)
    lg, rg = rs.normal(0, 2, (n, nc)).astype(F), rs.normal(0, 1.5, (n, nc, 4)).astype(F)
    ctr, wh = rs.uniform((0, 0), (BOX_IMAGE[1], BOX_IMAGE[0]), (n, 2)), rs.uniform(4, 40, (n, 2))
    props = np.clip(np.concatenate([ctr - wh / 2, ctr + wh / 2], 1), 0, (BOX_IMAGE[1], BOX_IMAGE[0]) * 2).astype(F)
    for i in range(n):
        kind = (i + n) % 4
        if kind == 1:
            lg[i] = 1.25                                        # all equal: 1 / n_classes
        if kind == 2:
            # +-80 mixed; exp(80) = 5.5e34 still fits float32, so every other such row holds +-100, whose exp(100) is inf without
            # the subtraction of the maximum
            lg[i] = np.where(np.arange(nc) % 2 == 0, 1.0, -1.0) * (80.0 if i // 4 % 2 == 0 else 100.0)
        if kind in (1, 2):
            rg[i, :, 2:] = (25.0, 30.0)                          # d / 5 = 5 and 6, above log(1000 / 16) = 4.135
        if kind == 3:
            rg[i, :, 2:] = (-40.0, -60.0)                        # strongly negative: the box collapses onto its centre
        if i % 7 == 5:
            props[i, 2] = props[i, 0]                            # a proposal of zero width
        if i % 4 == 0:
            rg[i, :, :2] = ((-300.0, 8.0), (300.0, -8.0), (5.0, 300.0), (-5.0, -300.0), (0.5, 0.5))[i // 4 % 5]  # 30 sizes off each side
    logits[:, :nc], reg[:, :4 * nc] = lg, rg.reshape(n, -1)
    return logits, reg, props


# ---- hp_paste_masks: H = 37, W = 300 (a second pass of the 256 threads over the columns), 5 classes in rows of 8
PASTE_SIZE = (37, 300)
PASTE_BOXES = [
    ("interior", 100.3, 8.2, 140.9, 30.6),
    ("negative_corner", 0.2, 0.3, 25.4, 20.1),      # expanded corner (-0.7, -0.41): truncation gives 0, the floor would give -1
    ("beyond_image", -50.5, -20.3, 350.7, 60.4),    # wider and taller than the image
    ("sub_pixel", 150.2, 20.3, 150.5, 20.6),        # 0.3 x 0.3 px: w = h = 1
    ("far_corner", 260.4, 20.3, 300.0, 37.0),       # touches (W, H)
    ("zero_at_origin", 0.0, 0.0, 0.0, 0.0),
    ("second_pass", 252.0, 5.3, 298.1, 30.2),       # columns 250 .. 299
    ("interior_2", 30.7, 2.4, 75.2, 33.3),
]
PASTE_NC, PASTE_LD = 5, 8


def paste_case(pad=np.nan):
    rs = np.random.RandomState(28)
    n = len(PASTE_BOXES)
    nchw = (rs.normal(0, 2, (n, PASTE_NC, 28, 28)) + np.arange(PASTE_NC)[None, :, None, None] - 2).astype(F)  # planes differ per class
    labels = (np.arange(n) % 4 + 1).astype(np.int32)
    boxes = np.array([b[1:] for b in PASTE_BOXES], F)
    return SimpleNamespace(nchw=nchw, logits=interleave_masks(nchw, PASTE_LD, pad), labels=labels, boxes=boxes, H=PASTE_SIZE[0], W=PASTE_SIZE[1])


# ---- pre-processing: pixel totals that are no multiple of 256 and cross one block; two images
PREPROCESS_CASES = [(2, 5, 7), (2, 13, 21)]
RESIZE_CASES = [(2, 9, 13, 6, 9, 32, 32), (2, 6, 9, 11, 16, 32, 32)]  # n, h_in, w_in, h_out, w_out, h_pad, w_pad


def images_case(n, h, w):
    return np.random.RandomState(h * w).uniform(0, 1, (n, 3, h, w)).astype(F)
