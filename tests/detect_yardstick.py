"""Yardsticks of the detector stages' GPU tests: how far a float32 evaluation of each definition lies from the float64 reference
(tests/detect_ref.py).  Unlike the reference this module knows the order in which the kernels of detect.hip and pool_head.hip
operate, and that they do not contract a multiply and an add (``fp contract(off)``).  Nothing here is compared with a kernel, it
only sizes the bounds.  Every figure of MEASURED_F32_ERROR is measured over the whole case table and asserted by
tests/test_detect_reference.py on the CPU; tests/test_gpu_detect_stages.py allows the kernels 4x (another order of association, the
device's expf / log2f / division in place of NumPy's), and a discrete decision whose margin is below 4x the error of its deciding
quantity is fragile: either outcome is a correct float32 answer.

The scales S the errors are relative to: boxes -- max(image size, |anchor or proposal coordinates|, decoded width and height) per
box; pooled features -- max|map| of the level; probabilities, scores and masks -- 1; normalised pixels -- 1 / std of the channel;
sample coordinates -- max(|roi on the map|, map size); expanded mask corners -- max(image size, |box coordinates|).

Measured (worst |f32 - f64| / S over the table): rpn_boxes 9.7e-8, rpn_wh 1.5e-7, rpn_scores 8.55e-8, nms_iou 2.98e-8,
roi_level_v 2.49e-7, roi_coord 2.55e-7, roi_values 1.36e-6, box_scores 7.73e-8, box_boxes 1.23e-7, paste_corner 6.91e-8,
paste_masks 2.05e-6, preprocess 5.55e-8, resize 3.29e-7.  roi_values and paste_masks are the largest because the sample
coordinates, of magnitude up to 30 px, are rounded to float32 before a map of slope max|map| per px is interpolated at them."""

import numpy as np

import detect_ref as R

F = np.float32
D = np.float64
CLIP = F(R.XFORM_CLIP)


def _sigmoid32(x):
    with np.errstate(over="ignore"):
        return (F(1) / (F(1) + np.exp(-np.asarray(x, F)))).astype(F)


def _decode32(boxes, d, wxy, wwh, im_h, im_w):
    """The kernels' decode: ``boxes [..., 4]``, ``d [..., 4]`` float32 -> clipped boxes, raw boxes; centre form, clamp, exp,
    corners, clip.  ``wxy`` / ``wwh`` None: the weights (1, 1, 1, 1) are not divided by."""
    b, d = np.asarray(boxes, F), np.asarray(d, F)
    wd, ht = b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]
    cx, cy = b[..., 0] + F(0.5) * wd, b[..., 1] + F(0.5) * ht
    dx, dy, dw, dh = d[..., 0], d[..., 1], d[..., 2], d[..., 3]
    if wxy is not None:
        dx, dy, dw, dh = dx / F(wxy), dy / F(wxy), dw / F(wwh), dh / F(wwh)
    dw, dh = np.minimum(dw, CLIP), np.minimum(dh, CLIP)
    pcx, pcy = dx * wd + cx, dy * ht + cy
    pw, ph = np.exp(dw) * wd, np.exp(dh) * ht
    raw = np.stack([pcx - F(0.5) * pw, pcy - F(0.5) * ph, pcx + F(0.5) * pw, pcy + F(0.5) * ph], -1)
    assert raw.dtype == F
    out = raw.copy()
    out[..., 0::2] = np.minimum(np.maximum(out[..., 0::2], F(0)), F(im_w))
    out[..., 1::2] = np.minimum(np.maximum(out[..., 1::2], F(0)), F(im_h))
    return out, raw


def box_scale(im_h, im_w, source, wh):
    """S of a decoded box: ``source [..., 4]`` the anchor or the proposal, ``wh [..., 2]`` the decoded width and height."""
    s = np.maximum(np.abs(np.asarray(source, D)).max(-1), np.abs(np.asarray(wh, D)).max(-1))
    return np.maximum(s, max(float(im_h), float(im_w)))


# ---------------------------------------------------------------------------------------------------------------- hp_rpn_decode
def rpn_f32(case):
    idx = case.idx.astype(np.int64)
    a, pos = idx % 3, idx // 3
    y, x = pos // case.gw, pos % case.gw
    sx, sy = (x * case.stride_w).astype(F), (y * case.stride_h).astype(F)
    base = case.base.reshape(3, 4)[a]
    anchors = np.stack([sx + base[:, 0], sy + base[:, 1], sx + base[:, 2], sy + base[:, 3]], 1)
    boxes, _ = _decode32(anchors, case.deltas.reshape(-1, 3, 4)[pos, a], None, None, case.im_h, case.im_w)
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    return dict(boxes=boxes, scores=_sigmoid32(case.obj), valid=(w >= F(case.min_size)) & (h >= F(case.min_size)), wh=np.stack([w, h], 1))


def rpn_scale(case, ref):
    return box_scale(case.im_h, case.im_w, ref["anchors"], ref["wh"])


def rpn_fragile(case, ref):
    """Entries whose small-box flag may fall either way in float32."""
    return ref["valid_margin"] < 4 * MEASURED_F32_ERROR["rpn_wh"] * rpn_scale(case, ref)


# ----------------------------------------------------------------------------------------------------------------------- hp_nms
def iou_f32(boxes):
    b = np.asarray(boxes, F)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.maximum(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), F(0))
    ih = np.maximum(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), F(0))
    inter = iw * ih
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / ((area[:, None] + area[None, :]) - inter)
    assert iou.dtype == F
    return iou


def nms_fragile(ref):
    """Pairs (i before j, one group) whose comparison with the threshold may fall either way in float32."""
    return np.triu(ref["margin"] < 4 * MEASURED_F32_ERROR["nms_iou"], 1)


# ---------------------------------------------------------------------------------------------------------- hp_roi_align_levels
def level_v32(rois):
    r = np.asarray(rois, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2]))
        v = (F(4) + np.log2(s / F(224))) + F(1e-6)
    assert v.dtype == F
    return v


def _axis32(start, bin_size, n, size, g):
    p, s = np.arange(n, dtype=F)[:, None], np.arange(g, dtype=F)[None, :]
    y = (F(start) + p * F(bin_size)) + ((s + F(0.5)) * F(bin_size)) / F(g)
    assert y.dtype == F
    valid = ~((y < F(-1)) | (y > F(size)))
    yc = np.where(y <= 0, F(0), y)
    lo = yc.astype(np.int64)
    top = lo >= size - 1
    lo = np.where(top, size - 1, lo)
    hi = np.where(top, size - 1, lo + 1)
    yc = np.where(top, lo.astype(F), yc)
    return y, valid, lo, hi, (yc - lo.astype(F)).astype(F)


def roi_f32(maps, scales, k_min, rois, out_size, g, levels):
    """Values ``[K][out][out][C]`` and sample coordinates in float32, in the kernel's order: per sample ``w1 v1 + w2 v2 + w3 v3 +
    w4 v4`` from the left, the samples added rows outside and columns inside, divided by their number.  ``levels`` from the
    reference (the level is compared on its own)."""
    rois = np.asarray(rois, F)
    K, C = len(rois), maps[0].shape[-1]
    values = np.zeros((K, out_size, out_size, C), F)
    coords, valids = [], []
    for k in range(K):
        f = maps[levels[k]][int(rois[k, 0])]
        H, W = f.shape[:2]
        sc = F(scales[levels[k]])
        x1, y1, x2, y2 = [F(v) * sc for v in rois[k, 1:]]
        rw, rh = max(x2 - x1, F(1)), max(y2 - y1, F(1))
        ys, vy, ylo, yhi, ly = _axis32(y1, rh / F(out_size), out_size, H, g)
        xs, vx, xlo, xhi, lx = _axis32(x1, rw / F(out_size), out_size, W, g)
        coords.append((ys, xs))
        valids.append((vy, vx))
        acc = np.zeros((out_size, out_size, C), F)
        for iy in range(g):
            for ix in range(g):
                ok = (vy[:, iy][:, None] & vx[:, ix][None, :])[..., None]
                hy, l_y = (F(1) - ly[:, iy])[:, None, None], ly[:, iy][:, None, None]
                hx, l_x = (F(1) - lx[:, ix])[None, :, None], lx[:, ix][None, :, None]
                yl, yh, xl, xh = ylo[:, iy][:, None], yhi[:, iy][:, None], xlo[:, ix][None, :], xhi[:, ix][None, :]
                val = (((hy * hx) * f[yl, xl] + (hy * l_x) * f[yl, xh]) + (l_y * hx) * f[yh, xl]) + (l_y * l_x) * f[yh, xh]
                acc = acc + np.where(ok, val, F(0))
        assert acc.dtype == F
        values[k] = acc / F(g * g)
    return values, coords, valids


def roi_coord_scale(rois, scales, levels, shapes):
    """S of the sample coordinates per roi: the larger of the roi's coordinates on its map and the map's sides."""
    r = np.abs(np.asarray(rois, D)[:, 1:]) * np.asarray(scales, D)[levels][:, None]
    return np.maximum(r.max(1), np.array([max(shapes[l]) for l in levels], D))


def roi_fragile(ref, rois, scales, shapes):
    """``(levels that may floor either way [K], bins with a sample that may be valid either way [K][out][out])``."""
    e = MEASURED_F32_ERROR
    sc = roi_coord_scale(rois, scales, ref["levels"], shapes)
    return ref["level_margin"] < 4 * e["roi_level_v"], ref["sample_margin"] < (4 * e["roi_coord"] * sc)[:, None, None]


# ----------------------------------------------------------------------------------------------------------- hp_box_postprocess
def box_f32(logits, ld, reg, ldr, props, n, nc, im_h, im_w):
    lg = np.asarray(logits, F).reshape(n, ld)[:, :nc]
    rg = np.asarray(reg, F).reshape(n, ldr)[:, :4 * nc].reshape(n, nc, 4)
    mx = lg.max(1, keepdims=True)
    den = np.zeros((n, 1), F)
    for k in range(nc):
        den = den + np.exp(lg[:, k:k + 1] - mx)
    scores = np.exp(lg - mx) / den
    assert scores.dtype == F
    boxes, _ = _decode32(np.asarray(props, F).reshape(n, 1, 4), rg, 10, 5, im_h, im_w)
    return scores, boxes


# --------------------------------------------------------------------------------------------------------------- hp_paste_masks
def paste_corners32(boxes):
    b = np.asarray(boxes, F)
    scale = F(30) / F(28)
    wh, hh = (b[:, 2] - b[:, 0]) * F(0.5) * scale, (b[:, 3] - b[:, 1]) * F(0.5) * scale
    xc, yc = (b[:, 2] + b[:, 0]) * F(0.5), (b[:, 3] + b[:, 1]) * F(0.5)
    out = np.stack([xc - wh, yc - hh, xc + wh, yc + hh], 1)
    assert out.dtype == F
    return out


def _resize_axis32(n_out, n_in, scale):
    src = np.maximum(F(scale) * (np.arange(n_out, dtype=F) + F(0.5)) - F(0.5), F(0))
    lo = np.minimum(src.astype(np.int64), n_in - 1)
    hi = np.minimum(lo + 1, n_in - 1)
    l = src - lo.astype(F)
    assert l.dtype == F
    return lo, hi, l


def _bilinear32(p, ylo, yhi, ly, xlo, xhi, lx):
    """``hy (hx p00 + lx p01) + ly (hx p10 + lx p11)`` over the last two axes of ``p``, float32."""
    ly, lx = ly[:, None], lx[None, :]
    hy, hx = F(1) - ly, F(1) - lx
    out = hy * (hx * p[..., ylo, :][..., xlo] + lx * p[..., ylo, :][..., xhi]) + ly * (hx * p[..., yhi, :][..., xlo] + lx * p[..., yhi, :][..., xhi])
    assert out.dtype == F
    return out


def paste_f32(case, rect, be):
    """Masks ``[n][H][W]`` float32 in the kernel's order; the integer box ``be`` and the rectangle from the reference."""
    n = len(case.boxes)
    out = np.zeros((n, case.H, case.W), F)
    for k in range(n):
        padded = np.zeros((30, 30), F)
        padded[1:-1, 1:-1] = _sigmoid32(case.nchw[k, case.labels[k]])
        w, h = max(int(be[k, 2] - be[k, 0] + 1), 1), max(int(be[k, 3] - be[k, 1] + 1), 1)
        ylo, yhi, ly = _resize_axis32(h, 30, F(30) / F(h))
        xlo, xhi, lx = _resize_axis32(w, 30, F(30) / F(w))
        mm = _bilinear32(padded, ylo, yhi, ly, xlo, xhi, lx)
        x0, x1, y0, y1 = rect[k]
        if y1 > y0 and x1 > x0:
            out[k, y0:y1, x0:x1] = mm[y0 - be[k, 1]:y1 - be[k, 1], x0 - be[k, 0]:x1 - be[k, 0]]
    return out


def paste_corner_scale(case):
    return np.maximum(np.abs(np.asarray(case.boxes, D)).max(1), max(case.H, case.W))


def paste_fragile(case, ref):
    return ref["trunc_margin"] < 4 * MEASURED_F32_ERROR["paste_corner"] * paste_corner_scale(case)


# ---------------------------------------------------------------------------------------------------------------- pre-processing
MEAN32, STD32 = np.asarray(R.IMAGE_MEAN, F), np.asarray(R.IMAGE_STD, F)
PIXEL_SCALE = 1.0 / STD32.astype(D)  # [3]: images are in [0, 1], the subtraction's operands are at most 1


def preprocess_f32(x):
    out = np.zeros(x.shape[:1] + x.shape[2:] + (4,), F)
    out[..., :3] = ((np.asarray(x, F) - MEAN32[None, :, None, None]) / STD32[None, :, None, None]).transpose(0, 2, 3, 1)
    return out


def resize_f32(x, ho, wo, hp, wp):
    x = np.asarray(x, F)
    n, _, hi, wi = x.shape
    ylo, yhi, ly = _resize_axis32(ho, hi, F(hi) / F(ho))
    xlo, xhi, lx = _resize_axis32(wo, wi, F(wi) / F(wo))
    out = np.zeros((n, hp, wp, 4), F)
    out[:, :ho, :wo] = preprocess_f32(_bilinear32(x, ylo, yhi, ly, xlo, xhi, lx))
    return out


# ------------------------------------------------------------------------------------------------------------------ measurement
def measure():
    """Worst ``|f32 - f64| / S`` per quantity over every case of detect_ref's tables, and ``decisions``: the number of discrete
    decisions of the float32 evaluation that differ from the reference's (none may)."""
    w = {k: 0.0 for k in MEASURED_F32_ERROR}
    flips = 0

    def up(key, err, scale=1.0):
        err = np.asarray(err, D) / scale
        if err.size:
            w[key] = max(w[key], float(np.nanmax(err)))

    for g, s in R.RPN_CASES:
        case = R.rpn_case(g, s)
        ref, got = R.rpn_ref(case), rpn_f32(case)
        S = rpn_scale(case, ref)
        up("rpn_boxes", np.abs(got["boxes"] - ref["boxes"]).max(1), S)
        rwh = np.stack([ref["boxes"][:, 2] - ref["boxes"][:, 0], ref["boxes"][:, 3] - ref["boxes"][:, 1]], 1)
        up("rpn_wh", np.abs(got["wh"] - rwh).max(1), S)
        up("rpn_scores", np.abs(got["scores"] - ref["scores"]))
        flips += int((got["valid"] != ref["valid"]).sum())
    for name in R.NMS_CASES:
        case = R.nms_case(name)
        ref, got = R.ref_nms(case.boxes, case.group, case.thr), iou_f32(case.boxes)
        same = np.isfinite(ref["margin"])
        up("nms_iou", np.abs(got - ref["iou"])[same])
        with np.errstate(invalid="ignore"):
            flips += int(((got > case.thr) != (ref["iou"] > float(case.thr)))[same].sum())
    for _, maps, scales, shapes, r, out, g in R.roi_calls():
        ref = R.ref_roi_align_levels(maps, scales, 2, r, out, g)
        v32 = level_v32(r)
        fin = np.isfinite(ref["v"])
        up("roi_level_v", np.abs(v32[fin] - ref["v"][fin]))
        lv32 = np.clip(np.floor(v32), 2, 1 + len(maps)).astype(np.int64) - 2
        flips += int((lv32 != ref["levels"]).sum())
        vals, coords, valids = roi_f32(maps, scales, 2, r, out, g, ref["levels"])
        sc = roi_coord_scale(r, scales, ref["levels"], shapes)
        for k in range(len(r)):
            ys, xs, H, W = ref["coords"][k]
            up("roi_coord", max(np.abs(coords[k][0] - ys).max(), np.abs(coords[k][1] - xs).max()), sc[k])
            flips += int((valids[k][0] != ~((ys < -1) | (ys > H))).sum() + (valids[k][1] != ~((xs < -1) | (xs > W))).sum())
            up("roi_values", np.abs(vals[k] - ref["values"][k]), float(np.abs(maps[ref["levels"][k]]).max()))
    for n, nc, ld, ldr in R.BOX_CASES:
        lg, rg, props = R.box_case(n, nc, ld, ldr)
        ref = R.ref_box_postprocess(lg, ld, rg, ldr, props, n, nc, *R.BOX_IMAGE)
        sc, bx = box_f32(lg, ld, rg, ldr, props, n, nc, *R.BOX_IMAGE)
        up("box_scores", np.abs(sc - ref["scores"]))
        S = box_scale(*R.BOX_IMAGE, np.asarray(props, D).reshape(n, 1, 4), ref["wh"])
        up("box_boxes", np.abs(bx - ref["boxes"]).max(-1), S)
    case = R.paste_case()
    ref = R.ref_paste_masks(case.logits, R.PASTE_LD, case.labels, case.boxes, len(case.boxes), case.H, case.W)
    c32 = paste_corners32(case.boxes)
    up("paste_corner", np.abs(c32 - ref["corners"]).max(1), paste_corner_scale(case))
    be = np.trunc(ref["corners"]).astype(np.int64)
    flips += int((np.trunc(c32).astype(np.int64) != be).sum())
    up("paste_masks", np.abs(paste_f32(case, ref["rect"], be) - ref["masks"]))
    for n, h, w_ in R.PREPROCESS_CASES:
        x = R.images_case(n, h, w_)
        up("preprocess", np.abs(preprocess_f32(x) - R.ref_preprocess(x, MEAN32, STD32))[..., :3], PIXEL_SCALE)
    for n, hi, wi, ho, wo, hp, wp in R.RESIZE_CASES:
        x = R.images_case(n, hi, wi)
        up("resize", np.abs(resize_f32(x, ho, wo, hp, wp) - R.ref_preprocess_resize(x, ho, wo, hp, wp, MEAN32, STD32))[..., :3], PIXEL_SCALE)
    w["decisions"] = flips
    return w


# Worst |f32 - f64| / S over the tables of detect_ref (see the module docstring for S); nms_iou, roi_level_v and the scores are absolute.
MEASURED_F32_ERROR = {"rpn_boxes": 9.7e-8, "rpn_wh": 1.5e-7, "rpn_scores": 8.55e-8, "nms_iou": 2.98e-8, "roi_level_v": 2.49e-7,
                      "roi_coord": 2.55e-7, "roi_values": 1.36e-6, "box_scores": 7.73e-8, "box_boxes": 1.23e-7, "paste_corner": 6.91e-8,
                      "paste_masks": 2.05e-6, "preprocess": 5.55e-8, "resize": 3.29e-7}
