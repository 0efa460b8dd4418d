"""float64 restatement of the detector's training targets and losses (torchvision 0.14's published definitions:
``models/detection/_utils.py`` Matcher / BalancedPositiveNegativeSampler / BoxCoder, ``ops/boxes.py`` box_iou, ``ops/roi_align.py``,
``models/detection/rpn.py`` and ``roi_heads.py`` losses).  torchvision itself cannot be run here, so parity with it is unpinned
and this file is the yardstick of ``csrc/det_losses.hip``: NumPy for the index logic, plain ``torch`` on the CPU with autograd for
the losses.  Every function takes the dtype it evaluates in: float64 is the reference, float32 is the same code as the measure of
what float32 arithmetic costs on a case (the tests allow 4 x that distance, floor one ulp).
"""

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_sample_ref import MASK32, philox4x32_10  # noqa: E402

EPS_DECISION = 1e-5
BETA = 1.0 / 9.0


# ---- Matcher on box_iou -------------------------------------------------------------------------------------------------------------
def box_iou(gt, boxes, dtype=np.float64):
    """``[G, n]``: area, lt / rb, clamped wh, inter / (a1 + a2 - inter), every operation in ``dtype``."""
    g, b = np.asarray(gt, dtype).reshape(-1, 4), np.asarray(boxes, dtype).reshape(-1, 4)
    a1 = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    a2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = np.maximum(g[:, None, :2], b[None, :, :2])
    rb = np.minimum(g[:, None, 2:], b[None, :, 2:])
    wh = np.maximum(rb - lt, dtype(0))
    inter = wh[..., 0] * wh[..., 1]
    return (inter / ((a1[:, None] + a2[None, :]) - inter)).astype(dtype)


def assign(boxes, image_of, gt, gt_off, high, low, allow_low_quality, dtype=np.float64, exact_ties=False):
    """``(match [n] (indices into the batch's gt table, -1, -2), iou [n], undecided [n] bool)``.  ``undecided`` marks the rows
    whose decision a perturbation of ``EPS_DECISION`` of an IoU could flip: the best IoU near a threshold, two ground truths
    near the row's maximum, or (low-quality matches) more than one row near a ground truth's maximum.  Ties at exactly 0 are
    exact in every format; ``exact_ties``: the coordinates are small integers, so every tie is."""
    boxes, image_of = np.asarray(boxes, dtype).reshape(-1, 4), np.asarray(image_of)
    n = boxes.shape[0]
    match, best_iou, undecided = np.full(n, -1, np.int32), np.zeros(n, dtype), np.zeros(n, bool)
    hi, lo = dtype(high), dtype(low)

    def near(d, at_zero):
        d = np.abs(d)
        tie = (d == 0) & (at_zero | exact_ties)
        return (d < EPS_DECISION) & ~tie

    for b in range(len(gt_off) - 1):
        rows = np.nonzero(image_of == b)[0]
        g0, g1 = int(gt_off[b]), int(gt_off[b + 1])
        if g1 == g0 or rows.size == 0:
            continue
        q = box_iou(np.asarray(gt)[g0:g1], boxes[rows], dtype)  # [g, r]
        arg = q.argmax(0)  # the first maximum
        vals = q[arg, np.arange(rows.size)]
        m = arg.astype(np.int32) + g0
        m[vals < lo] = -1
        m[(vals >= lo) & (vals < hi)] = -2
        und = near(vals - lo, False) | near(vals - hi, False)
        if g1 - g0 > 1:
            others = q.copy()
            others[arg, np.arange(rows.size)] = -1
            und |= near(vals - others.max(0), vals == 0)
        if allow_low_quality:
            gmax = q.max(1)
            restore = (q == gmax[:, None]).any(0)
            m[restore] = arg[restore] + g0
            d = np.abs(q - gmax[:, None])
            close = d < EPS_DECISION  # the rows at or near a ground truth's maximum
            safe = (gmax == 0) | exact_ties  # ties of this ground truth are exact in every format
            contested = np.where(safe, (close & (d > 0)).any(1), close.sum(1) > 1)
            und |= (close & contested[:, None]).any(0) & (vals < hi)  # at or above `high` the restore changes nothing
        match[rows], best_iou[rows], undecided[rows] = m, vals, und
    return match, best_iou, undecided


def canvas_anchors():
    """The 1536 anchors of a 64 x 96 canvas: levels 16 x 24, 8 x 12, 4 x 6, 2 x 3, 1 x 2 with three anchors each, in
    ``(level, y, x, a)`` order; sizes 8 .. 128, ratios 0.5, 1, 2, rounded as ``AnchorGenerator`` rounds."""
    out = []
    for (gh, gw), size in zip(((16, 24), (8, 12), (4, 6), (2, 3), (1, 2)), (8, 16, 32, 64, 128)):
        hr = np.sqrt(np.asarray((0.5, 1.0, 2.0), np.float32))
        wr = (np.float32(1) / hr).astype(np.float32)
        base = np.round(np.stack([-wr * size, -hr * size, wr * size, hr * size], 1) / np.float32(2)).astype(np.float32)
        y, x = np.meshgrid(np.arange(gh) * (64 // gh), np.arange(gw) * (96 // gw), indexing="ij")
        shifts = np.stack([x, y, x, y], -1).reshape(-1, 1, 4).astype(np.float32)
        out.append((shifts + base[None]).reshape(-1, 4))
    return np.concatenate(out)


def random_boxes(rng, n, W=96.0, H=64.0):
    c = rng.uniform((0, 0), (W, H), (n, 2))
    s = rng.uniform(4, 40, (n, 2))
    return np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)


def _accept(case):
    """A case stands when the reference itself leaves out at most 0.5 % of its rows under every setting it is run with."""
    for allow in (False, True):
        for high, low in ((0.7, 0.3), (0.5, 0.5)):
            und = assign(case["boxes"], case["image_of"], case["gt"], case["gt_off"], high, low, allow, exact_ties=case["exact_ties"])[2]
            if und.sum() > 0.005 * und.size:
                return False
    return True


def assign_cases():
    """name -> dict(boxes, image_of, gt, gt_off, exact_ties).  Seeds are walked until ``_accept`` holds: a property of the
    reference alone."""
    cases = {}
    anchors = canvas_anchors()
    for n_gt in (0, 1, 3, 9):  # a batch of 3 images, image 1 empty
        for seed in range(100):
            rng = np.random.default_rng(1000 * n_gt + seed)
            split = (n_gt - n_gt // 2, 0, n_gt // 2)
            case = dict(boxes=np.tile(anchors, (3, 1)), image_of=np.repeat(np.arange(3), anchors.shape[0]).astype(np.int32),
                        gt=random_boxes(rng, n_gt), gt_off=np.concatenate([[0], np.cumsum(split)]).astype(np.int32), exact_ties=False)
            if _accept(case):
                break
        else:
            raise AssertionError("no seed in 100 gives a decidable case")
        cases[f"canvas-gt{n_gt}"] = case
    for n in (1, 63, 64, 65, 257, 1025):  # 2 images
        for seed in range(100):
            rng = np.random.default_rng(7 * n + seed)
            image_of = np.sort(rng.integers(0, 2, n)).astype(np.int32)
            case = dict(boxes=random_boxes(rng, n), image_of=image_of, gt=random_boxes(rng, 5), gt_off=np.asarray([0, 2, 5], np.int32),
                        exact_ties=False)
            if _accept(case):
                break
        else:
            raise AssertionError("no seed in 100 gives a decidable case")
        cases[f"random-{n}"] = case
    cases["hand-tie"] = hand_tie_case()
    return cases


def hand_tie_case():
    """One ground truth (0, 0, 4, 4); anchors (-2, 0, 2, 4) and (2, 0, 6, 4) both meet it in 8 of 16 + 16 - 8 = 24: IoU 1 / 3 for
    both, the same quotient in every format, so both are the ground truth's maximum; (10, 10, 12, 12) misses it."""
    return dict(boxes=np.asarray([[-2, 0, 2, 4], [2, 0, 6, 4], [10, 10, 12, 12]], np.float32), image_of=np.zeros(3, np.int32),
                gt=np.asarray([[0, 0, 4, 4]], np.float32), gt_off=np.asarray([0, 1], np.int32), exact_ties=True)


# ---- BalancedPositiveNegativeSampler on Philox keys -------------------------------------------------------------------------------------
def sample_keys(image_of, seed, stream):
    """Word 0 of Philox4x32-10, counter (index of the row within its image, image, stream, 0), key (seed lo, seed hi)."""
    image_of = np.asarray(image_of, np.int64)
    index = np.zeros(image_of.size, np.int64)
    for b in np.unique(image_of):
        rows = np.nonzero(image_of == b)[0]
        index[rows] = np.arange(rows.size)
    c = np.stack([index, image_of, np.full_like(index, stream), np.zeros_like(index)], 1).astype(np.uint64)
    return philox4x32_10(c, (seed & MASK32, (seed >> 32) & MASK32))[:, 0].astype(np.int64)


def sample_counts(n_pos, n_neg, batch_size_per_image, positive_fraction):
    k_pos = min(n_pos, int(batch_size_per_image * positive_fraction))
    return k_pos, min(n_neg, batch_size_per_image - k_pos)


def sample(labels, image_of, n_images, batch_size_per_image, positive_fraction, seed, stream):
    """Per image ``(positive rows, negative rows)`` ascending: the ``k`` smallest ``(key, row)`` of each class."""
    labels, image_of = np.asarray(labels), np.asarray(image_of)
    keys = sample_keys(image_of, seed, stream)
    out = []
    for b in range(n_images):
        pos = np.nonzero((image_of == b) & (labels >= 1))[0]
        neg = np.nonzero((image_of == b) & (labels == 0))[0]
        k_pos, k_neg = sample_counts(pos.size, neg.size, batch_size_per_image, positive_fraction)
        pick = lambda rows, k: np.sort(rows[np.lexsort((rows, keys[rows]))[:k]])  # noqa: E731
        out.append((pick(pos, k_pos), pick(neg, k_neg)))
    return out


# ---- BoxCoder.encode_single -----------------------------------------------------------------------------------------------------------
def box_encode(boxes, match, gt, weights, dtype=np.float64):
    p = np.asarray(boxes, dtype).reshape(-1, 4)
    table = np.concatenate([np.asarray(gt, dtype).reshape(-1, 4), np.zeros((1, 4), dtype)])
    m = np.asarray(match)
    g = table[np.where((m >= 0) & (m < table.shape[0] - 1), m, table.shape[0] - 1)]
    wx, wy, ww, wh = (dtype(w) for w in weights)
    half = dtype(0.5)
    ex_w, ex_h = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    ex_cx, ex_cy = p[:, 0] + half * ex_w, p[:, 1] + half * ex_h
    gt_w, gt_h = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    gt_cx, gt_cy = g[:, 0] + half * gt_w, g[:, 1] + half * gt_h
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([wx * (gt_cx - ex_cx) / ex_w, wy * (gt_cy - ex_cy) / ex_h, ww * np.log(gt_w / ex_w), wh * np.log(gt_h / ex_h)],
                        1).astype(dtype)


# ---- roi_align, aligned = False, adaptive sampling ratio --------------------------------------------------------------------------------
def _bilinear(mask, y, x, dtype):
    """torchvision's ``bilinear_interpolate`` at the points ``y [M, 1]`` x ``x [1, M]``."""
    H, W = mask.shape
    y, x = np.broadcast_arrays(y, x)
    outside = (y < -1) | (y > H) | (x < -1) | (x > W)
    y, x = np.maximum(y, dtype(0)), np.maximum(x, dtype(0))
    y_low, x_low = y.astype(np.int64), x.astype(np.int64)
    top, right = y_low >= H - 1, x_low >= W - 1
    y_low, x_low = np.where(top, H - 1, y_low), np.where(right, W - 1, x_low)
    y_high, x_high = np.where(top, H - 1, y_low + 1), np.where(right, W - 1, x_low + 1)
    y, x = np.where(top, y_low.astype(dtype), y), np.where(right, x_low.astype(dtype), x)
    ly, lx = y - y_low.astype(dtype), x - x_low.astype(dtype)
    hy, hx = dtype(1) - ly, dtype(1) - lx
    m = mask.astype(dtype)
    val = (hy * hx) * m[y_low, x_low] + (hy * lx) * m[y_low, x_high] + (ly * hx) * m[y_high, x_low] + (ly * lx) * m[y_high, x_high]
    return np.where(outside, dtype(0), val).astype(dtype)


def mask_targets(masks, match, rois, M, dtype=np.float64):
    """``roi_align(masks[match][:, None], rois, (M, M), 1.0, -1, False)[:, 0]``: the loops of torchvision's kernel over rois and
    samples, the bins of a roi at once."""
    rois = np.asarray(rois, dtype).reshape(-1, 4)
    out = np.zeros((rois.shape[0], M, M), dtype)
    bins = np.arange(M).astype(dtype)
    for r, (x1, y1, x2, y2) in enumerate(rois):
        roi_w, roi_h = max(x2 - x1, dtype(1)), max(y2 - y1, dtype(1))
        bin_h, bin_w = roi_h / dtype(M), roi_w / dtype(M)
        gh, gw = int(np.ceil(roi_h / dtype(M))), int(np.ceil(roi_w / dtype(M)))
        acc = np.zeros((M, M), dtype)
        for iy in range(gh):
            y = (y1 + bins * bin_h) + (dtype(iy) + dtype(0.5)) * bin_h / dtype(gh)
            for ix in range(gw):
                x = (x1 + bins * bin_w) + (dtype(ix) + dtype(0.5)) * bin_w / dtype(gw)
                acc = acc + _bilinear(np.asarray(masks)[match[r]], y[:, None].astype(dtype), x[None, :].astype(dtype), dtype)
        out[r] = acc / dtype(max(gh * gw, 1))
    return out


# ---- the losses, with autograd ----------------------------------------------------------------------------------------------------------
def _leaf(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype).requires_grad_()


def _grads(losses, leaves):
    """Each loss's own gradient with respect to its leaves (an upstream gradient of 1)."""
    out = []
    for loss in losses:
        gs = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
        out.append([torch.zeros_like(l) if g is None else g for g, l in zip(gs, leaves)])
    return out


def rpn_loss(objectness, deltas, labels, targets, sampled, dtype=torch.float64):
    """``(loss_objectness, loss_rpn_box_reg, grad_objectness [A], grad_deltas [A, 4])`` as numpy float64."""
    obj, dlt = _leaf(objectness, dtype), _leaf(deltas, dtype)
    lab, tgt = torch.tensor(np.asarray(labels)), torch.tensor(np.asarray(targets), dtype=dtype)
    s = torch.tensor(np.asarray(sampled), dtype=torch.int64)
    sp = s[lab[s] >= 1]
    l_obj = F.binary_cross_entropy_with_logits(obj[s], (lab[s] >= 1).to(dtype))
    l_box = F.smooth_l1_loss(dlt[sp], tgt[sp], beta=BETA, reduction="sum") / s.numel()
    (g_obj, _), (_, g_box) = _grads([l_obj, l_box], [obj, dlt])
    return tuple(v.detach().double().numpy() for v in (l_obj, l_box, g_obj, g_box))


def fastrcnn_loss(logits, box_regression, labels, targets, n_classes, dtype=torch.float64):
    """``(loss_classifier, loss_box_reg, grad_logits [n, ld], grad_regression)``: the columns beyond ``n_classes`` are padding."""
    x, reg = _leaf(logits, dtype), _leaf(box_regression, dtype)
    lab, tgt = torch.tensor(np.asarray(labels), dtype=torch.int64), torch.tensor(np.asarray(targets), dtype=dtype)
    n = lab.numel()
    l_cls = F.cross_entropy(x[:, :n_classes], lab)
    pos = torch.where(lab > 0)[0]
    own = reg[:, :4 * n_classes].reshape(n, n_classes, 4)[pos, lab[pos]]
    l_box = F.smooth_l1_loss(own, tgt[pos], beta=BETA, reduction="sum") / n
    (g_cls, _), (_, g_reg) = _grads([l_cls, l_box], [x, reg])
    return tuple(v.detach().double().numpy() for v in (l_cls, l_box, g_cls, g_reg))


def mask_loss(mask_logits, labels, targets, dtype=torch.float64):
    """``(loss_mask, grad_logits [n, C, M, M])``; no rows: 0."""
    x = _leaf(mask_logits, dtype)
    lab, tgt = torch.tensor(np.asarray(labels), dtype=torch.int64), torch.tensor(np.asarray(targets), dtype=dtype)
    if lab.numel() == 0:
        return np.float64(0), np.zeros(x.shape)
    loss = F.binary_cross_entropy_with_logits(x[torch.arange(lab.numel()), lab], tgt)
    ((g,),) = _grads([loss], [x])
    return loss.detach().double().numpy(), g.detach().double().numpy()


def bound(ref64, ref32):
    """The project's usual bound: 4 x the float32 evaluation's distance from the float64 one, floor one float32 ulp of the
    largest entry."""
    ref64, ref32 = np.asarray(ref64, np.float64), np.asarray(ref32, np.float64)
    finite = np.isfinite(ref64) & np.isfinite(ref32)
    with np.errstate(invalid="ignore"):
        dist = np.abs(ref64 - ref32)[finite].max() if finite.any() else 0.0
    top = np.abs(ref64[finite]).max() if finite.any() else 0.0
    return max(4.0 * dist, float(np.spacing(np.float32(top))))
