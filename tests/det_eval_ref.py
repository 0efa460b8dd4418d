"""The specification of the detection / segmentation scoring (happypose_amd.evaluation: box_iou, mask_iou, DetectionMeter,
CocoMeter; csrc/det_eval.hip), in numpy float64 and integers.  It never imports the package.

The definitions are the published ones, restated: torchvision 0.14.1 ``ops.box_iou``; pycocotools 2.0 ``COCOeval.evaluateImg`` /
``accumulate`` / ``summarize`` without area ranges and crowd regions; the reference's ``DetectionMeter`` with its default
arguments.  Everything is a literal loop, written for reading rather than speed.
"""

import numpy as np

GROUP_KEYS = ("scene_id", "view_id", "label")
COCO_IOU_THRESHOLDS = tuple(round(0.5 + 0.05 * k, 2) for k in range(10))
RECALL_POINTS = np.linspace(0.0, 1.0, 101)


# ---- IoU -------------------------------------------------------------------------------------------------------------------------
def box_iou(boxes1, boxes2, dtype=np.float64):
    """torchvision's ``box_iou`` on xyxy boxes, all pairs, evaluated in ``dtype`` operation by operation."""
    b1, b2 = np.asarray(boxes1, dtype=dtype).reshape(-1, 4), np.asarray(boxes2, dtype=dtype).reshape(-1, 4)
    out = np.zeros((len(b1), len(b2)), dtype=dtype)
    zero = dtype(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, a in enumerate(b1):
            for j, b in enumerate(b2):
                area_a = (a[2] - a[0]) * (a[3] - a[1])
                area_b = (b[2] - b[0]) * (b[3] - b[1])
                w = max(min(a[2], b[2]) - max(a[0], b[0]), zero)
                h = max(min(a[3], b[3]) - max(a[1], b[1]), zero)
                inter = w * h
                out[i, j] = inter / (area_a + area_b - inter)
    return out


def pack_masks(masks):
    """``[n, H, W]`` (non-zero = set) -> ``[n, ceil(H W / 64)]`` uint64: bit ``i`` of word ``k`` is pixel ``64 k + i``, tail bits 0."""
    m = np.asarray(masks)
    n = m.shape[0]
    flat = (m.reshape(n, -1) != 0)
    n_words = (flat.shape[1] + 63) // 64
    padded = np.zeros((n, n_words * 64), dtype=np.uint64)
    padded[:, :flat.shape[1]] = flat
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (padded.reshape(n, n_words, 64) * weights).sum(axis=2, dtype=np.uint64)


def mask_counts(mask1, mask2):
    """``(inter, union)`` pixel counts of two masks."""
    a, b = np.asarray(mask1) != 0, np.asarray(mask2) != 0
    return int((a & b).sum()), int((a | b).sum())


def mask_iou(mask1, mask2):
    """float64 IoU of the float32 quotient the device computes: ``float32(inter) / float32(union)``, 0 for an empty union."""
    inter, union = mask_counts(mask1, mask2)
    return 0.0 if union == 0 else float(np.float32(inter) / np.float32(union))


# ---- COCO ------------------------------------------------------------------------------------------------------------------------
def coco_thresholds(thresholds):
    """What the kernel compares with: ``float32(min(t, 1 - 1e-10))``."""
    return np.asarray([np.float32(min(float(t), 1 - 1e-10)) for t in thresholds], dtype=np.float32)


def coco_match(iou, gt_ignore, thresholds):
    """pycocotools' matching loop for one image and label.  ``iou [D, G]`` with the detections in descending-score order and the
    ground truths with the non-ignored ones first.  Returns ``det_match [T, D]``, ``det_ignore [T, D]``, ``gt_match [T, G]``."""
    iou = np.asarray(iou, dtype=np.float64)
    assert iou.ndim == 2 and iou.shape[1] == len(gt_ignore)
    D, G = iou.shape
    thr = coco_thresholds(thresholds).astype(np.float64)
    det_match = np.full((len(thr), D), -1, dtype=np.int64)
    det_ignore = np.zeros((len(thr), D), dtype=bool)
    gt_match = np.full((len(thr), G), -1, dtype=np.int64)
    for t, th in enumerate(thr):
        for d in range(D):
            best, m = th, -1
            for g in range(G):
                if gt_match[t, g] >= 0:
                    continue
                if m > -1 and not gt_ignore[m] and gt_ignore[g]:  # matched to a regular ground truth, now among the ignored ones
                    break
                if not iou[d, g] >= best:  # pycocotools: `if ious[d, g] < iou: continue`; a NaN never matches
                    continue
                best, m = iou[d, g], g
            if m == -1:
                continue
            det_match[t, d], gt_match[t, m], det_ignore[t, d] = m, d, bool(gt_ignore[m])
    return det_match, det_ignore, gt_match


def coco_accumulate(det_label, det_score, det_match, det_ignore, gt_label, gt_ignore, thresholds=COCO_IOU_THRESHOLDS):
    """pycocotools' ``accumulate`` + ``summarize``: ``AP``, ``AP50``, ``AP75``, ``AR`` in float64 (-1 when nothing counts)."""
    thr = list(thresholds)
    det_match, det_ignore = np.asarray(det_match).reshape(len(thr), -1), np.asarray(det_ignore).reshape(len(thr), -1)
    eps = np.spacing(1)
    precision, recall = {}, {}
    for label in sorted(set(gt_label)):
        n_gt = sum(1 for lab, ig in zip(gt_label, gt_ignore) if lab == label and not ig)
        if n_gt == 0:
            continue
        ids = [i for i, lab in enumerate(det_label) if lab == label]
        order = [ids[k] for k in np.argsort([-det_score[i] for i in ids], kind="mergesort")] if ids else []
        for t in range(len(thr)):
            tp = fp = 0.0
            rc, pr = [], []
            for i in order:
                if det_ignore[t, i]:
                    tp, fp = tp + 0.0, fp + 0.0  # an ignored detection counts neither way, but keeps its place in the curve
                elif det_match[t, i] >= 0:
                    tp += 1.0
                else:
                    fp += 1.0
                rc.append(tp / n_gt)
                pr.append(tp / (fp + tp + eps))
            recall[label, t] = rc[-1] if rc else 0.0
            for i in range(len(pr) - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            q = np.zeros(len(RECALL_POINTS))
            for ri, pi in enumerate(np.searchsorted(rc, RECALL_POINTS, side="left") if rc else []):
                if pi < len(pr):
                    q[ri] = pr[pi]
            precision[label, t] = q
    if not precision:
        return {"AP": -1.0, "AP50": -1.0, "AP75": -1.0, "AR": -1.0}
    labels = sorted({k[0] for k in precision})

    def mean_precision(ts):
        return float(np.mean([precision[label, t] for label in labels for t in ts])) if ts else -1.0

    at = lambda v: [t for t, th in enumerate(thr) if abs(th - v) < 1e-9]  # noqa: E731
    return {"AP": mean_precision(list(range(len(thr)))), "AP50": mean_precision(at(0.5)), "AP75": mean_precision(at(0.75)),
            "AR": float(np.mean([recall[label, t] for label in labels for t in range(len(thr))]))}


def _groups(preds, gts):
    keys = sorted({tuple(r[k] for k in GROUP_KEYS) for r in list(preds) + list(gts)})
    return [(key, [i for i, r in enumerate(preds) if tuple(r[k] for k in GROUP_KEYS) == key],
             [j for j, r in enumerate(gts) if tuple(r[k] for k in GROUP_KEYS) == key]) for key in keys]


def pair_iou(iou_type, pred, gt):
    if iou_type == "bbox":
        return float(box_iou([pred["box"]], [gt["box"]])[0, 0])
    return mask_iou(pred["mask"], gt["mask"])


def coco_evaluate(preds, gts, iou_type, thresholds=COCO_IOU_THRESHOLDS, max_dets=100, return_ious=False):
    """COCO's evaluation of record lists (dicts with the group keys, ``score`` / ``ignore``, ``box`` / ``mask``)."""
    det_label, det_score, gt_label, gt_ignore, dm, di, all_ious = [], [], [], [], [], [], []
    for key, p_ids, g_ids in _groups(preds, gts):
        p_ids = [p_ids[k] for k in np.argsort([-preds[i]["score"] for i in p_ids], kind="mergesort")][:max_dets] if p_ids else []
        g_ids = [g_ids[k] for k in np.argsort([bool(gts[j].get("ignore", False)) for j in g_ids], kind="mergesort")] if g_ids else []
        ign = [bool(gts[j].get("ignore", False)) for j in g_ids]
        iou = np.array([[pair_iou(iou_type, preds[i], gts[j]) for j in g_ids] for i in p_ids], dtype=np.float64).reshape(len(p_ids), len(g_ids))
        all_ious.extend(iou.reshape(-1).tolist())
        m, ig, _ = coco_match(iou, ign, thresholds)
        det_label += [key[2]] * len(p_ids)
        det_score += [preds[i]["score"] for i in p_ids]
        gt_label += [key[2]] * len(g_ids)
        gt_ignore += ign
        dm.append(m), di.append(ig)
    T = len(thresholds)
    dm = np.concatenate(dm, axis=1) if dm else np.zeros((T, 0), dtype=np.int64)
    di = np.concatenate(di, axis=1) if di else np.zeros((T, 0), dtype=bool)
    out = coco_accumulate(det_label, det_score, dm, di, gt_label, gt_ignore, thresholds)
    return (out, np.asarray(all_ious)) if return_ious else out


# ---- the reference's DetectionMeter (default arguments: every ground truth valid, every prediction kept) ----------------------------
def average_precision(y_true, y_score):
    """scikit-learn's ``average_precision_score`` for binary labels: sum over the distinct score thresholds, in descending order,
    of (recall step) x (precision there)."""
    pairs = sorted(zip(y_score, y_true), key=lambda p: -p[0])
    n_pos = sum(1 for _, y in pairs if y)
    if n_pos == 0:
        return 0.0
    ap, tp, prev_recall = 0.0, 0, 0.0
    for k, (s, y) in enumerate(pairs):
        tp += 1 if y else 0
        if k + 1 < len(pairs) and pairs[k + 1][0] == s:
            continue  # not the last detection of this score
        recall = tp / n_pos
        ap += (recall - prev_recall) * (tp / (k + 1))
        prev_recall = recall
    return ap


def detection_meter(preds, gts, iou_type, iou_threshold=0.5):
    """The reference's ``DetectionMeter.add`` + ``summary`` on record lists.  Scores inside one group must be distinct."""
    views = {(r["scene_id"], r["view_id"]) for r in gts}
    preds = [r for r in preds if (r["scene_id"], r["view_id"]) in views]
    pred_tp = [False] * len(preds)
    n_matched = 0
    for key, p_ids, g_ids in _groups(preds, gts):
        taken = set()
        for i in sorted(p_ids, key=lambda i: -preds[i]["score"]):
            best, best_iou = None, None
            for j in g_ids:  # the first ground truth on a tie
                v = pair_iou(iou_type, preds[i], gts[j])
                if j in taken or not v >= iou_threshold:
                    continue
                if best is None or v > best_iou:
                    best, best_iou = j, v
            if best is not None:
                taken.add(best)
                pred_tp[i] = True
                n_matched += 1
    labels = sorted({r["label"] for r in gts})
    n_gts = {label: sum(1 for r in gts if r["label"] == label) for label in labels}

    def compute_ap(ids, n_gt):
        y = [pred_tp[i] for i in ids]
        return average_precision(y, [preds[i]["score"] for i in ids]) * sum(y) / n_gt

    aps = {}
    for label in labels:
        ids = [i for i, r in enumerate(preds) if r["label"] == label]
        if ids and any(pred_tp[i] for i in ids):
            aps[label] = compute_ap(ids, n_gts[label])
    n_gt_valid = sum(n_gts.values())
    if aps:
        mAP, AP = float(np.mean(list(aps.values()))), compute_ap(list(range(len(preds))), n_gt_valid)
    else:
        mAP, AP = 0.0, 0.0
    return {"n_gt": len(gts), "n_gt_valid": n_gt_valid, "n_pred": len(preds), "n_matched": n_matched,
            "matched_gt_ratio": n_matched / n_gt_valid, "pred_matched_ratio": len(preds) / max(n_matched, 1),
            "iou_valid_recall": n_matched / n_gt_valid, "AP": AP, "mAP": mAP}


# ---- hand cases ------------------------------------------------------------------------------------------------------------------
def _rec(view, label, box, score=None, ignore=False):
    r = {"scene_id": 0, "view_id": view, "label": label, "box": box}
    if score is None:
        r["ignore"] = ignore
    else:
        r["score"] = score
    return r


A, B, FAR = (0.0, 0.0, 10.0, 10.0), (20.0, 0.0, 30.0, 10.0), (100.0, 100.0, 110.0, 110.0)

# Every box below either coincides with a ground truth (IoU 1: matched at all ten thresholds) or is disjoint from all (IoU 0), so
# each threshold gives the same curve and AP = AP50 = AP75.  precision = tp / (tp + fp + eps) with eps = 2^-52 is below the exact
# ratio by about one part in 2^52: the values are asserted to 1e-12.
HAND_CASES = {
    # One prediction exactly on the one ground truth.  Sorted detections: [TP].  recall = [1], precision = [1].  Every one of the
    # 101 recall points r <= 1 finds index 0 (searchsorted left), precision 1.  AP = 101 / 101 = 1.  AR = 1.
    "one_on_one": dict(preds=[_rec(0, "a", A, score=0.9)], gts=[_rec(0, "a", A)], AP=1.0, AR=1.0),
    # Two ground truths, one prediction on the first.  recall = [1/2], precision = [1].  The recall points 0, 0.01, ..., 0.50 (51
    # of them; 0.50 == 1/2 finds index 0 with side="left") read precision 1, the 50 points above 0.5 fall past the curve: 0.
    # AP = 51 / 101.  AR = 1/2.
    "one_of_two": dict(preds=[_rec(0, "a", A, score=0.9)], gts=[_rec(0, "a", A), _rec(0, "a", B)], AP=51.0 / 101.0, AR=0.5),
    # One ground truth; a false positive scored ABOVE the true positive.  Sorted: [FP, TP].  tp = [0, 1], fp = [1, 1].
    # recall = [0, 1], precision = [0, 1/2], monotone from the right: [1/2, 1/2].  Point 0 finds index 0, every other point index
    # 1: all 101 read 1/2.  AP = 1/2.  AR = 1.
    "fp_above_tp": dict(preds=[_rec(0, "a", FAR, score=0.9), _rec(0, "a", A, score=0.8)], gts=[_rec(0, "a", A)], AP=0.5, AR=1.0),
    # The same with a second ground truth that nobody finds.  recall = [0, 1/2], precision [0, 1/2] -> [1/2, 1/2].  The 51 points
    # up to 0.50 read 1/2, the rest 0.  AP = 0.5 x 51 / 101.  AR = 1/2.
    "fp_above_tp_one_of_two": dict(preds=[_rec(0, "a", FAR, score=0.9), _rec(0, "a", A, score=0.8)],
                                   gts=[_rec(0, "a", A), _rec(0, "a", B)], AP=0.5 * 51.0 / 101.0, AR=0.5),
    # A false positive scored BELOW the true positive changes nothing at the sampled points: sorted [TP, FP], recall = [1, 1],
    # precision = [1, 1/2]; every point finds index 0.  AP = 1.
    "fp_below_tp": dict(preds=[_rec(0, "a", A, score=0.9), _rec(0, "a", FAR, score=0.1)], gts=[_rec(0, "a", A)], AP=1.0, AR=1.0),
    # An ignored ground truth (B) and a prediction on it: matched to an ignored ground truth, the prediction is ignored -- neither
    # true nor false positive -- and B does not count as a ground truth.  What is left is "one_on_one".  AP = 1.
    "ignored_gt": dict(preds=[_rec(0, "a", A, score=0.9), _rec(0, "a", B, score=0.95)], gts=[_rec(0, "a", A), _rec(0, "a", B, ignore=True)],
                       AP=1.0, AR=1.0),
    # Two labels: "a" as one_on_one (AP 1), "b" as one_of_two (AP 51/101); a prediction on a frame without any ground truth of its
    # label "c" belongs to no counted label.  AP = mean over labels = (1 + 51/101) / 2.  AR = (1 + 1/2) / 2.
    "two_labels": dict(preds=[_rec(0, "a", A, score=0.9), _rec(0, "b", A, score=0.9), _rec(1, "c", A, score=0.9)],
                       gts=[_rec(0, "a", A), _rec(0, "b", A), _rec(0, "b", B)], AP=(1.0 + 51.0 / 101.0) / 2.0, AR=0.75),
    # A prediction on the right place with the wrong label never meets the ground truth: label "a" has one ground truth and no
    # detection, its curve is empty.  AP = 0.  AR = 0.
    "wrong_label": dict(preds=[_rec(0, "b", A, score=0.9)], gts=[_rec(0, "a", A)], AP=0.0, AR=0.0),
}


# ---- box inputs of the GPU test and their tolerance --------------------------------------------------------------------------------
def box_cases():
    """``(boxes1 [n, 4], boxes2 [n, 4])`` float32, compared row by row: the special cases first, then seeded boxes."""
    special = [((0, 0, 10, 10), (0, 0, 10, 10)),                  # identical: 1
               ((0, 0, 10, 10), (2, 3, 5, 6)),                    # contained: 9 / 100
               ((0, 0, 10, 10), (10, 0, 20, 10)),                 # touching along an edge: 0
               ((0, 0, 10, 10), (30, 40, 50, 60)),                # disjoint: 0
               ((-20.5, -7.25, -3.0, 4.5), (-10.0, -3.5, 6.0, 9.0)),  # negative coordinates
               ((5, 0, 5, 10), (0, 0, 10, 10)),                   # zero width: 0 / 100
               ((3, 3, 3, 3), (3, 3, 3, 3)),                      # two zero-area boxes: 0 / 0 = NaN
               ((1, 2, 1, 9), (4, 4, 8, 4))]                      # two zero-area boxes apart: NaN
    rs = np.random.RandomState(11)
    n = 500
    x1, y1 = rs.uniform(-50, 600, n), rs.uniform(-50, 440, n)
    a = np.stack([x1, y1, x1 + rs.uniform(0.5, 200, n), y1 + rs.uniform(0.5, 200, n)], axis=1)
    shift = rs.uniform(-60, 60, (n, 2))
    grow = rs.uniform(0.5, 1.5, (n, 2))
    b = np.stack([a[:, 0] + shift[:, 0], a[:, 1] + shift[:, 1], a[:, 0] + shift[:, 0] + (a[:, 2] - a[:, 0]) * grow[:, 0],
                  a[:, 1] + shift[:, 1] + (a[:, 3] - a[:, 1]) * grow[:, 1]], axis=1)
    b1 = np.concatenate([np.asarray([s[0] for s in special], dtype=np.float64), a]).astype(np.float32)
    b2 = np.concatenate([np.asarray([s[1] for s in special], dtype=np.float64), b]).astype(np.float32)
    return b1, b2


def box_rows(b1, b2, dtype):
    return np.asarray([box_iou(b1[i:i + 1], b2[i:i + 1], dtype=dtype)[0, 0] for i in range(len(b1))])


def box_bound():
    """``(ref64, measured, bound)`` on :func:`box_cases`: the float64 IoUs of the float32 boxes, the largest error of the float32
    restatement of the formula against them, and what the kernel is allowed: 4 x that."""
    b1, b2 = box_cases()
    ref64, ref32 = box_rows(b1, b2, np.float64), box_rows(b1, b2, np.float32)
    assert np.array_equal(np.isnan(ref64), np.isnan(ref32))
    measured = float(np.nanmax(np.abs(ref32.astype(np.float64) - ref64)))
    return ref64, measured, 4.0 * measured


# ---- the frames of the end-to-end meter test ---------------------------------------------------------------------------------------
def _shape_mask(h, w, kind, cx, cy, rx, ry):
    y, x = np.mgrid[0:h, 0:w]
    if kind == "rect":
        return (np.abs(x - cx) <= rx) & (np.abs(y - cy) <= ry)
    return ((x - cx) / (rx + 0.5)) ** 2 + ((y - cy) / (ry + 0.5)) ** 2 <= 1.0


def _record(view, label, mask, **more):
    ys, xs = np.where(mask)
    box = (float(xs.min()), float(ys.min()), float(xs.max() + 1), float(ys.max() + 1))
    return {"scene_id": 0, "view_id": view, "label": label, "mask": mask, "box": box, **more}


def meter_frames(seed=5, n_frames=6, h=60, w=80):
    """``(preds, gts)`` record lists: rectangles and ellipses as ground truth; predictions are the ground truths shifted and
    grown, duplicated with lower scores, partly mislabelled, plus one on a frame without ground truth.  All scores differ."""
    rs = np.random.RandomState(seed)
    labels = ["a", "b", "c"]
    gts, preds = [], []
    for view in range(n_frames):
        for _ in range(rs.randint(2, 5)):
            shape = (rs.choice(["rect", "ellipse"]), rs.randint(12, w - 12), rs.randint(10, h - 10), rs.randint(4, 11), rs.randint(3, 9))
            label = labels[rs.randint(3)]
            gts.append(_record(view, label, _shape_mask(h, w, *shape), ignore=False))
            kind, cx, cy, rx, ry = shape
            for copy in range(rs.randint(0, 4)):  # 0: missed; 1: found; 2 - 3: duplicates
                moved = (kind, cx + rs.randint(-3, 4), cy + rs.randint(-2, 3), rx + rs.randint(-1, 3), ry + rs.randint(-1, 2))
                wrong = rs.rand() < 0.15
                preds.append(_record(view, labels[(labels.index(label) + 1) % 3] if wrong else label, _shape_mask(h, w, *moved)))
    preds.append(_record(n_frames + 3, "a", _shape_mask(h, w, "rect", 30, 30, 6, 5)))
    scores = rs.permutation(len(preds))
    for r, s in zip(preds, scores):
        r["score"] = float(0.05 + 0.9 * s / len(preds))
    return preds, gts
