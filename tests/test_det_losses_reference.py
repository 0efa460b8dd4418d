"""The float64 restatement of the detector's targets and losses (tests/det_losses_ref.py) against cases worked out by hand, and
the conditions the GPU tests' inputs must meet.  No GPU."""

import math

import numpy as np

import det_losses_ref as R


def test_tied_anchors_are_both_restored_as_low_quality_matches():
    """Ground truth (0, 0, 4, 4), area 16.  Anchor (-2, 0, 2, 4): intersection 2 x 4 = 8, union 16 + 16 - 8 = 24, IoU 1 / 3; anchor
    (2, 0, 6, 4) the same by symmetry.  1 / 3 lies between 0.3 and 0.7 (-2 before the restore) and is the ground truth's maximum
    for both: with low-quality matches both come back as 0; without, both stay -2.  The third anchor misses: -1."""
    c = R.hand_tie_case()
    for dtype in (np.float64, np.float32):
        m, iou, und = R.assign(c["boxes"], c["image_of"], c["gt"], c["gt_off"], 0.7, 0.3, True, dtype, exact_ties=True)
        assert m.tolist() == [0, 0, -1] and not und.any()
        assert iou[0] == iou[1] == dtype(8) / dtype(24) and iou[2] == 0
        m, _, und = R.assign(c["boxes"], c["image_of"], c["gt"], c["gt_off"], 0.7, 0.3, False, dtype, exact_ties=True)
        assert m.tolist() == [-2, -2, -1] and not und.any()


def test_thresholds_are_closed_below():
    """Ground truth (0, 0, 10, 10), area 100.  Anchors inside it: (0, 0, 10, 3) -> 30 / 100 = 0.3: not < low, so -2;
    (0, 0, 10, 7) -> 0.7: >= high, matched; (0, 0, 5, 5) -> 0.25: -1.  The quotients are the format's nearest value to 0.3 and
    0.7, which is what the threshold literal is too."""
    boxes = np.asarray([[0, 0, 10, 3], [0, 0, 10, 7], [0, 0, 5, 5]], np.float32)
    gt = np.asarray([[0, 0, 10, 10]], np.float32)
    for dtype in (np.float64, np.float32):
        m, iou, _ = R.assign(boxes, np.zeros(3, np.int32), gt, [0, 1], 0.7, 0.3, False, dtype, exact_ties=True)
        assert m.tolist() == [-2, 0, -1]
        assert iou.tolist() == [dtype(0.3), dtype(0.7), dtype(0.25)]


def test_image_without_ground_truths_is_background():
    boxes = R.random_boxes(np.random.default_rng(0), 6)
    gt = np.asarray([[0, 0, 96, 64]], np.float32)
    m, iou, _ = R.assign(boxes, np.asarray([0, 0, 0, 1, 1, 1]), gt, [0, 0, 1], 0.5, 0.5, True)
    assert (m[:3] == -1).all() and (iou[:3] == 0).all() and (m[3:] != -1).any()


def test_sample_counts_when_a_class_runs_short():
    """256 per image at 0.5: 3 positives, 300 negatives -> 3 and 253; 200 positives, 10 negatives -> 128 and 10.
    512 at 0.25: 0 positives -> 0 and min(n_neg, 512)."""
    assert R.sample_counts(3, 300, 256, 0.5) == (3, 253)
    assert R.sample_counts(200, 10, 256, 0.5) == (128, 10)
    assert R.sample_counts(0, 1000, 512, 0.25) == (0, 512)
    labels = np.asarray([1] * 3 + [0] * 300 + [-1] * 5 + [1] * 200 + [0] * 10)
    image_of = np.asarray([0] * 308 + [1] * 210)
    (p0, n0), (p1, n1) = R.sample(labels, image_of, 2, 256, 0.5, seed=5, stream=1)
    assert p0.tolist() == [0, 1, 2] and n0.size == 253 and (labels[n0] == 0).all() and (np.diff(n0) > 0).all()
    assert p1.size == 128 and n1.tolist() == list(range(508, 518)) and (labels[p1] == 1).all() and p1.min() >= 308
    keys = R.sample_keys(image_of, 5, 1)
    kept, dropped = keys[p1], keys[np.setdiff1d(np.arange(308, 508), p1)]
    assert kept.max() <= dropped.min()
    # a row's key is a function of (index within its image, image): image 1 alone gives the same keys
    assert (R.sample_keys(np.ones(210, np.int64), 5, 1) == keys[308:]).all()


def test_box_encode_by_hand():
    """Proposal (0, 0, 10, 20): w 10, h 20, centre (5, 10).  Reference (2, 4, 12, 14): w 10, h 10, centre (7, 9).  Weights
    (10, 10, 5, 5): dx = 10 (7 - 5) / 10 = 2, dy = 10 (9 - 10) / 20 = -0.5, dw = 5 log 1 = 0, dh = 5 log 0.5."""
    out = R.box_encode([[0, 0, 10, 20]], [0], [[2, 4, 12, 14]], (10, 10, 5, 5))
    assert np.allclose(out, [[2, -0.5, 0, 5 * math.log(0.5)]], rtol=0, atol=1e-15)


def test_smooth_l1_on_both_sides_of_beta():
    """beta = 1 / 9.  d = 0.05 < beta: 0.5 d^2 / beta = 0.01125, slope d / beta = 0.45; d = -0.5: |d| - beta / 2 = 4 / 9, slope -1.
    One sampled positive row, n_sampled = 1: the loss is the sum over its four values / 1."""
    lo, lb, go, gb = R.rpn_loss([0.0], [[0.05, -0.5, 0.0, 0.0]], [1], [[0, 0, 0, 0]], [0])
    assert abs(lb - (0.01125 + 4 / 9)) < 1e-15 and np.allclose(gb, [[0.45, -1, 0, 0]], rtol=0, atol=1e-15)
    assert abs(lo - math.log(2)) < 1e-15 and abs(go[0] + 0.5) < 1e-15  # BCE(0, 1) = log 2, sigmoid(0) - 1 = -0.5


def test_one_row_softmax():
    """logits (1, 2, 3), label 2: loss = log(e^-2 + e^-1 + 1), gradient = softmax - one-hot; a padding column is ignored."""
    s = math.exp(-2) + math.exp(-1) + 1
    lc, lb, gc, gr = R.fastrcnn_loss([[1.0, 2.0, 3.0, 99.0]], np.zeros((1, 12)), [2], np.zeros((1, 4)), 3)
    assert abs(lc - math.log(s)) < 1e-15 and lb == 0
    assert np.allclose(gc, [[math.exp(-2) / s, math.exp(-1) / s, 1 / s - 1, 0]], rtol=0, atol=1e-15)


def test_roi_align_small_and_outside():
    """A 4 x 4 mask of ones, M = 2.
    roi (1, 1, 1.5, 1.5) is smaller than one bin: its width is raised to 1, bins of 0.5, one sample per bin at 1.25 and 1.75: 1.
    roi (-4, 0, 4, 4): width 8, bins of 4, ceil(8 / 2) = 4 samples per bin along x at -3.5, -2.5, -1.5 (left of -1: 0), -0.5 (clamped
    to 0: 1) in bin 0 and 0.5 .. 3.5 (1) in bin 1; along y two samples per bin, all inside: [[0.25, 1], [0.25, 1]]."""
    ones = np.ones((1, 4, 4), np.uint8)
    for dtype in (np.float64, np.float32):
        out = R.mask_targets(ones, [0, 0], [[1, 1, 1.5, 1.5], [-4, 0, 4, 4]], 2, dtype)
        assert out[0].tolist() == [[1, 1], [1, 1]] and out[1].tolist() == [[0.25, 1], [0.25, 1]]


def test_gpu_assignment_cases_are_decidable():
    """What tests/test_gpu_det_losses.py requires of its inputs: the reference leaves out at most 0.5 % of a case's rows (rows
    within 1e-5 of a threshold or of a contested maximum), and none of the hand-tie case."""
    cases = R.assign_cases()
    assert {"canvas-gt0", "canvas-gt1", "canvas-gt3", "canvas-gt9", "random-1", "random-63", "random-64", "random-65", "random-257",
            "random-1025", "hand-tie"} == set(cases)
    assert cases["canvas-gt0"]["boxes"].shape == (3 * 1536, 4)
    for name, c in cases.items():
        for allow in (False, True):
            for high, low in ((0.7, 0.3), (0.5, 0.5)):
                m64, _, und = R.assign(c["boxes"], c["image_of"], c["gt"], c["gt_off"], high, low, allow, exact_ties=c["exact_ties"])
                assert und.sum() <= 0.005 * und.size, (name, allow, high, int(und.sum()))
                if name == "hand-tie":
                    assert not und.any()
                # the float32 evaluation of the restatement decides every other row the same way
                m32 = R.assign(c["boxes"], c["image_of"], c["gt"], c["gt_off"], high, low, allow, np.float32, exact_ties=c["exact_ties"])[0]
                assert (m32[~und] == m64[~und]).all(), (name, allow, high)
