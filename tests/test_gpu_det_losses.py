"""The detector's training targets and losses on the device (csrc/det_losses.hip, happypose_amd.detection_losses,
happypose_amd.training.h_maskrcnn) against the float64 restatement tests/det_losses_ref.py.  torchvision cannot be run here:
parity with it is unpinned, the restatement is the yardstick.  Bounds are 4 x the restatement's own float32-vs-float64 distance
on the case, floor one float32 ulp of the largest entry; every measured figure is printed before it is asserted."""

import numpy as np
import pytest
import torch

import det_losses_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def check(name, got, ref64, ref32):
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    b = R.bound(ref64, ref32)
    assert (np.isfinite(got) == np.isfinite(ref64)).all(), name
    fin = np.isfinite(ref64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref64)[fin].max() if fin.any() else 0.0
    print(f"{name}: error {err:.3e} bound {b:.3e}")
    assert err <= b, (name, err, b)


# ---- assignment ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def assign_cases():
    return R.assign_cases()


@pytest.mark.parametrize("name", ["canvas-gt0", "canvas-gt1", "canvas-gt3", "canvas-gt9", "random-1", "random-63", "random-64", "random-65",
                                  "random-257", "random-1025", "hand-tie"])
def test_assign_is_exact(assign_cases, name):
    from happypose_amd import ops

    c = assign_cases[name]
    for allow in (False, True):
        for high, low in ((0.7, 0.3), (0.5, 0.5)):
            m64, iou64, und = R.assign(c["boxes"], c["image_of"], c["gt"], c["gt_off"], high, low, allow, exact_ties=c["exact_ties"])
            iou32 = R.assign(c["boxes"], c["image_of"], c["gt"], c["gt_off"], high, low, allow, np.float32, exact_ties=c["exact_ties"])[1]
            assert und.sum() <= 0.005 * und.size and (name != "hand-tie" or not und.any())
            match, iou = ops.det_assign(dev(c["boxes"]), dev(c["image_of"]), dev(c["gt"]).reshape(-1, 4), c["gt_off"], high, low, allow)
            match, iou = match.cpu().numpy(), iou.cpu().numpy()
            assert match.dtype == np.int32 and (match[~und] == m64[~und]).all(), (name, allow, high, np.nonzero(match != m64)[0][:8])
            check(f"iou {name} allow={allow} {high}/{low}", iou, iou64, iou32)
            again = ops.det_assign(dev(c["boxes"]), dev(c["image_of"]), dev(c["gt"]).reshape(-1, 4), c["gt_off"], high, low, allow)
            assert again[0].cpu().numpy().tobytes() == match.tobytes() and again[1].cpu().numpy().tobytes() == iou.tobytes()


def test_assign_argument_errors():
    from happypose_amd import ops

    boxes, gt = dev(np.zeros((4, 4), np.float32)), dev(np.zeros((1, 4), np.float32))
    with pytest.raises(AssertionError):
        ops.det_assign(boxes, [0, 0, 0, 2], gt, [0, 1], 0.5, 0.5)        # image 2 of 1
    with pytest.raises(AssertionError):
        ops.det_assign(boxes, dev([0, 0, 0, 2]), gt, [0, 1], 0.5, 0.5)   # the same ids on the device
    with pytest.raises(AssertionError):
        ops.det_assign(boxes, [0] * 4, gt, [0, 1], 0.3, 0.7)             # low above high
    with pytest.raises(ValueError):
        ops.det_assign(boxes.cpu(), [0] * 4, gt, [0, 1], 0.5, 0.5)
    m, iou = ops.det_assign(boxes[:0], [], gt, [0, 1], 0.5, 0.5)
    assert m.shape == (0,) and iou.shape == (0,)


# ---- sampling ------------------------------------------------------------------------------------------------------------------------
def test_sample_keys_are_philox():
    from happypose_amd import ops

    zero = ops.det_sample_keys(dev([0], torch.int32), 1, seed=0, stream=0)
    assert int(zero[0]) == 0x6627E8D5  # Random123's known answer for counter 0, key 0 (tests/test_mesh_sample_reference.py), word 0
    image_of = np.asarray([0] * 70 + [2] * 5 + [1] * 300 + [2] * 3, np.int32)  # image 2 in two runs
    seed = 0x0123456789ABCDEF
    keys = ops.det_sample_keys(dev(image_of), 3, seed, stream=2).cpu().numpy()
    assert (keys == R.sample_keys(image_of, seed, 2)).all()
    assert (ops.det_sample_keys(dev(image_of), 3, seed, stream=2).cpu().numpy() == keys).all()
    # a row's key does not depend on the other images
    alone = ops.det_sample_keys(dev(np.ones(300, np.int32)), 3, seed, stream=2).cpu().numpy()
    assert (alone == keys[75:375]).all()


@pytest.mark.parametrize("batch,fraction", [(256, 0.5), (512, 0.25)])
def test_sample_selection_equals_the_reference(batch, fraction):
    from happypose_amd import ops

    rng = np.random.default_rng(batch)
    labels = np.concatenate([rng.choice([-1, 0, 1, 3], 1536, p=[0.1, 0.8, 0.05, 0.05]), rng.choice([0, 2], 700, p=[0.2, 0.8]),
                             np.zeros(40, np.int64)])  # positives short, negatives short, no positives
    image_of = np.repeat([0, 1, 2], [1536, 700, 40]).astype(np.int32)
    ref = R.sample(labels, image_of, 3, batch, fraction, seed=11, stream=1)
    got = ops.det_sample(dev(labels), dev(image_of), 3, batch, fraction, seed=11, stream=1)
    again = ops.det_sample(dev(labels), dev(image_of), 3, batch, fraction, seed=11, stream=1)
    for (rp, rn), (gp, gn), (ap, an) in zip(ref, got, again):
        assert gp.cpu().tolist() == rp.tolist() and gn.cpu().tolist() == rn.tolist()
        assert ap.cpu().tolist() == rp.tolist() and an.cpu().tolist() == rn.tolist()
    other = ops.det_sample(dev(labels), dev(image_of), 3, batch, fraction, seed=12, stream=1)
    assert other[0][1].cpu().tolist() != ref[0][1].tolist()


# ---- box encoding and mask targets ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)])
def test_box_encode(weights):
    from happypose_amd import ops

    rng = np.random.default_rng(3)
    boxes, gt = R.random_boxes(rng, 1025), R.random_boxes(rng, 9)
    match = rng.integers(-2, 9, 1025).astype(np.int32)
    got = ops.det_box_encode(dev(boxes), dev(match), dev(gt), weights).cpu().numpy()
    ref64, ref32 = R.box_encode(boxes, match, gt, weights), R.box_encode(boxes, match, gt, weights, np.float32)
    assert (np.isneginf(got[match < 0][:, 2:])).all()  # the zero box: log 0
    check(f"box_encode {weights}", got, ref64, ref32)


def _mask_case(h, w, n, seed):
    rng = np.random.default_rng(seed)
    masks = np.zeros((4, h, w), np.uint8)
    yy, xx = np.mgrid[:h, :w]
    for g in range(4):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(5, 20)
        masks[g] = ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r)
    sizes = np.exp(rng.uniform(np.log(0.4), np.log(60), (n, 2)))  # 0.4 .. 60 px: adaptive ratios 1 .. 3 at M = 28
    sizes[0] = (0.4, 60.0)
    c = rng.uniform((0, 0), (w, h), (n, 2))
    rois = np.concatenate([c - sizes / 2, c + sizes / 2], 1).astype(np.float32)
    if n > 1:
        rois[1] = (w + 10, h + 5, w + 30, h + 40)  # outside the frame
    return masks, rng.integers(0, 4, n).astype(np.int32), rois


@pytest.mark.parametrize("h,w", [(37, 53), (48, 64)])
@pytest.mark.parametrize("n", [1, 7, 33])
@pytest.mark.parametrize("M", [28, 5])
def test_mask_targets(h, w, n, M):
    from happypose_amd import detection_losses as L

    masks, match, rois = _mask_case(h, w, n, 100 * n + M)
    got = L.project_masks_on_boxes(dev(masks), dev(rois), dev(match), M).cpu().numpy()
    ref64, ref32 = R.mask_targets(masks, match, rois, M), R.mask_targets(masks, match, rois, M, np.float32)
    if n > 1:
        assert (got[1] == 0).all()
    check(f"mask_targets {h}x{w} n={n} M={M}", got, ref64, ref32)


# ---- the losses ----------------------------------------------------------------------------------------------------------------------
def _rpn_case(n_sampled_per_image, n_images, seed, scale=2.0, positives=True):
    rng = np.random.default_rng(seed)
    A = 1536 * 2
    obj = (rng.standard_normal(A) * scale).astype(np.float32)
    deltas = (rng.standard_normal((A, 4)) * 0.3).astype(np.float32)
    targets = (rng.standard_normal((A, 4)) * 0.3).astype(np.float32)
    targets[::3] = deltas[::3] + np.float32(0.05) * rng.standard_normal((len(deltas[::3]), 4)).astype(np.float32)  # inside beta
    labels = rng.choice([-1, 0, 1], A, p=[0.1, 0.6, 0.3]).astype(np.int32) if positives else np.zeros(A, np.int32)
    sampled = np.concatenate([i * 1536 + rng.choice(np.nonzero(labels[i * 1536:(i + 1) * 1536] >= 0)[0], n_sampled_per_image, replace=False)
                              for i in range(n_images)]).astype(np.int32)
    return obj, deltas, labels, targets, sampled


def _run_rpn(case):
    from happypose_amd import ops

    obj, deltas, labels, targets, sampled = case
    loss, g_obj, g_del = ops.loss_rpn(dev(obj), dev(deltas), dev(labels), dev(targets), dev(sampled))
    return loss.cpu().numpy(), g_obj.cpu().numpy(), g_del.cpu().numpy()


def _check_rpn(name, case):
    got = _run_rpn(case)
    r64, r32 = R.rpn_loss(*case), R.rpn_loss(*case, dtype=torch.float32)
    for i, part in enumerate(("objectness", "box")):
        check(f"rpn {name} loss_{part}", got[0][i], r64[i], r32[i])
        check(f"rpn {name} grad_{part}", got[1 + i], r64[2 + i], r32[2 + i])
    return got


@pytest.mark.parametrize("per_image,n_images", [(1, 1), (64, 1), (256, 1), (256, 2)])
def test_loss_rpn(per_image, n_images):
    case = _rpn_case(per_image, n_images, seed=per_image + n_images)
    got = _check_rpn(f"{per_image}x{n_images}", case)
    again = _run_rpn(case)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    untouched = np.setdiff1d(np.arange(3072), case[4])
    assert (got[1][untouched] == 0).all() and (got[2][untouched] == 0).all()


def test_loss_rpn_edges():
    from happypose_amd import detection_losses as L

    big = list(_rpn_case(256, 2, seed=9))
    big[0] = np.where(np.arange(3072) % 2 == 0, 80.0, -80.0).astype(np.float32)
    got = _check_rpn("logits +-80", tuple(big))
    assert np.isfinite(got[0]).all()
    none = _rpn_case(256, 2, seed=10, positives=False)
    got = _check_rpn("no positives", none)
    assert got[0][1] == 0 and (got[2] == 0).all()
    # one NaN row: the loss is NaN, the neighbours' gradients come back bit for bit
    case = _rpn_case(256, 2, seed=11)
    clean = _run_rpn(case)
    obj = case[0].copy()
    row = case[4][5]
    obj[row] = np.nan
    bad = _run_rpn((obj,) + case[1:])
    assert np.isnan(bad[0][0]) and np.isnan(bad[1][row])
    keep = np.arange(3072) != row
    assert bad[1][keep].tobytes() == clean[1][keep].tobytes() and bad[2].tobytes() == clean[2].tobytes() and bad[0][1] == clean[0][1]
    # a non-unit upstream gradient through the public function
    o, d = dev(case[0]).requires_grad_(), dev(case[1]).requires_grad_()
    labels = [dev(case[2][:1536]).float(), dev(case[2][1536:]).float()]
    targets = [dev(case[3][:1536]), dev(case[3][1536:])]
    lo, lb, sampled = L.rpn_compute_loss(o, d, labels, targets, seed=4, return_sampled=True)
    (2.5 * lo + 0.5 * lb).backward()
    unit = _run_rpn(case[:4] + (sampled.cpu().numpy(),))
    assert o.grad.cpu().numpy().tobytes() == (unit[1] * np.float32(2.5)).tobytes()
    assert d.grad.cpu().numpy().tobytes() == (unit[2] * np.float32(0.5)).tobytes()
    ref = R.sample(case[2], np.repeat([0, 1], 1536), 2, 256, 0.5, 4, L.STREAM_RPN)
    assert sampled.cpu().tolist() == np.concatenate([p for p, _ in ref] + [n for _, n in ref]).tolist()
    with pytest.raises(ValueError):
        L.rpn_compute_loss(o.detach().cpu(), d, labels, targets)


def _frcnn_case(n, C, seed, scale=2.0, positives=True):
    rng = np.random.default_rng(seed)
    ld = (C + 3) // 4 * 4
    logits = (rng.standard_normal((n, ld)) * scale).astype(np.float32)
    reg = (rng.standard_normal((n, 4 * C)) * 0.3).astype(np.float32)
    labels = (rng.integers(0, C, n) * (rng.random(n) < 0.5)).astype(np.int32) if positives else np.zeros(n, np.int32)
    targets = (rng.standard_normal((n, 4)) * 0.3).astype(np.float32)
    return logits, reg, labels, targets, C


def _run_frcnn(case):
    from happypose_amd import ops

    logits, reg, labels, targets, C = case
    loss, g_cls, g_reg = ops.loss_fastrcnn(dev(logits), dev(reg), dev(labels), dev(targets), C)
    return loss.cpu().numpy(), g_cls.cpu().numpy(), g_reg.cpu().numpy()


def _check_frcnn(name, case):
    got = _run_frcnn(case)
    r64, r32 = R.fastrcnn_loss(*case), R.fastrcnn_loss(*case, dtype=torch.float32)
    for i, part in enumerate(("classifier", "box")):
        check(f"fastrcnn {name} loss_{part}", got[0][i], r64[i], r32[i])
        check(f"fastrcnn {name} grad_{part}", got[1 + i], r64[2 + i], r32[2 + i])
    assert (got[1][:, case[4]:] == 0).all()  # padding columns
    return got


@pytest.mark.parametrize("n", [1, 63, 65, 512])
@pytest.mark.parametrize("C", [2, 5, 22])
def test_loss_fastrcnn(n, C):
    case = _frcnn_case(n, C, seed=n + C)
    got = _check_frcnn(f"n={n} C={C}", case)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, _run_frcnn(case)))


def test_loss_fastrcnn_edges():
    from happypose_amd import detection_losses as L

    big = list(_frcnn_case(65, 5, seed=1))
    big[0] = np.where(np.random.default_rng(2).random(big[0].shape) < 0.5, 80.0, -80.0).astype(np.float32)
    assert np.isfinite(_check_frcnn("logits +-80", tuple(big))[0]).all()
    got = _check_frcnn("no positives", _frcnn_case(65, 5, seed=3, positives=False))
    assert got[0][1] == 0 and (got[2] == 0).all()
    case = _frcnn_case(65, 5, seed=4)
    clean = _run_frcnn(case)
    logits = case[0].copy()
    logits[7, 1] = np.nan
    bad = _run_frcnn((logits,) + case[1:])
    keep = np.arange(65) != 7
    assert np.isnan(bad[0][0]) and np.isnan(bad[1][7, :5]).all() and bad[0][1] == clean[0][1]
    assert bad[1][keep].tobytes() == clean[1][keep].tobytes() and bad[2].tobytes() == clean[2].tobytes()
    x, r = dev(case[0]).requires_grad_(), dev(case[1]).requires_grad_()
    lc, lb = L.fastrcnn_loss(x, r, [dev(case[2][:30]), dev(case[2][30:])], [dev(case[3][:30]), dev(case[3][30:])], num_classes=5)
    assert lc.item() == clean[0][0] and lb.item() == clean[0][1]
    (3.0 * lc + 0.25 * lb).backward()
    assert x.grad.cpu().numpy().tobytes() == (clean[1] * np.float32(3.0)).tobytes()
    assert r.grad.cpu().numpy().tobytes() == (clean[2] * np.float32(0.25)).tobytes()
    with pytest.raises(AssertionError):
        L.fastrcnn_loss(x, r, [dev(np.full(65, 5, np.int32))], [dev(case[3])], num_classes=5)  # label outside the classes
    with pytest.raises(ValueError):
        L.fastrcnn_loss(x.detach().cpu(), r, [dev(case[2])], [dev(case[3])], num_classes=5)


def _mask_loss_case(n, C, seed, scale=2.0):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((n, C, 28, 28)) * scale).astype(np.float32), rng.integers(0, C, n).astype(np.int32),
            rng.random((n, 28, 28)).astype(np.float32))


def _run_mask(case):
    from happypose_amd import ops

    loss, grad = ops.loss_mask(dev(case[0]), dev(case[1]), dev(case[2]))
    return loss.cpu().numpy(), grad.cpu().numpy()


def _check_mask(name, case):
    got = _run_mask(case)
    r64, r32 = R.mask_loss(*case), R.mask_loss(*case, dtype=torch.float32)
    check(f"mask {name} loss", got[0][0], r64[0], r32[0])
    check(f"mask {name} grad", got[1], r64[1], r32[1])
    return got


@pytest.mark.parametrize("n", [0, 1, 7, 33])
@pytest.mark.parametrize("C", [2, 5])
def test_loss_mask(n, C):
    case = _mask_loss_case(n, C, seed=10 * n + C)
    got = _check_mask(f"n={n} C={C}", case)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, _run_mask(case)))
    if n == 0:
        assert got[0][0] == 0
    other = np.ones((n, C), bool)
    other[np.arange(n), case[1]] = False
    assert (got[1][other] == 0).all()  # non-zero in the label's channel only


def test_loss_mask_edges():
    from happypose_amd import detection_losses as L

    big = list(_mask_loss_case(7, 2, seed=1))
    big[0] = np.where(np.random.default_rng(2).random(big[0].shape) < 0.5, 80.0, -80.0).astype(np.float32)
    assert np.isfinite(_check_mask("logits +-80", tuple(big))[0]).all()
    case = _mask_loss_case(7, 2, seed=3)
    clean = _run_mask(case)
    logits = case[0].copy()
    logits[3, case[1][3], 5, 6] = np.nan
    bad = _run_mask((logits,) + case[1:])
    keep = np.arange(7) != 3
    assert np.isnan(bad[0][0]) and bad[1][keep].tobytes() == clean[1][keep].tobytes()
    # through the public function: masks projected on boxes, a non-unit upstream, and the image without objects
    masks, match, rois = _mask_case(48, 64, 7, seed=5)
    labels_gt = np.asarray([1, 1, 0, 1], np.int64)
    x = dev(case[0]).requires_grad_()
    empty = dict(m=torch.zeros((0, 48, 64), dtype=torch.uint8, device=DEV), p=torch.zeros((0, 4), device=DEV),
                 l=torch.zeros(0, dtype=torch.int64, device=DEV))
    loss, labels, targets = L.maskrcnn_loss(x, [dev(rois), empty["p"]], [dev(masks), empty["m"]], [dev(labels_gt), empty["l"]],
                                            [dev(match).long(), empty["l"]], return_targets=True)
    assert labels.cpu().tolist() == labels_gt[match].tolist()
    unit = _run_mask((case[0], labels_gt[match].astype(np.int32), targets.cpu().numpy()))
    assert loss.item() == unit[0][0]
    (1.5 * loss).backward()
    assert x.grad.cpu().numpy().tobytes() == (unit[1] * np.float32(1.5)).tobytes()
    none = L.maskrcnn_loss(dev(case[0][:0]).requires_grad_(), [empty["p"]], [empty["m"]], [empty["l"]], [empty["l"]])
    assert none.item() == 0
    none.backward()
    with pytest.raises(ValueError):
        L.maskrcnn_loss(x.detach().cpu(), [dev(rois)], [dev(masks)], [dev(labels_gt)], [dev(match).long()])


# ---- the step ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step():
    from happypose_amd import training
    from happypose_amd.detector import synthetic_maskrcnn

    model = synthetic_maskrcnn(DEV, n_classes=3, input_size=(96, 128))
    rng = np.random.default_rng(0)
    images = [dev(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)) for _ in range(2)]
    masks = np.zeros((2, 96, 128), np.uint8)
    masks[0, 10:50, 20:70] = 1
    masks[1, 40:90, 60:120] = 1
    targets = [dict(boxes=dev(np.asarray([[20, 10, 70, 50], [60, 40, 120, 90]], np.float32)), labels=dev(np.asarray([1, 2], np.int64)),
                    masks=dev(masks)),
               dict(boxes=torch.zeros((0, 4), device=DEV), labels=torch.zeros(0, dtype=torch.int64, device=DEV),
                    masks=torch.zeros((0, 96, 128), dtype=torch.uint8, device=DEV))]
    x = torch.stack(images).permute(0, 3, 1, 2).float() / 255
    before = [model(x[b:b + 1].contiguous()) for b in range(2)]
    cfg = training.DetectorTrainingConfig(rpn_box_reg_alpha=2.0, objectness_alpha=0.5, classifier_alpha=1.5, mask_alpha=3.0, box_reg_alpha=0.25)
    runs = []
    for _ in range(2):
        meters = {k: training.AverageValueMeter() for k in ("loss_rpn_box_reg", "loss_objectness", "loss_box_reg", "loss_classifier", "loss_mask")}
        dbg = {}
        loss = training.h_maskrcnn((images, targets), model, meters, cfg, seed=7, debug_dict=dbg)
        runs.append((loss, meters, dbg))
    after = [model(x[b:b + 1].contiguous()) for b in range(2)]
    return dict(model=model, images=images, targets=targets, cfg=cfg, runs=runs, before=before, after=after)


def test_h_maskrcnn_is_the_hand_composition(step):
    from happypose_amd import detection_losses as L

    loss, meters, d = step["runs"][0]
    t, cfg, B = step["targets"], step["cfg"], 2
    assert list(meters) == ["loss_rpn_box_reg", "loss_objectness", "loss_box_reg", "loss_classifier", "loss_mask"]
    assert d["anchors"].shape == (3 * (24 * 32 + 12 * 16 + 6 * 8 + 3 * 4 + 2 * 2), 4)
    obj = torch.cat([m.detach()[..., :3].reshape(B, -1) for m in d["objectness_maps"]], 1).reshape(-1)
    dlt = torch.cat([m.detach().reshape(B, -1, 4) for m in d["delta_maps"]], 1).reshape(-1, 4)
    lo, lrb, sampled = L.rpn_compute_loss(obj, dlt, d["rpn_labels"], d["rpn_regression_targets"], seed=d["seeds"]["rpn"], return_sampled=True)
    assert sampled.tolist() == d["rpn_sampled"].tolist() and (d["rpn_labels"][1] == 0).all()
    props, midx, labels, rtargets = L.roi_select_training_samples(d["rpn_proposals"], t, seed=d["seeds"]["box"])
    for a, b in zip(props + midx + labels + rtargets, d["proposals"] + d["matched_idxs"] + d["labels"] + d["regression_targets"]):
        assert torch.equal(a, b)
    assert all(p.shape[0] <= 512 for p in props) and (labels[1] == 0).all() and (labels[0] > 0).any()
    lc, lbr = L.fastrcnn_loss(d["class_logits"].detach(), d["box_regression"].detach(), labels, rtargets, num_classes=3)
    lm = L.maskrcnn_loss(d["mask_logits"].detach(), d["mask_proposals"], [x["masks"] for x in t], [x["labels"] for x in t], d["mask_matched_idxs"])
    assert d["mask_logits"].shape[1:] == (3, 28, 28) and d["mask_logits"].shape[0] == int((labels[0] > 0).sum())
    hand = dict(loss_rpn_box_reg=lrb, loss_objectness=lo, loss_box_reg=lbr, loss_classifier=lc, loss_mask=lm)
    for k, v in hand.items():
        print(k, v.item())
        assert np.isfinite(v.item()) and meters[k].n == 1 and meters[k].sum == v.item() and d["losses"][k].item() == v.item(), k
    total = (cfg.rpn_box_reg_alpha * lrb + cfg.objectness_alpha * lo + cfg.box_reg_alpha * lbr + cfg.classifier_alpha * lc + cfg.mask_alpha * lm)
    assert loss.item() == total.item() and loss.is_cuda and loss.shape == ()


def test_h_maskrcnn_gradients_and_repeatability(step):
    from happypose_amd import detection_losses as L

    (loss, _, d), (loss2, meters2, d2) = step["runs"]
    t, cfg, B = step["targets"], step["cfg"], 2
    assert loss.item() == loss2.item()
    for k in ("class_logits", "box_regression", "mask_logits", "rpn_sampled"):
        assert torch.equal(d[k].detach(), d2[k].detach()), k
    leaves = d["objectness_maps"] + d["delta_maps"] + [d["class_logits"], d["box_regression"], d["mask_logits"]]
    assert all(x.requires_grad and x.is_leaf for x in leaves)
    loss.backward()
    # each loss function's own backward with its alpha as the upstream gradient
    om, dm = [m.detach().clone().requires_grad_() for m in d["objectness_maps"]], [m.detach().clone().requires_grad_() for m in d["delta_maps"]]
    obj = torch.cat([m[..., :3].reshape(B, -1) for m in om], 1).reshape(-1)
    dlt = torch.cat([m.reshape(B, -1, 4) for m in dm], 1).reshape(-1, 4)
    lo, lrb = L.rpn_compute_loss(obj, dlt, d["rpn_labels"], d["rpn_regression_targets"], seed=d["seeds"]["rpn"])
    torch.autograd.backward([lo, lrb], [torch.tensor(float(cfg.objectness_alpha), device=DEV), torch.tensor(float(cfg.rpn_box_reg_alpha), device=DEV)])
    for a, b in zip(om + dm, d["objectness_maps"] + d["delta_maps"]):
        assert torch.equal(a.grad, b.grad)
    assert any(bool((m.grad != 0).any()) for m in d["objectness_maps"]) and all(bool((m.grad[..., 3] == 0).all()) for m in d["objectness_maps"])
    x, r = d["class_logits"].detach().clone().requires_grad_(), d["box_regression"].detach().clone().requires_grad_()
    lc, lbr = L.fastrcnn_loss(x, r, d["labels"], d["regression_targets"], num_classes=3)
    torch.autograd.backward([lc, lbr], [torch.tensor(float(cfg.classifier_alpha), device=DEV), torch.tensor(float(cfg.box_reg_alpha), device=DEV)])
    assert torch.equal(x.grad, d["class_logits"].grad) and torch.equal(r.grad, d["box_regression"].grad)
    assert bool((x.grad[:, 3:] == 0).all()) and bool((r.grad != 0).any())
    ml = d["mask_logits"].detach().clone().requires_grad_()
    lm = L.maskrcnn_loss(ml, d["mask_proposals"], [x_["masks"] for x_ in t], [x_["labels"] for x_ in t], d["mask_matched_idxs"])
    lm.backward(torch.tensor(float(cfg.mask_alpha), device=DEV))
    assert torch.equal(ml.grad, d["mask_logits"].grad) and bool((ml.grad != 0).any())


def test_inference_is_untouched_by_a_training_step(step):
    for before, after in zip(step["before"], step["after"]):
        for a, b in zip(before, after):
            assert a.keys() == b.keys()
            for k in a:
                assert torch.equal(a[k], b[k]), k


def test_h_maskrcnn_refuses_other_sizes(step):
    from happypose_amd import training

    images = [torch.zeros((64, 128, 3), dtype=torch.uint8, device=DEV)] * 2
    with pytest.raises(NotImplementedError):
        training.h_maskrcnn((images, step["targets"]), step["model"], {}, step["cfg"])
    with pytest.raises(ValueError):
        training.h_maskrcnn(([i.cpu() for i in step["images"]], step["targets"]), step["model"], {}, step["cfg"])
