"""GPU tests of csrc/det_eval.hip (hp_mask_pack, hp_det_iou, hp_det_match) and of the meters built on them
(evaluation.DetectionMeter, evaluation.CocoMeter, evaluation.scene_ground_truth) against tests/det_eval_ref.py.

Packing, pixel counts, the mask IoU (one float32 rounding of an integer quotient) and the matching are compared by exact equality;
the box IoU within 4x the measured error of a float32 restatement against float64 on the same inputs (``det_eval_ref.box_bound``);
the meters' scores to 1e-12 (integer match tables, float64 accumulation on both sides).
"""

import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import det_eval_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _u64(words: torch.Tensor) -> np.ndarray:
    return words.cpu().numpy().view(np.uint64)


# ---- pack ------------------------------------------------------------------------------------------------------------------------
PLANES = [(1, 1), (7, 9), (8, 8), (5, 13), (30, 40), (480, 640)]


@pytest.mark.parametrize("h,w", PLANES)
@pytest.mark.parametrize("odd_base", [False, True])
def test_mask_pack(dev, h, w, odd_base):
    """Words and areas against a numpy packing.  ``odd_base``: the masks are a slice of a larger buffer that starts at an odd
    byte, which forces the byte-load (ballot) instantiation whatever the plane size."""
    from happypose_amd import ops

    n = 3 if h * w > 10000 else 5
    rs = np.random.RandomState(h * 1000 + w)
    masks = rs.choice(np.array([0, 1, 2, 255], np.uint8), size=(n, h, w), p=[0.55, 0.15, 0.15, 0.15])
    masks[-1] = 0
    if n > 1:
        masks[-2] = 255
    if odd_base:
        buf = torch.zeros(n * h * w + 1, dtype=torch.uint8, device=dev)
        buf[1:] = torch.as_tensor(masks.reshape(-1), device=dev)
        t = buf[1:].view(n, h, w)
        assert t.data_ptr() % 2 == 1 and t.is_contiguous()
    else:
        t = torch.as_tensor(masks, device=dev)
    words, area = ops.mask_pack(t)
    assert words.shape == (n, (h * w + 63) // 64) == (n, ops.mask_pack_words(h, w)) and area.dtype == torch.int32
    want = R.pack_masks(masks)
    assert np.array_equal(_u64(words), want)
    assert np.array_equal(area.cpu().numpy(), (masks != 0).reshape(n, -1).sum(1))
    tail = (h * w) % 64
    if tail:
        assert (_u64(words)[:, -1] >> np.uint64(tail) == 0).all()
    # the storage of a bool tensor qualifies
    wb, ab = ops.mask_pack(torch.as_tensor(masks != 0, device=dev))
    assert torch.equal(wb, words) and torch.equal(ab, area)


def test_mask_pack_empty_and_limits(dev):
    from happypose_amd import ops

    words, area = ops.mask_pack(torch.zeros((0, 5, 13), dtype=torch.bool, device=dev))
    assert words.shape == (0, 2) and area.shape == (0,)
    assert ops.mask_pack_words(4096, 4096) == 2 ** 18
    with pytest.raises(AssertionError):
        ops.mask_pack_words(4096, 4097)  # more than 2^24 pixels: counts would not be exact in float32


# ---- counts ----------------------------------------------------------------------------------------------------------------------
_COUNT_CASES = {}


def _count_case(h, w, n=9):
    """Seeded masks of density 0, 0.01, 0.5 and 1 with their numpy pair counts, computed once."""
    if (h, w) not in _COUNT_CASES:
        rs = np.random.RandomState(h + w)
        dens = [0.0, 0.0, 0.01, 0.5, 1.0, 0.5, 0.01, 0.5, 0.3][:n]
        masks = np.stack([rs.rand(h, w) < d for d in dens])
        flat = masks.reshape(n, -1).astype(np.int64)
        inter = flat @ flat.T
        area = flat.sum(1)
        union = area[:, None] + area[None, :] - inter
        _COUNT_CASES[h, w] = (masks, inter, union)
    return _COUNT_CASES[h, w]


def _check_rows(out, inter, union, i, j):
    got_i, got_u, got = out["inter"].cpu().numpy(), out["union"].cpu().numpy(), out["mask_iou"].cpu().numpy()
    assert got_i.dtype == np.int32 and got.dtype == np.float32
    assert np.array_equal(got_i, inter[i, j]) and np.array_equal(got_u, union[i, j])
    wi, wu = inter[i, j], union[i, j]
    with np.errstate(invalid="ignore"):
        want = np.where(wu == 0, np.float32(0), wi.astype(np.float32) / wu.astype(np.float32)).astype(np.float32)
    assert np.array_equal(got, want)  # one rounding: exact equality


@pytest.mark.parametrize("h,w", [(5, 13), (30, 40), (61, 67)])
def test_det_iou_mask_counts(dev, h, w):
    from happypose_amd import ops

    masks, inter, union = _count_case(h, w)
    n = len(masks)
    packed = ops.mask_pack(torch.as_tensor(masks, device=dev))
    i, j = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    out = ops.det_iou(i, j, packed_pred=packed, packed_gt=packed)
    assert out["box_iou"] is None
    _check_rows(out, inter, union, i, j)
    iou = out["mask_iou"].cpu().numpy().reshape(n, n)
    assert iou[0, 1] == 0.0 and iou[0, 0] == 0.0  # all-empty against all-empty
    assert np.array_equal(np.diag(iou), (np.diag(union) > 0).astype(np.float32)) and np.diag(iou)[3:6].tolist() == [1.0, 1.0, 1.0]  # a mask against itself
    # shuffled rows, repeated indices, a second run: the same integers and bits
    rs = np.random.RandomState(1)
    perm = rs.permutation(n * n)
    _check_rows(ops.det_iou(i[perm], j[perm], packed_pred=packed, packed_gt=packed), inter, union, i[perm], j[perm])
    ri, rj = rs.randint(0, n, 300), np.full(300, 3)
    _check_rows(ops.det_iou(ri, rj, packed_pred=packed, packed_gt=packed), inter, union, ri, rj)
    again = ops.det_iou(i, j, packed_pred=packed, packed_gt=packed)
    for k in ("inter", "union", "mask_iou"):
        assert torch.equal(again[k].view(torch.int32), out[k].view(torch.int32))
    # the all-pairs convenience
    from happypose_amd.evaluation import mask_iou

    assert torch.equal(mask_iou(torch.as_tensor(masks, device=dev), torch.as_tensor(masks[:4], device=dev)), out["mask_iou"].reshape(n, n)[:, :4])


def test_det_iou_70000_rows(dev):
    """More rows than any 16-bit grid dimension holds."""
    from happypose_amd import ops

    masks, inter, union = _count_case(5, 13)
    n = len(masks)
    packed = ops.mask_pack(torch.as_tensor(masks, device=dev))
    rs = np.random.RandomState(2)
    i, j = rs.randint(0, n, 70000), rs.randint(0, n, 70000)
    _check_rows(ops.det_iou(i, j, packed_pred=packed, packed_gt=packed), inter, union, i, j)


def test_det_iou_vga_block(dev):
    """One 100 x 15 block at 480 x 640: rectangles and noise, counts against numpy on the packed words."""
    from happypose_amd import ops

    rs = np.random.RandomState(3)
    h, w = 480, 640

    def make(n):
        m = np.zeros((n, h, w), bool)
        for k in range(n):
            x0, y0 = rs.randint(0, w - 150), rs.randint(0, h - 150)
            m[k, y0:y0 + rs.randint(20, 150), x0:x0 + rs.randint(20, 150)] = True
        m[0] = rs.rand(h, w) < 0.5
        return m

    pred, gt = make(100), make(15)
    pp, pg = ops.mask_pack(torch.as_tensor(pred, device=dev)), ops.mask_pack(torch.as_tensor(gt, device=dev))
    i, j = np.repeat(np.arange(100), 15), np.tile(np.arange(15), 100)
    out = ops.det_iou(i, j, packed_pred=pp, packed_gt=pg)
    fp, fg = pred.reshape(100, -1).astype(np.float32), gt.reshape(15, -1).astype(np.float32)
    inter = (fp @ fg.T).astype(np.int64)  # counts below 2^24: exact in float32
    union = fp.sum(1).astype(np.int64)[:, None] + fg.sum(1).astype(np.int64)[None, :] - inter
    _check_rows(out, inter, union, i, j)
    again = ops.det_iou(i, j, packed_pred=pp, packed_gt=pg)
    assert torch.equal(again["inter"], out["inter"]) and torch.equal(again["mask_iou"].view(torch.int32), out["mask_iou"].view(torch.int32))


def test_det_iou_checks_ids_on_the_host(dev):
    from happypose_amd import ops

    masks, _, _ = _count_case(5, 13)
    packed = ops.mask_pack(torch.as_tensor(masks, device=dev))
    with pytest.raises(AssertionError):
        ops.det_iou([0, len(masks)], [0, 0], packed_pred=packed, packed_gt=packed)
    with pytest.raises(AssertionError):
        ops.det_iou([0], [-1], packed_pred=packed, packed_gt=packed)
    out = ops.det_iou([], [], packed_pred=packed, packed_gt=packed)
    assert out["inter"].shape == (0,) and out["mask_iou"].shape == (0,)


# ---- boxes -----------------------------------------------------------------------------------------------------------------------
def test_det_iou_boxes(dev):
    from happypose_amd import evaluation, ops

    b1, b2 = R.box_cases()
    ref64, measured, bound = R.box_bound()
    n = len(b1)
    out = ops.det_iou(np.arange(n), np.arange(n), boxes_pred=torch.as_tensor(b1, device=dev), boxes_gt=torch.as_tensor(b2, device=dev))
    assert out["mask_iou"] is None and out["inter"] is None
    got = out["box_iou"].cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref64)) and np.isnan(ref64).sum() == 2  # the two zero-area pairs
    err = np.nanmax(np.abs(got.astype(np.float64) - ref64))
    print(f"box_iou: float32 restatement vs float64 {measured:.3e}, bound {bound:.3e}, kernel vs float64 {err:.3e}")
    assert err <= bound
    assert got[0] == 1.0 and got[2] == 0.0 and got[3] == 0.0 and got[5] == 0.0 and abs(got[1] - 0.09) <= bound
    # all pairs, with torchvision's semantics
    full = evaluation.box_iou(torch.as_tensor(b1[:12], device=dev), torch.as_tensor(b2[:9], device=dev)).cpu().numpy()
    want = R.box_iou(b1[:12], b2[:9])
    assert full.shape == (12, 9) and np.array_equal(np.isnan(full), np.isnan(want))
    assert np.nanmax(np.abs(full - want)) <= bound
    assert evaluation.box_iou(torch.zeros((0, 4), device=dev), torch.as_tensor(b2[:3], device=dev)).shape == (0, 3)


def test_det_iou_boxes_and_masks_in_one_call(dev):
    from happypose_amd import ops

    masks, inter, union = _count_case(5, 13)
    n = len(masks)
    packed = ops.mask_pack(torch.as_tensor(masks, device=dev))
    b1, b2 = R.box_cases()
    boxes = torch.as_tensor(b1[:n], device=dev)
    i, j = np.arange(n), np.arange(n)[::-1].copy()
    out = ops.det_iou(i, j, boxes_pred=boxes, boxes_gt=boxes, packed_pred=packed, packed_gt=packed)
    _check_rows(out, inter, union, i, j)
    want = np.asarray([R.box_iou(b1[a:a + 1], b1[b:b + 1])[0, 0] for a, b in zip(i, j)])
    assert np.array_equal(np.isnan(out["box_iou"].cpu().numpy()), np.isnan(want))
    assert np.nanmax(np.abs(out["box_iou"].cpu().numpy() - want)) <= R.box_bound()[2]


# ---- matching --------------------------------------------------------------------------------------------------------------------
def _match(dev, mats, ignores, thresholds):
    from happypose_amd import ops

    iou = np.concatenate([np.asarray(m, np.float32).reshape(-1) for m in mats]) if mats else np.zeros(0, np.float32)
    n_det = [np.asarray(m).shape[0] for m in mats]
    n_gt = [len(g) for g in ignores]
    out = ops.det_match(torch.as_tensor(iou, device=dev), n_det, n_gt, np.concatenate([np.asarray(g, bool) for g in ignores]) if ignores else [],
                        thresholds)
    return {k: v.cpu().numpy() for k, v in out.items()}, n_det, n_gt


def _check_match(got, mats, ignores, thresholds, n_det, n_gt):
    d0 = g0 = 0
    for m, ig, D, G in zip(mats, ignores, n_det, n_gt):
        dm, di, gm = R.coco_match(np.asarray(m, np.float32).reshape(D, G), ig, thresholds)
        assert np.array_equal(got["det_match"][:, d0:d0 + D], dm), (D, G)
        assert np.array_equal(got["det_ignore"][:, d0:d0 + D], di), (D, G)
        assert np.array_equal(got["gt_match"][:, g0:g0 + G], gm), (D, G)
        d0, g0 = d0 + D, g0 + G


def test_det_match_hand_cases(dev):
    nan = np.nan
    mats = [[[0.75, 0.75]],                 # a tie goes to the later ground truth
            [[0.6, 0.9]],                   # an ignored ground truth with the larger IoU loses to a regular one that qualifies
            [[0.4, 0.9]],                   # ... and is taken when no other qualifies: the detection is ignored
            [[0.9], [0.8]],                 # a matched ground truth is not reused
            [[0.5]],                        # IoU exactly equal to the threshold matches
            [[nan, 0.7], [nan, nan]],       # NaN never matches
            [[0.7, 0.7, 0.7, 0.7]]]         # a tie inside each class: the later regular one
    ignores = [[False, False], [False, True], [False, True], [False], [False], [False, False], [False, False, True, True]]
    got, n_det, n_gt = _match(dev, mats, ignores, [0.5])
    assert got["det_match"].tolist() == [[1, 0, 1, 0, -1, 0, 1, -1, 1]]
    assert got["det_ignore"].tolist() == [[False, False, True, False, False, False, False, False, False]]
    assert got["gt_match"].tolist() == [[-1, 0, 0, -1, -1, 0, 0, 0, -1, 0, -1, 0, -1, -1]]
    _check_match(got, mats, ignores, [0.5], n_det, n_gt)


def test_det_match_seeded(dev):
    """IoUs quantised to k / 64: ties and threshold equalities occur and are exact in float32.  Every combination of D in
    {0, 1, 100} and G in {0, 1, 63, 64, 65, 130}, repeated, and a few hundred small groups; all ten thresholds."""
    rs = np.random.RandomState(4)
    shapes = [(D, G) for D in (0, 1, 100) for G in (0, 1, 63, 64, 65, 130)] * 2 + [(rs.randint(0, 6), rs.randint(0, 6)) for _ in range(300)]
    mats, ignores = [], []
    for D, G in shapes:
        m = rs.randint(0, 65, (D, G)) / 64.0
        m[rs.rand(D, G) < 0.5] = 0.0  # sparse, like real frames
        if D and G and rs.rand() < 0.3:
            m[rs.randint(D), rs.randint(G)] = np.nan
        mats.append(m.astype(np.float32))
        ignores.append(np.sort(rs.rand(G) < 0.3))  # the non-ignored ones first
    thr = list(R.COCO_IOU_THRESHOLDS)
    got, n_det, n_gt = _match(dev, mats, ignores, thr)
    assert got["det_match"].shape == (10, sum(n_det)) and got["gt_match"].shape == (10, sum(n_gt))
    _check_match(got, mats, ignores, thr, n_det, n_gt)
    again, _, _ = _match(dev, mats, ignores, thr)
    assert all(np.array_equal(again[k], got[k]) for k in got)


def test_det_match_without_groups(dev):
    got, _, _ = _match(dev, [], [], [0.5, 0.75])
    assert got["det_match"].shape == (2, 0) and got["gt_match"].shape == (2, 0)


# ---- meters ----------------------------------------------------------------------------------------------------------------------
def _collection(records, dev, with_score):
    from happypose_amd.tensor_collection import PandasTensorCollection

    cols = ["scene_id", "view_id", "label"] + (["score"] if with_score else ["ignore"])
    infos = pd.DataFrame([{k: r[k] for k in cols} for r in records], columns=cols)
    boxes = torch.as_tensor(np.asarray([r["box"] for r in records], np.float32).reshape(-1, 4), device=dev)
    masks = torch.as_tensor(np.stack([r["mask"] for r in records]), device=dev)
    return PandasTensorCollection(infos, bboxes=boxes, masks=masks)


@pytest.fixture(scope="module")
def frames():
    return R.meter_frames()


@pytest.mark.parametrize("iou_type", ["bbox", "segm"])
def test_coco_meter(dev, frames, iou_type):
    from happypose_amd.evaluation import CocoMeter

    preds, gts = frames
    want, ious = R.coco_evaluate(preds, gts, iou_type, return_ious=True)
    if iou_type == "bbox":  # no float64 IoU within 1e-4 of a threshold: the float32 boxes cannot flip a match
        gap = np.abs(ious[:, None] - np.asarray(R.COCO_IOU_THRESHOLDS)[None]).min()
        assert gap >= 1e-4, gap
    meter = CocoMeter(iou_type=iou_type)
    views = sorted({r["view_id"] for r in preds + gts})
    for part in (views[:3], views[3:]):  # two add calls; the second holds the frame that has a prediction and no ground truth
        meter.add(_collection([r for r in preds if r["view_id"] in part], dev, True), _collection([r for r in gts if r["view_id"] in part], dev, False))
    summary, dfs = meter.summary()
    print(iou_type, summary, want)
    assert summary["n_pred"] == len(preds) and summary["n_gt"] == len(gts)
    for k in ("AP", "AP50", "AP75", "AR"):
        assert abs(summary[k] - want[k]) <= 1e-12, k
    assert 0.05 < want["AP"] < 0.9 and set(dfs["labels"]["label"]) == {"a", "b", "c"}
    assert len(dfs["dets"]) == len(preds) and len(dfs["gts"]) == len(gts) and "match_0.5" in dfs["dets"]


@pytest.mark.parametrize("iou_type", ["bbox", "segm"])
def test_coco_meter_ignored_ground_truths(dev, frames, iou_type):
    """Every second ground truth ignored through the column, and the same through visib_gt_min."""
    from happypose_amd.evaluation import CocoMeter

    preds, gts = frames
    gts = [dict(g, ignore=(k % 2 == 1)) for k, g in enumerate(gts)]
    want = R.coco_evaluate(preds, gts, iou_type)
    meter = CocoMeter(iou_type=iou_type)
    meter.add(_collection(preds, dev, True), _collection(gts, dev, False))
    by_visib = CocoMeter(iou_type=iou_type, visib_gt_min=0.5)
    g = _collection(gts, dev, False)
    g.infos["visib_fract"] = np.where(g.infos["ignore"], 0.2, 0.9)
    g.infos = g.infos.drop(columns="ignore")
    by_visib.add(_collection(preds, dev, True), g)
    for m in (meter, by_visib):
        summary, _ = m.summary()
        for k in ("AP", "AP50", "AP75", "AR"):
            assert abs(summary[k] - want[k]) <= 1e-12, k


@pytest.mark.parametrize("iou_type", ["bbox", "segm"])
def test_detection_meter(dev, frames, iou_type):
    from happypose_amd.evaluation import DetectionMeter

    preds, gts = frames
    want = R.detection_meter(preds, gts, iou_type)
    if iou_type == "bbox":
        _, ious = R.coco_evaluate(preds, gts, "bbox", return_ious=True)
        assert np.abs(ious - 0.5).min() >= 1e-4  # the float32 boxes cannot flip a match
    meter = DetectionMeter(iou_type=iou_type)
    meter.add(_collection(preds, dev, True), _collection(gts, dev, False))
    summary, dfs = meter.summary()
    print(iou_type, summary, want)
    assert set(summary) == set(want)
    for k, v in want.items():
        assert abs(summary[k] - v) <= 1e-12, k
    assert summary["n_matched"] > 3 and summary["n_pred"] == len(preds) - 1  # the prediction on the frame without ground truth is dropped
    assert set(dfs) == {"gt", "matches", "preds", "ap"}


# ---- scene -----------------------------------------------------------------------------------------------------------------------
SCENE_RES = (120, 160)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def test_scene_ground_truth(dev, golden_dir):
    """The reference's test asset twice, overlapping in one 120 x 160 camera."""
    from happypose_amd import ops, scene as S
    from happypose_amd.evaluation import CocoMeter, scene_ground_truth
    from happypose_amd.mesh_store import RigidObject, RigidObjectDataset
    from happypose_amd.tensor_collection import PandasTensorCollection

    ds = RigidObjectDataset([RigidObject(label, golden_dir / "obj_000001.npz", mesh_units="mm") for label in ("can_a", "can_b")])
    renderer = S.SceneRenderer(ds, device=dev)
    h, w = SCENE_RES
    TWO = np.tile(np.eye(4), (2, 1, 1))
    TWO[0, :3, :3], TWO[0, :3, 3] = _rot((1, 0.3, 0.2), 65.0), (-0.02, 0.0, 0.34)
    TWO[1, :3, :3], TWO[1, :3, 3] = _rot((0.2, 1, -0.4), -110.0), (0.02, 0.005, 0.42)
    objects = [S.Panda3dObjectData("can_a", TWO=TWO[0]), S.Panda3dObjectData("can_b", TWO=TWO[1])]
    cameras = [S.Panda3dCameraData(K=np.array([[170.0, 0, w / 2], [0, 170.0, h / 2], [0, 0, 1]]), resolution=SCENE_RES)]
    gt = scene_ground_truth(renderer, objects, cameras, frames=[(3, 7)])
    assert len(gt) == 2 and gt.masks.shape == (2, h, w) and gt.masks.dtype == torch.bool and gt.bboxes.shape == (2, 4)
    assert gt.infos["scene_id"].tolist() == [3, 3] and gt.infos["view_id"].tolist() == [7, 7] and gt.infos["label"].tolist() == ["can_a", "can_b"]
    vis = renderer.scene_visibility(objects, cameras)
    _, area = ops.mask_pack(gt.masks)
    assert area.cpu().numpy().tolist() == vis["px_count_visib"].tolist() == gt.infos["px_count_visib"].tolist()
    assert vis["px_count_visib"].iloc[1] < vis["px_count_all"].iloc[1], "the two instances must overlap"
    masks = gt.masks.cpu().numpy()
    for k in range(2):  # the boxes enclose exactly the visible pixels
        ys, xs = np.where(masks[k])
        assert gt.bboxes[k].cpu().numpy().tolist() == [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
        x, y, bw, bh = vis["bbox_visib"].iloc[k]
        assert gt.bboxes[k].cpu().numpy().tolist() == [x, y, x + bw, y + bh]

    def as_predictions(m):
        infos = gt.infos[["scene_id", "view_id", "label"]].copy()
        infos["score"] = [0.9, 0.8]
        return PandasTensorCollection(infos, masks=m, bboxes=gt.bboxes.clone())

    for iou_type in ("bbox", "segm"):
        meter = CocoMeter(iou_type=iou_type)
        meter.add(as_predictions(gt.masks.clone()), gt)
        summary, _ = meter.summary()
        assert abs(summary["AP"] - 1.0) <= 1e-12 and abs(summary["AR"] - 1.0) <= 1e-12, (iou_type, summary)
    # half of one prediction's mask removed: the value the reference computes
    halved = gt.masks.clone()
    ys = np.where(masks[0].any(1))[0]
    halved[0, int(ys.mean()):] = False
    meter = CocoMeter(iou_type="segm")
    meter.add(as_predictions(halved), gt)
    summary, _ = meter.summary()
    recs = lambda m, scores: [{"scene_id": 3, "view_id": 7, "label": lab, "mask": m[k], **({"score": scores[k]} if scores else {"ignore": False})}  # noqa: E731
                              for k, lab in enumerate(("can_a", "can_b"))]
    want = R.coco_evaluate(recs(halved.cpu().numpy(), [0.9, 0.8]), recs(masks, None), "segm")
    print(summary, want)
    assert want["AP"] < 0.9
    for k in ("AP", "AP50", "AP75", "AR"):
        assert abs(summary[k] - want[k]) <= 1e-12, k
