"""The data sets' batch assembly on the device (csrc/batch_data.hip, happypose_amd.datasets) against the NumPy restatement
(tests/batch_data_ref.py).

Everything is compared exactly (integers and copied bits) except ``TCO``: per entry ``|err| <= 8 * 2^-24 * sum_k |a_ik| |b_kj|``
with ``a = inverse(TWC)`` and ``b = TWO`` of the float64 reference -- the rounding bound of a 3-term float32 dot product, with
slack for the inverse's own products.  The restatement computes the sum from its own operands."""

import sys
from collections import defaultdict
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import batch_data_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEEDS = [11, 12, 13, 14, 15, 16, 17, 2 ** 63 + 5]
MIN_AREA = 4.0


def dev(a):
    return torch.as_tensor(a).to(DEV)


def same_bits(a: torch.Tensor, b: np.ndarray) -> bool:
    a = a.detach().cpu().contiguous().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == np.ascontiguousarray(b).tobytes()


def _poses(rs, n):
    q, _ = np.linalg.qr(rs.randn(n, 3, 3))
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :3], T[:, :3, 3] = q, rs.uniform(-1.5, 1.5, (n, 3))
    return T.astype(np.float32)


# ---- select -------------------------------------------------------------------------------------------------------------------------
def _block(seg, uid, x1, y1, x2, y2):
    seg[y1:y2 + 1, x1:x2 + 1] = uid


@pytest.fixture(scope="module")
def sel():
    """B = 6, max_ids = 7 on 16 x 20 id maps: frame 0 has no objects, the objects of frame 1 all fail min_area = 4 (one pixel, a row,
    a 3 x 2 block of area 2), frame 2 has a single valid slot, frames 3 and 4 have 4 and 5, frame 5 has 2.  Frame 3 lists id 9 twice
    (counted in its first slot) and id 77, which is absent; frame 4 holds a box with area == min_area."""
    from happypose_amd import ops

    segs = np.zeros((6, 16, 20), np.int32)
    _block(segs[1], 1, 3, 3, 3, 3), _block(segs[1], 2, 0, 8, 9, 8), _block(segs[1], 3, 12, 1, 14, 2)
    _block(segs[2], 4, 2, 2, 9, 9), _block(segs[2], 5, 15, 15, 15, 15)
    _block(segs[3], 9, 0, 0, 4, 4), _block(segs[3], 8, 6, 0, 10, 5), _block(segs[3], 7, 12, 0, 19, 7), _block(segs[3], 6, 0, 8, 7, 15)
    _block(segs[3], 5, 10, 10, 10, 12)
    _block(segs[4], 1, 0, 0, 2, 2), _block(segs[4], 2, 4, 0, 9, 3), _block(segs[4], 3, 11, 0, 15, 6), _block(segs[4], 4, 0, 5, 5, 12)
    _block(segs[4], 5, 8, 8, 16, 14), _block(segs[4], 2 ** 31 - 1, 18, 12, 19, 15)
    _block(segs[5], 3, 1, 1, 6, 6), _block(segs[5], 2, 10, 1, 17, 9), _block(segs[5], 1, 0, 12, 19, 12)
    ids = [[], [1, 2, 3], [5, 4], [9, 77, 8, 9, 5, 7, 6], [2 ** 31 - 1, 1, 2, 3, 4, 5], [1, 2, 3]]
    boxes, n_px, count, table = R.seg_tables(segs, ids)
    assert n_px.shape == (6, 7)
    rs = np.random.RandomState(4)
    TWC, TWO = _poses(rs, 6), _poses(rs, 42).reshape(6, 7, 4, 4)
    d_boxes, d_n_px = ops.seg_boxes(dev(segs), ids)
    assert np.array_equal(d_n_px.cpu().numpy(), n_px) and np.array_equal(d_boxes.cpu().numpy()[n_px > 0], boxes[n_px > 0])
    return SimpleNamespace(boxes=boxes, n_px=n_px, count=count, TWC=TWC, TWO=TWO, d_boxes=d_boxes, d_n_px=d_n_px, d_TWC=dev(TWC), d_TWO=dev(TWO))


def _ref(s, first, seed, row_offset=0, keep=None, min_area=MIN_AREA, rows=slice(None)):
    return R.select_ref(s.n_px[rows], s.boxes[rows], s.count[rows], None if keep is None else keep[rows], min_area, first, seed, row_offset,
                        s.TWC[rows], s.TWO[rows])


def _run(s, first, seed, row_offset=0, keep=None, min_area=MIN_AREA, rows=slice(None)):
    from happypose_amd import ops

    c = lambda t: t[rows].contiguous()  # noqa: E731
    return ops.pose_batch_select(c(s.d_n_px), c(s.d_boxes), c(s.d_TWC), c(s.d_TWO), count=s.count[rows], keep=None if keep is None else dev(keep[rows]),
                                 min_area=min_area, first=first, seed=seed, row_offset=row_offset)


def _compare(got, ref):
    chosen, valid, bbox, TCO, dst, n_valid = got
    assert np.array_equal(chosen.cpu().numpy(), ref["chosen"]) and chosen.dtype == torch.int32
    assert np.array_equal(valid.cpu().numpy(), ref["valid"])
    assert np.array_equal(dst.cpu().numpy(), ref["dst"]) and int(n_valid.item()) == ref["n_valid"]
    v = ref["valid"]
    assert same_bits(bbox.cpu()[torch.as_tensor(v)], ref["bbox"][v])
    err = np.abs(TCO.cpu().numpy().astype(np.float64) - ref["TCO"])[v]
    print(f"TCO: largest error / bound = {(err / np.maximum(ref['TCO_bound'][v], 1e-300)).max():.3g}")
    assert (err <= ref["TCO_bound"][v]).all()


def test_the_cases_are_what_the_docstring_says(sel):
    n = _ref(sel, True, 0)["n_valid_slots"]
    assert n.tolist() == [0, 0, 1, 4, 5, 2]
    assert (sel.n_px[1, :3] > 0).all() and sel.n_px[3, 1] == 0 and sel.n_px[3, 3] == 0  # all fail by area; absent; listed twice
    b = sel.boxes[4, 1]
    assert (b[3] - b[1]) * (b[2] - b[0]) == MIN_AREA  # >= keeps it
    # the seeded choice takes more than one value in a frame with 3 or more valid slots -- on the restatement, before any kernel runs
    picks = np.stack([_ref(sel, False, s)["chosen"] for s in SEEDS])
    assert len(set(picks[:, 3])) > 1 and len(set(picks[:, 4])) > 1


@pytest.mark.parametrize("mode", ["first"] + SEEDS)
def test_select_against_the_restatement(sel, mode):
    first, seed = mode == "first", 0 if mode == "first" else mode
    _compare(_run(sel, first, seed), _ref(sel, first, seed))


def test_select_without_min_area_and_with_keep(sel):
    ref = _ref(sel, True, 0, min_area=None)
    assert ref["chosen"].tolist() == [-1, 0, 0, 0, 0, 0]  # a one-pixel object is valid without min_area
    _compare(_run(sel, True, 0, min_area=None), ref)
    keep = np.zeros((6, 7), np.uint8)
    keep[2, 0] = keep[3, 1] = keep[3, 5] = keep[3, 6] = keep[4, 4] = 1  # frame 2: only the invalid slot; frame 3: the absent id and two valid
    ref = _ref(sel, True, 0, keep=keep)
    assert ref["chosen"].tolist() == [-1, -1, -1, 5, 4, -1]
    _compare(_run(sel, True, 0, keep=keep), ref)
    _compare(_run(sel, False, SEEDS[1], keep=keep), _ref(sel, False, SEEDS[1], keep=keep))


def test_row_offset_gives_the_tail_of_a_longer_batch(sel):
    full, tail = _run(sel, False, SEEDS[2]), _run(sel, False, SEEDS[2], row_offset=2, rows=slice(2, 6))
    _compare(tail, _ref(sel, False, SEEDS[2], row_offset=2, rows=slice(2, 6)))
    for k in (0, 1, 2, 3):  # chosen, valid, bbox, TCO of frames 2 .. 5, bit for bit
        assert same_bits(tail[k], full[k][2:].cpu().numpy())
    again = _run(sel, False, SEEDS[2])
    assert all(same_bits(a, b.cpu().numpy()) for a, b in zip(again, full))


def test_select_arguments():
    from happypose_amd import ops

    n_px, boxes = torch.zeros(2, 3, dtype=torch.int32, device=DEV), torch.zeros(2, 3, 4, dtype=torch.int32, device=DEV)
    TWC, TWO = torch.eye(4, device=DEV).repeat(2, 1, 1), torch.eye(4, device=DEV).repeat(2, 3, 1, 1)
    with pytest.raises(ValueError):
        ops.pose_batch_select(n_px.cpu(), boxes, TWC, TWO)
    with pytest.raises(ValueError):
        ops.pose_batch_select(n_px.long(), boxes, TWC, TWO)
    with pytest.raises(ValueError):
        ops.pose_batch_select(n_px, boxes[:, :2].contiguous(), TWC, TWO)
    with pytest.raises(ValueError):
        ops.pose_batch_select(n_px, boxes, TWC.double(), TWO)
    out = ops.pose_batch_select(n_px[:0], boxes[:0], TWC[:0], TWO[:0])
    assert [t.shape[0] for t in out[:5]] == [0] * 5 and int(out[5].item()) == 0


# ---- gather -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(37, 53), (480, 640)])
def test_gather_against_the_restatement(hw):
    from happypose_amd import ops

    h, w = hw
    rs = np.random.RandomState(h)
    rgb = rs.randint(0, 256, (5, h, w, 3)).astype(np.uint8)
    depth = rs.randn(5, h, w).astype(np.float32)
    depth[:, 0, 0], depth[:, -1, -1], depth[:, h // 2, 1] = np.nan, -0.0, np.float32(np.inf)
    valid = np.array([1, 0, 1, 1, 0], bool)
    dst = (np.cumsum(valid) - valid).astype(np.int32)
    want_rgb, want_depth = R.gather_ref(rgb, valid, depth)
    out = torch.full((5, 3, h, w), 0xA5, dtype=torch.uint8, device=DEV)  # 3 rows and 2 rows of padding
    out_depth = torch.full((5, h, w), 123.0, dtype=torch.float32, device=DEV)
    got, got_depth = ops.batch_gather_chw(dev(rgb), dev(valid), dev(dst), depth=dev(depth), out=out, out_depth=out_depth)
    assert got.data_ptr() == out.data_ptr()
    assert same_bits(got[:3], want_rgb) and same_bits(got_depth[:3], want_depth)
    assert (got[3:] == 0xA5).all() and (got_depth[3:] == 123.0).all()  # the canary
    assert torch.equal(got[:3], dev(rgb)[dev(valid)].permute(0, 3, 1, 2))
    only, none = ops.batch_gather_chw(dev(rgb), dev(valid), dev(dst), 3)
    assert none is None and same_bits(only, want_rgb)


def test_gather_arguments():
    from happypose_amd import ops

    rgb = torch.zeros(2, 4, 6, 3, dtype=torch.uint8, device=DEV)
    valid, dst = torch.ones(2, dtype=torch.bool, device=DEV), torch.arange(2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.batch_gather_chw(rgb.cpu(), valid, dst, 2)
    with pytest.raises(ValueError):
        ops.batch_gather_chw(rgb.float(), valid, dst, 2)
    with pytest.raises(ValueError):
        ops.batch_gather_chw(rgb, valid, dst.long(), 2)
    with pytest.raises(ValueError):
        ops.batch_gather_chw(rgb, valid, dst, 2, depth=torch.zeros(2, 4, 5, device=DEV))
    got, _ = ops.batch_gather_chw(rgb[:0], valid[:0], dst[:0], 0)
    assert got.shape == (0, 3, 4, 6)


# ---- masks --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(37, 53), (480, 640)])
def test_instance_masks_against_the_restatement(hw):
    from happypose_amd import ops

    h, w = hw
    pool = np.array([0, 0, 1, 2, 3, 70000, 2 ** 31 - 1], np.int32)  # background 0 and ids up to 2^31 - 1
    seg = pool[np.random.RandomState(w).randint(0, len(pool), (3, h, w))]
    table = np.array([[2 ** 31 - 1, 1, 5, 3], [1, 2, 3, 0], [70000, 3, 3, 9]], np.int32)  # id 5 is absent; frame 2 lists id 3 twice
    slot_row = np.array([[3, 0, 5, -1], [-1, -1, -1, -1], [1, 4, 2, 6]], np.int32)        # frame 1 keeps nothing; slot (2, 3) is past count
    count = np.array([4, 4, 3], np.int32)
    G = 6
    want = R.masks_ref(seg, table, np.where(np.arange(4)[None] < count[:, None], slot_row, -1), G)
    assert not (want == 0xFF).any() and want[5].sum() == 0 and want[3].sum() > 0
    out = torch.full((G, h, w), 0xFF, dtype=torch.uint8, device=DEV)
    got = ops.instance_masks(dev(seg), table, slot_row, G, count=count, out=out)
    assert got.data_ptr() == out.data_ptr() and same_bits(got, want)
    assert same_bits(ops.instance_masks(dev(seg), dev(table), dev(slot_row), G, count=count), want)  # tables on the device
    assert ops.instance_masks(dev(seg), table, np.full_like(slot_row, -1), 0).shape == (0, h, w)  # G = 0


def test_instance_masks_arguments():
    from happypose_amd import ops

    seg = torch.zeros(2, 4, 6, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.instance_masks(seg.cpu(), [[1], [1]], [[0], [1]], 2)
    with pytest.raises(ValueError):
        ops.instance_masks(seg.float(), [[1], [1]], [[0], [1]], 2)
    with pytest.raises(ValueError):
        ops.instance_masks(seg, [[1], [1]], [[0, 1], [1, 2]], 2)
    assert ops.instance_masks(seg[:0], np.zeros((0, 1), np.int32), np.zeros((0, 1), np.int32), 0).shape == (0, 4, 6)


# ---- the classes --------------------------------------------------------------------------------------------------------------------
H, W = 120, 160


def _look_at(eye, target):
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = np.stack([x, np.cross(z, x), z], axis=1), eye
    return T


@pytest.fixture(scope="module")
def world():
    """Three objects in a row seen by three cameras at 120 x 160; camera 2 looks away from them."""
    from happypose_amd import augmentations as A
    from happypose_amd import scene as S
    from happypose_amd.renderer import BatchRenderer, make_scene_lights
    from happypose_amd.synthetic import make_object_dataset

    ds = make_object_dataset(n_objects=3, tex_size=64, n_lat=12, n_lon=16)
    batch_renderer = BatchRenderer(ds, device=torch.device("cuda:0"))
    renderer = S.SceneRenderer(renderer=batch_renderer)
    labels = list(batch_renderer.store.labels)
    records = []
    for k, label in enumerate(labels):
        TWO = np.eye(4)
        TWO[:3, 3] = [0.28 * (k - 1), 0.02 * k, 0.0]
        records.append(SimpleNamespace(label=str(label), unique_id=k + 1, TWO=TWO))
    K = np.array([[150.0, 0, 79.5], [0, 150.0, 59.5], [0, 0, 1]])
    eyes = [np.array([0.1, -1.0, 0.35]), np.array([-0.2, -0.9, 0.5]), np.array([0.0, -1.0, 0.3])]
    TWC = np.stack([_look_at(eyes[0], np.zeros(3)), _look_at(eyes[1], np.zeros(3)), _look_at(eyes[2], 2 * eyes[2])])
    cameras = [S.Panda3dCameraData(K=K, resolution=(H, W), TWC=T) for T in TWC]
    (g,) = renderer.render_scene_tensors([S.Panda3dObjectData(label=r.label, TWO=r.TWO) for r in records], cameras, make_scene_lights(),
                                         render_depth=True)
    batch = A.ObservationBatch(rgb=S._to_u8_hwc(g["rgb"]), depth=g["depth"][:, 0].contiguous(), segmentation=(g["ids"] + 1).contiguous(),
                               K=dev(np.tile(K, (3, 1, 1)).astype(np.float32)))
    seg = batch.segmentation.cpu().numpy()
    assert (seg[2] == 0).all() and all(len(np.unique(seg[b])) >= 3 for b in (0, 1)), "the scene: two frames with objects, one without"
    return SimpleNamespace(ds=ds, batch_renderer=batch_renderer, batch=batch, records=[records] * 3, TWC=TWC.astype(np.float32), seg=seg,
                           labels=[r.label for r in records])


@pytest.fixture(scope="module")
def pose_batch(world):
    from happypose_amd import datasets

    return datasets.PoseDataset(resize=(H, W), apply_rgb_augmentation=False).make_batch(world.batch, world.records, world.TWC, None, seed=3)


def test_pose_dataset_makes_the_batch(world, pose_batch):
    from happypose_amd import datasets, ops, training

    data = pose_batch
    assert isinstance(data, datasets.BatchPoseData) and data.frame_ids == [0, 1] and len(data.object_datas) == 2
    assert data.rgbs.shape == (2, 3, H, W) and data.rgbs.dtype == torch.uint8 and data.depths.shape == (2, H, W)
    assert torch.equal(data.rgbs, world.batch.rgb[:2].permute(0, 3, 1, 2)) and same_bits(data.depths, world.batch.depth[:2].cpu().numpy())
    ids = [[r.unique_id for r in rec] for rec in world.records]
    boxes, n_px = ops.seg_boxes(world.batch.segmentation, ids)
    slots = [rec.unique_id - 1 for rec in data.object_datas]
    for row, (b, k) in enumerate(zip(data.frame_ids, slots)):
        assert int(n_px[b, k]) > 0 and torch.equal(data.bboxes[row], boxes[b, k].float())
        assert list(R.modal_boxes(world.seg[b], [k + 1])[0]) == data.bboxes[row].tolist()
        a, t = R.rigid_inverse(world.TWC[b]), np.asarray(world.records[b][k].TWO, np.float32).astype(np.float64)
        err = np.abs(data.TCO[row].cpu().numpy().astype(np.float64) - a @ t)
        assert (err <= R.TCO_BOUND_FACTOR * (np.abs(a) @ np.abs(t))).all()
    assert torch.equal(data.K, world.batch.K[:2])
    bt = training._batch(data, "test")
    assert bt["B"] == 2 and bt["labels"] == [r.label for r in data.object_datas] and bt["rgbs"] is data.rgbs
    first = datasets.PoseDataset(resize=(H, W), apply_rgb_augmentation=False, return_first_object=True, keep_labels_set={world.labels[1], world.labels[2]})
    assert [r.label for r in first.make_batch(world.batch, world.records, world.TWC, None, seed=0).object_datas] == [world.labels[1]] * 2


def test_pose_dataset_with_augmentations_repeats_bit_for_bit(world):
    from happypose_amd import datasets

    from happypose_amd import augmentations as A

    ds = datasets.PoseDataset(resize=(H, W), apply_rgb_augmentation=True, apply_depth_augmentation=True)
    # the rgb chain is the generator's first consumer: this one applies a transform to both frames that stay (read from the draw itself)
    draw = A.make_rgb_augmentations()[0].draw(3, np.random.default_rng(6))
    assert (draw["apply"] & np.any([p["apply"] for p in draw["inner"]], axis=0))[:2].all()
    a = ds.make_batch(world.batch, world.records, world.TWC, np.random.default_rng(6), seed=9)
    b = ds.make_batch(world.batch, world.records, world.TWC, np.random.default_rng(6), seed=9)
    for x, y in ((a.rgbs, b.rgbs), (a.depths, b.depths), (a.TCO, b.TCO), (a.bboxes, b.bboxes)):
        assert same_bits(x, y.cpu().numpy())
    assert a.frame_ids == b.frame_ids and [r.label for r in a.object_datas] == [r.label for r in b.object_datas]
    plain = world.batch.rgb[:2].permute(0, 3, 1, 2)
    assert not torch.equal(a.rgbs[0], plain[0]) and not torch.equal(a.rgbs[1], plain[1])


def test_detection_dataset_makes_the_targets(world):
    from happypose_amd import datasets

    cat = {l: 5 + i for i, l in enumerate(world.labels)}
    images, targets = datasets.DetectionDataset(cat, min_area=50, resize=(H, W)).make_batch(world.batch, world.records, np.random.default_rng(1))
    assert images.shape == (3, H, W, 3) and images.dtype == torch.uint8 and len(targets) == 3
    for b, t in enumerate(targets):
        objects = [dict(unique_id=r.unique_id, label=r.label, bbox_modal=box) for r, box in
                   zip(world.records[b], R.modal_boxes(world.seg[b], [r.unique_id for r in world.records[b]])) if box is not None]
        ref = R.detection_make_data_from_obs(world.seg[b], objects, cat, min_area=50, idx=b)
        g = len(ref["labels"])
        assert t["boxes"].shape == (g, 4) and t["boxes"].dtype == torch.float32 and t["labels"].shape == (g,) and t["labels"].dtype == torch.int64
        assert t["masks"].shape == (g, H, W) and t["masks"].dtype == torch.uint8 and t["area"].shape == (g,)
        assert t["boxes"].is_cuda and t["labels"].is_cuda and t["masks"].is_cuda
        assert same_bits(t["masks"], ref["masks"]) and np.array_equal(t["boxes"].cpu().numpy(), ref["boxes"].astype(np.float32))
        assert t["labels"].tolist() == ref["labels"].tolist() and t["area"].tolist() == ref["area"].tolist()
        assert t["iscrowd"].shape == ref["iscrowd"].shape and t["image_id"].tolist() == [b]
    assert targets[2]["boxes"].shape[0] == 0 and targets[0]["boxes"].shape[0] >= 2


def test_no_valid_object_and_cpu_batches_raise(world):
    import dataclasses

    from happypose_amd import datasets

    with pytest.raises(datasets.NoObjectError):
        datasets.PoseDataset(resize=(H, W), min_area=1e9, apply_rgb_augmentation=False).make_batch(world.batch, world.records, world.TWC, None, seed=0)
    cpu = dataclasses.replace(world.batch, rgb=world.batch.rgb.cpu(), segmentation=world.batch.segmentation.cpu(), depth=None)
    with pytest.raises(ValueError):
        datasets.PoseDataset(resize=(H, W), apply_rgb_augmentation=False).make_batch(cpu, world.records, world.TWC, None, seed=0)
    with pytest.raises(ValueError):
        datasets.DetectionDataset({}, resize=(H, W)).make_batch(cpu, world.records, np.random.default_rng(0))


# ---- the chain: SceneRenderer -> PoseDataset.make_batch -> training.h_pose -----------------------------------------------------------
def test_the_batch_feeds_h_pose(world):
    """The model and the mesh tables are the small seeded ones of tests/test_gpu_training.py (two objects, the labels of the
    scene's first two; the predictor samples 2000 points per object, more than the scene's coarse meshes have), so the batch is
    made from those two labels."""
    from happypose_amd import datasets, training
    from happypose_amd.mesh_store import MeshDataBase
    from happypose_amd.models import create_pose_model_cosypose, pose_model_param_shapes
    from happypose_amd.renderer import BatchRenderer
    from happypose_amd.synthetic import make_object_dataset, predictor_weights

    ds = make_object_dataset(2, seed=1, tex_size=256)
    renderer = BatchRenderer(ds, device=torch.device("cuda:0"))
    mesh_db = MeshDataBase.from_object_ds(ds).batched().to(DEV)
    assert [o.label for o in ds.list_objects] == world.labels[:2]
    weights = predictor_weights(pose_model_param_shapes("resnet18", 6), seed=1)
    model = create_pose_model_cosypose(dict(backbone_str="resnet18"), renderer, state_dict=weights, max_batch=4)
    data = datasets.PoseDataset(resize=(H, W), apply_rgb_augmentation=False, keep_labels_set=set(world.labels[:2])).make_batch(
        world.batch, world.records, world.TWC, None, seed=3)
    assert data.frame_ids == [0, 1] and data.rgbs.shape == (2, 3, H, W)
    meters = defaultdict(training.AverageValueMeter)
    loss = training.h_pose(model, mesh_db, data, meters, training.CosyPoseTrainingConfig(n_points_loss=64), n_iterations=1,
                           input_generator="gt+noise", seed=7)
    assert loss.is_cuda and loss.shape == () and bool(torch.isfinite(loss))
    assert meters["loss_TCO-iter=1"].n == 1 and np.isfinite(meters["loss_TCO-iter=1"].mean)
