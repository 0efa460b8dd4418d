"""Hand-made cases that pin the restatement of the data sets' batch assembly (tests/batch_data_ref.py) and the host side of
happypose_amd.datasets / ops (argument checks that need no GPU).

The reference's ``PoseDataset.make_data_from_obs`` imports under the namespace shim of tools/gen_golden.py but cannot run to its
end there: ``TWC.inverse() * TWO`` needs pinocchio's SE3, which is not installed and is an inert stub under the shim.  So there is
no recorded golden file for this step; these cases are worked out by hand from the reference's lines."""

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import batch_data_ref as R  # noqa: E402


def _scene():
    """8 x 10 id map: id 1 a 3 x 4 block (box 1, 1, 4, 3: area 3 * 2 = 6 without + 1, 12 pixels), id 2 one pixel (area 0), id 3 a
    row of 6 (box 2, 6, 7, 6: area 0), id 5 a 4 x 3 block (box 6, 0, 8, 3: area 2 * 3 = 6); id 4 is absent."""
    seg = np.zeros((8, 10), np.int32)
    seg[1:4, 1:5] = 1
    seg[5, 0] = 2
    seg[6, 2:8] = 3
    seg[0:4, 6:9] = 5
    ids = [1, 2, 3, 4, 5]
    boxes = R.modal_boxes(seg, ids)
    objects = [dict(unique_id=u, label=f"obj_{u}", bbox_modal=np.array(b if b is not None else [0, 0, 0, 0]), TWO=np.eye(4))
               for u, b in zip(ids, boxes)]
    return seg, objects


def _uids(objs):
    return [o["unique_id"] for o in objs]


def test_modal_boxes_are_inclusive():
    seg, objects = _scene()
    assert [list(o["bbox_modal"]) for o in objects] == [[1, 1, 4, 3], [0, 5, 0, 5], [2, 6, 7, 6], [0, 0, 0, 0], [6, 0, 8, 3]]


def test_invisible_objects_are_removed_and_a_one_pixel_object_is_valid_without_min_area():
    seg, objects = _scene()
    assert _uids(R.pose_valid_objects(seg, objects)) == [1, 2, 3, 5]


def test_min_area_is_greater_or_equal_on_the_inclusive_box_without_plus_one():
    seg, objects = _scene()
    # areas 6, 0, 0, 6: with + 1 they would be 12, 1, 6, 12
    assert _uids(R.pose_valid_objects(seg, objects, min_area=6)) == [1, 5]        # area == min_area passes (>=)
    assert _uids(R.pose_valid_objects(seg, objects, min_area=6.5)) == []
    assert _uids(R.pose_valid_objects(seg, objects, min_area=0)) == [1, 2, 3, 5]  # 0 >= 0
    assert _uids(R.pose_valid_objects(seg, objects, min_area=1)) == [1, 5]        # the row of 6 pixels has area 0


def test_keep_labels_set_and_return_first_object():
    seg, objects = _scene()
    assert _uids(R.pose_valid_objects(seg, objects, keep_labels_set={"obj_3", "obj_5", "obj_4"})) == [3, 5]
    first = lambda n: 0  # noqa: E731
    assert R.pose_make_data_from_obs(seg, objects, np.eye(4), first)[0]["unique_id"] == 1
    assert R.pose_make_data_from_obs(seg, objects, np.eye(4), first, keep_labels_set={"obj_5"})[0]["unique_id"] == 5
    assert R.pose_make_data_from_obs(seg, objects, np.eye(4), lambda n: n - 1)[0]["unique_id"] == 5


def test_a_frame_without_a_valid_object_gives_none():
    seg, objects = _scene()
    assert R.pose_make_data_from_obs(seg, objects, np.eye(4), lambda n: 0, min_area=7) is None
    assert R.pose_make_data_from_obs(np.zeros_like(seg), objects, np.eye(4), lambda n: 0) is None
    assert R.pose_make_data_from_obs(seg, [], np.eye(4), lambda n: 0) is None


def test_tco_is_the_rigid_inverse_times_two():
    c, s = np.cos(0.3), np.sin(0.3)
    TWC = np.array([[c, -s, 0, 1.0], [s, c, 0, 2.0], [0, 0, 1, 3.0], [0, 0, 0, 1]], np.float32)
    TWO = np.array([[1, 0, 0, 0.5], [0, 0, -1, 0.25], [0, 1, 0, -1.0], [0, 0, 0, 1]], np.float32)
    seg, objects = _scene()
    objects[0]["TWO"] = TWO
    _, bbox, TCO = R.pose_make_data_from_obs(seg, objects, TWC, lambda n: 0)
    assert list(bbox) == [1, 1, 4, 3]
    assert np.abs(TCO - np.linalg.inv(TWC.astype(np.float64)) @ TWO.astype(np.float64)).max() < 1e-7  # TWC is rigid to float32 rounding
    assert np.array_equal(TCO[3], [0, 0, 0, 1])


def test_detection_keeps_area_strictly_above_min_area_and_counts_iscrowd_before_the_filter():
    seg, objects = _scene()
    cat = {f"obj_{u}": 10 + u for u in range(1, 6)}
    t = R.detection_make_data_from_obs(seg, objects, cat, min_area=5, idx=3)
    assert t["labels"].tolist() == [11, 15] and t["boxes"].tolist() == [[1, 1, 4, 3], [6, 0, 8, 3]] and t["area"].tolist() == [6, 6]
    assert t["masks"].shape == (2, 8, 10) and t["masks"].dtype == np.uint8
    assert np.array_equal(t["masks"][0], seg == 1) and np.array_equal(t["masks"][1], seg == 5)
    assert t["iscrowd"].shape == (4,) and t["image_id"].tolist() == [3]  # 4 visible objects, 2 kept
    # strict: area == min_area is dropped here, and the one-pixel object (area 0) never passes, not even with min_area = 0
    assert R.detection_make_data_from_obs(seg, objects, cat, min_area=6)["labels"].tolist() == []
    assert R.detection_make_data_from_obs(seg, objects, cat, min_area=0)["labels"].tolist() == [11, 15]
    empty = R.detection_make_data_from_obs(np.zeros_like(seg), objects, cat)
    assert empty["boxes"].shape == (0, 4) and empty["masks"].shape == (0, 8, 10) and empty["iscrowd"].shape == (0,)


def test_table_form_follows_the_per_observation_functions():
    seg, objects = _scene()
    segs = [seg, np.zeros_like(seg), seg]
    ids = [[1, 2, 3, 4, 5], [1, 2], [5, 5, 1]]  # frame 2 lists id 5 twice: counted in its first slot
    boxes, n_px, count, table = R.seg_tables(segs, ids)
    assert n_px.tolist() == [[12, 1, 6, 0, 12], [0, 0, 0, 0, 0], [12, 0, 12, 0, 0]] and count.tolist() == [5, 2, 3]
    TWC, TWO = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1)), np.tile(np.eye(4, dtype=np.float32), (3, 5, 1, 1))
    r = R.select_ref(n_px, boxes, count, None, None, True, 0, 0, TWC, TWO)
    assert r["chosen"].tolist() == [0, -1, 0] and r["valid"].tolist() == [True, False, True]
    assert r["dst"].tolist() == [0, 1, 1] and r["n_valid"] == 2 and r["n_valid_slots"].tolist() == [4, 0, 2]
    assert r["bbox"][2].tolist() == [6, 0, 8, 3]
    keep = np.zeros((3, 5), np.uint8)
    keep[0, 2] = keep[2, 2] = 1
    assert R.select_ref(n_px, boxes, count, keep, None, True, 0, 0, TWC, TWO)["chosen"].tolist() == [2, -1, 2]
    # the seeded choice: k = mulhi32(x0, n) walks the valid slots, and rows depend on (seed, row_offset + b) alone
    seen = {tuple(R.select_ref(n_px, boxes, count, None, None, False, s, 0, TWC, TWO)["chosen"]) for s in range(16)}
    assert len({c[0] for c in seen}) > 1 and all(c[0] in (0, 1, 2, 4) and c[1] == -1 and c[2] in (0, 2) for c in seen)
    tail = R.select_ref(n_px[1:], boxes[1:], count[1:], None, None, False, 5, 1, TWC[1:], TWO[1:])
    assert tail["chosen"].tolist() == R.select_ref(n_px, boxes, count, None, None, False, 5, 0, TWC, TWO)["chosen"].tolist()[1:]


def test_philox_word_matches_the_training_restatement():
    import training_ref as T

    assert np.array_equal(R.philox_x0(0x123456789ABCDEF, np.arange(5) + 2 ** 33), T.noise_words(5, 0x123456789ABCDEF, 2 ** 33)[:, 0])


def test_masks_and_gather_restatements():
    seg, _ = _scene()
    segs = np.stack([seg, seg.T.copy().reshape(8, 10)])
    table, slot_row = np.array([[1, 5], [3, 2]], np.int32), np.array([[1, -1], [-1, 0]], np.int32)
    m = R.masks_ref(segs, table, slot_row, 3)
    assert np.array_equal(m[1], seg == 1) and np.array_equal(m[0], segs[1] == 2) and (m[2] == 0xFF).all()
    rgb = np.arange(2 * 2 * 3 * 3, dtype=np.uint8).reshape(2, 2, 3, 3)
    out, depth = R.gather_ref(rgb, [False, True], np.ones((2, 2, 3), np.float32))
    assert out.shape == (1, 3, 2, 3) and out[0, 1, 1, 2] == rgb[1, 1, 2, 1] and depth.shape == (1, 2, 3)


def test_wrappers_reject_cpu_tensors():
    torch = pytest.importorskip("torch")
    from happypose_amd import augmentations as A
    from happypose_amd import datasets, ops

    with pytest.raises(ValueError):
        ops.pose_batch_select(torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, 4, dtype=torch.int32), torch.eye(4)[None],
                              torch.eye(4)[None, None].repeat(1, 2, 1, 1))
    with pytest.raises(ValueError):
        ops.batch_gather_chw(torch.zeros(1, 2, 2, 3, dtype=torch.uint8), torch.ones(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), 1)
    with pytest.raises(ValueError):
        ops.instance_masks(torch.zeros(1, 2, 2, dtype=torch.int32), [[1]], [[0]], 1)
    batch = A.ObservationBatch(rgb=torch.zeros(1, 4, 4, 3, dtype=torch.uint8), segmentation=torch.zeros(1, 4, 4, dtype=torch.int32), K=torch.eye(3)[None])
    with pytest.raises(ValueError):
        datasets.PoseDataset(resize=(4, 4), apply_rgb_augmentation=False).make_batch(batch, [[]], np.eye(4)[None], None, seed=0)
    with pytest.raises(ValueError):
        datasets.DetectionDataset({}, resize=(4, 4)).make_batch(batch, [[]], np.random.default_rng(0))
    assert issubclass(datasets.NoObjectError, Exception)
    assert [f.name for f in __import__("dataclasses").fields(datasets.BatchPoseData)][:6] == ["rgbs", "object_datas", "bboxes", "TCO", "K", "depths"]
