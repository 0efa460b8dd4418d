"""NumPy restatement of the batch assembly of the training data sets (include/happypose_amd.h: hp_pose_batch_select,
hp_batch_gather_chw, hp_instance_masks), written from the reference's ``PoseDataset.make_data_from_obs`` + ``collate_fn``
(toolbox/datasets/pose_dataset.py) and ``DetectionDataset.make_data_from_obs`` (cosypose/datasets/detection_dataset.py), line by
line where a line decides something.  Test infrastructure: it imports nothing from happypose_amd.  Integers everywhere, float64 for
the pose product.  tests/test_batch_data_reference.py pins it on hand-made cases; tests/test_gpu_batch_data.py compares the
kernels with it.

An observation here is ``segmentation [H, W]`` plus a list of objects, dicts with ``unique_id``, ``label``, ``bbox_modal`` (inclusive
x1, y1, x2, y2, as make_detections_from_segmentation gives it) and ``TWO``.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from mesh_sample_ref import MASK32, philox4x32_10  # noqa: E402

TCO_BOUND_FACTOR = 8 * 2.0 ** -24  # per entry: 8 * 2^-24 * sum_k |a_ik| |b_kj|


# ---- the two reference functions, one observation at a time -------------------------------------------------------------------------
def modal_boxes(segmentation, unique_ids):
    """``make_detections_from_segmentation``: the inclusive min / max of the columns and rows of every id; None when absent."""
    out = []
    for uid in unique_ids:
        ys, xs = np.nonzero(np.asarray(segmentation) == uid)
        out.append(None if len(ys) == 0 else [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())])
    return out


def remove_invisible_objects(segmentation, objects):
    ids_in_segm = np.unique(segmentation)
    ids_visible = set(ids_in_segm[ids_in_segm > 0].tolist())
    return [o for o in objects if o["unique_id"] in ids_visible]


def pose_valid_objects(segmentation, objects, min_area=None, keep_labels_set=None):
    """``PoseDataset.make_data_from_obs`` up to ``valid_objects`` (pose_dataset.py:268-293)."""
    objects = remove_invisible_objects(segmentation, objects)
    unique_ids_visible = set(np.unique(segmentation).tolist())
    valid_objects = []
    for obj in objects:
        valid = False
        # `np.all(obj.bbox_modal) >= 0` compares a boolean with 0: always true, as written in the reference
        if obj["unique_id"] in unique_ids_visible and np.all(obj["bbox_modal"]) >= 0:
            valid = True
        if valid and min_area is not None:
            bbox = obj["bbox_modal"]
            area = (bbox[3] - bbox[1]) * (bbox[2] - bbox[0])
            valid = bool(area >= min_area)
        if valid and keep_labels_set is not None:
            valid = obj["label"] in keep_labels_set
        if valid:
            valid_objects.append(obj)
    return valid_objects


def rigid_inverse(T):
    """``Transform.inverse()`` (pinocchio's SE3): ``(R^T, -R^T t)``, float64."""
    T = np.asarray(T, np.float32).astype(np.float64)
    out = np.zeros(T.shape)
    out[..., :3, :3] = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, 3] = -np.einsum("...ki,...k->...i", T[..., :3, :3], T[..., :3, 3])
    out[..., 3, 3] = 1.0
    return out


def pose_make_data_from_obs(segmentation, objects, TWC, k_of_n, min_area=None, keep_labels_set=None):
    """The rest of ``make_data_from_obs``: None, or ``(object, bbox, TCO float64)``.  ``k_of_n(n)`` picks among ``n`` valid objects
    (``return_first_object``: ``lambda n: 0``; otherwise the seeded choice, which replaces ``random.sample``)."""
    valid_objects = pose_valid_objects(segmentation, objects, min_area, keep_labels_set)
    if len(valid_objects) == 0:
        return None
    obj = valid_objects[k_of_n(len(valid_objects))]
    TCO = rigid_inverse(TWC) @ np.asarray(obj["TWO"], np.float32).astype(np.float64)
    return obj, np.asarray(obj["bbox_modal"]), TCO


def detection_make_data_from_obs(segmentation, objects, label_to_category_id, min_area=50, idx=0):
    """``DetectionDataset.make_data_from_obs`` after the augmentations (detection_dataset.py:83-133).  Its line
    ``masks = masks == obj_ids[:, None, None]`` compares the 0 / 1 masks with the ids once more, which leaves a mask only for
    ``unique_id == 1``; the masks here are ``segmentation == unique_id``, what the lines before it build."""
    objects = remove_invisible_objects(segmentation, objects)
    categories = np.array([label_to_category_id[o["label"]] for o in objects], np.int64)
    boxes = np.array([list(o["bbox_modal"]) for o in objects], np.int64).reshape(-1, 4)
    area = (boxes[:, 3] - boxes[:, 1]) * (boxes[:, 2] - boxes[:, 0])
    masks = np.stack([np.asarray(segmentation) == o["unique_id"] for o in objects]) if objects else np.zeros((0,) + np.shape(segmentation), bool)
    keep = area > min_area
    num_objs = len(objects)  # `len(obj_ids)`: BEFORE the filter
    return {"boxes": boxes[keep], "labels": categories[keep], "masks": masks[keep].astype(np.uint8), "image_id": np.array([idx]),
            "area": area[keep], "iscrowd": np.zeros(num_objs, np.int64)}


# ---- the table form the kernels take ------------------------------------------------------------------------------------------------
def philox_x0(seed: int, rows) -> np.ndarray:
    """Word 0 of Philox4x32-10, key (seed lo, seed hi), counter (row lo, row hi, 0, 0)."""
    rows = np.asarray(rows, np.uint64).reshape(-1)
    c = np.zeros((len(rows), 4), np.uint64)
    c[:, 0], c[:, 1] = rows & np.uint64(MASK32), rows >> np.uint64(32)
    return philox4x32_10(c, (seed & MASK32, (seed >> 32) & MASK32))[:, 0]


def seeded_k(seed: int, row: int):
    x0 = int(philox_x0(seed, [row])[0])
    return lambda n: (x0 * n) >> 32  # mulhi32


def seg_tables(segmentations, ids):
    """``hp_seg_boxes`` on lists: ``boxes [B, max_ids, 4]``, ``n_px [B, max_ids]``, ``count [B]``, ``table [B, max_ids]``.  An id
    listed twice is counted in its first slot; a slot without pixels has n_px 0 and a box of -7 (unspecified in the kernel)."""
    B, max_ids = len(ids), max(max((len(r) for r in ids), default=0), 1)
    boxes, n_px = np.full((B, max_ids, 4), -7, np.int32), np.zeros((B, max_ids), np.int32)
    table, count = np.zeros((B, max_ids), np.int32), np.array([len(r) for r in ids], np.int32)
    for b, row in enumerate(ids):
        table[b, :len(row)] = row
        for k, uid in enumerate(row):
            if uid in list(row[:k]):
                continue
            ys, xs = np.nonzero(np.asarray(segmentations[b]) == uid)
            if len(ys):
                boxes[b, k], n_px[b, k] = (xs.min(), ys.min(), xs.max(), ys.max()), len(ys)
    return boxes, n_px, count, table


def select_ref(n_px, boxes, count, keep, min_area, first, seed, row_offset, TWC, TWO):
    """``hp_pose_batch_select`` from its tables: ``make_data_from_obs`` of frame ``b`` with the objects ``slot k -> {unique_id: k + 1}``
    on a synthetic id map that holds exactly the slots with pixels.  Returns a dict of arrays; ``TCO`` float64 and ``TCO_bound``."""
    B, max_ids = n_px.shape
    out = dict(chosen=np.full(B, -1, np.int32), valid=np.zeros(B, bool), bbox=np.zeros((B, 4), np.float32), TCO=np.zeros((B, 4, 4)),
               TCO_bound=np.zeros((B, 4, 4)), n_valid_slots=np.zeros(B, np.int32))
    for b in range(B):
        cnt = int(np.clip(count[b], 0, max_ids))
        seg = np.array([k + 1 for k in range(cnt) if n_px[b, k] > 0] + [0])
        objects = [dict(unique_id=k + 1, label=k, bbox_modal=boxes[b, k].astype(np.int64), TWO=TWO[b, k]) for k in range(cnt)]
        labels = None if keep is None else {k for k in range(cnt) if keep[b, k]}
        out["n_valid_slots"][b] = len(pose_valid_objects(seg, objects, min_area, labels))
        data = pose_make_data_from_obs(seg, objects, TWC[b], (lambda n: 0) if first else seeded_k(seed, row_offset + b), min_area, labels)
        if data is None:
            continue
        obj, bbox, TCO = data
        out["chosen"][b], out["valid"][b], out["bbox"][b], out["TCO"][b] = obj["label"], True, bbox, TCO
        out["TCO_bound"][b] = TCO_BOUND_FACTOR * (np.abs(rigid_inverse(TWC[b])) @ np.abs(np.asarray(TWO[b, obj["label"]], np.float64)))
    out["dst"] = (np.cumsum(out["valid"]) - out["valid"]).astype(np.int32)  # exclusive scan
    out["n_valid"] = int(out["valid"].sum())
    return out


def gather_ref(rgb, valid, depth=None):
    """``collate_fn``: ``rgb[valid].permute(0, 3, 1, 2)`` and ``depth[valid]``."""
    valid = np.asarray(valid, bool)
    return np.ascontiguousarray(np.asarray(rgb)[valid].transpose(0, 3, 1, 2)), None if depth is None else np.asarray(depth)[valid].copy()


def masks_ref(segmentations, table, slot_row, G, fill=0xFF):
    """``hp_instance_masks``: rows no slot names keep ``fill``."""
    seg = np.asarray(segmentations)
    out = np.full((G,) + seg.shape[1:], fill, np.uint8)
    for b in range(seg.shape[0]):
        for k in range(table.shape[1]):
            if 0 <= slot_row[b, k] < G:
                out[slot_row[b, k]] = seg[b] == table[b, k]
    return out
