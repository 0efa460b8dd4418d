"""Batch assembly of the training data sets on the device: the step between a scene observation and the trainers' steps, the
reference's ``PoseDataset.make_data_from_obs`` + ``collate_fn`` (``toolbox/datasets/pose_dataset.py``) and
``DetectionDataset.make_data_from_obs`` (``cosypose/datasets/detection_dataset.py``) with their names and argument orders
(``csrc/batch_data.hip``; the rules are in ``include/happypose_amd.h``: ``hp_pose_batch_select``, ``hp_batch_gather_chw``,
``hp_instance_masks``).

The classes have no ``scene_ds``: they work on an ``augmentations.ObservationBatch`` of frames that already live on the GPU
(``SceneRenderer``'s output, say) and on ``object_datas``, one list of records per frame.  A record is anything with ``label``,
``unique_id`` (the object's value in ``batch.segmentation``) and, for ``PoseDataset``, ``TWO`` -- an object with these attributes or
a dict.  Dataset readers and the VOC loader stay out: the background frames come with the batch.

What leaves the device per batch: ``PoseDataset`` reads back the chosen slot and the valid flag of every frame (to pick the
records), ``DetectionDataset`` the box table (to evaluate the keep rule and lay out the mask rows).  No pixel does.

The reference's random STREAMS are not reproduced: the augmentations draw from the ``numpy.random.Generator`` handed in, the
object choice from ``(seed, row_offset + b)``.
"""

from __future__ import annotations

import dataclasses
from typing import Any, Dict, List, Optional, Sequence, Set, Tuple

import numpy as np
import torch

from . import augmentations as A
from . import ops

RGB_CHAIN_P = 0.8  # DetectionDataset: `random.random() < 0.8` around the rgb chain


@dataclasses.dataclass
class PoseData:
    """One row of a ``BatchPoseData``: ``rgb [h, w, 3]`` uint8, ``bbox [4]``, ``TCO [4, 4]``, ``K [3, 3]``, ``depth [h, w]``."""

    rgb: torch.Tensor
    bbox: torch.Tensor
    TCO: torch.Tensor
    K: torch.Tensor
    depth: Optional[torch.Tensor]
    object_data: Any


@dataclasses.dataclass
class BatchPoseData:
    """``rgbs [bsz, 3, h, w]`` uint8, ``depths [bsz, h, w]`` float32, ``bboxes [bsz, 4]`` float32 (x1, y1, x2, y2, inclusive),
    ``TCO [bsz, 4, 4]`` and ``K [bsz, 3, 3]`` float32, on the device; ``object_datas``: the chosen record of every row.
    ``frame_ids`` (not in the reference): the input frame every row came from."""

    rgbs: torch.Tensor
    object_datas: List[Any]
    bboxes: torch.Tensor
    TCO: torch.Tensor
    K: torch.Tensor
    depths: Optional[torch.Tensor] = None
    frame_ids: Optional[List[int]] = None


class NoObjectError(Exception):
    pass


def _field(record, name: str):
    return record[name] if isinstance(record, dict) else getattr(record, name)


def _check_batch(batch: A.ObservationBatch, object_datas, what: str) -> Tuple[int, torch.device]:
    for name in ("rgb", "segmentation"):
        t = getattr(batch, name)
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{what}: batch.{name} must be a tensor on the device (there is no CPU implementation)")
    B = batch.batch_size
    if len(object_datas) != B:
        raise ValueError(f"{what}: one list of object records per frame ({B}), got {len(object_datas)}")
    return B, batch.rgb.device


def _unique_ids(object_datas) -> List[List[int]]:
    return [[int(_field(o, "unique_id")) for o in objs] for objs in object_datas]


def _pose_table(object_datas, max_ids: int) -> np.ndarray:
    table = np.zeros((len(object_datas), max_ids, 4, 4), np.float32)
    for b, objs in enumerate(object_datas):
        for k, o in enumerate(objs):
            table[b, k] = np.asarray(_field(o, "TWO"), np.float64).reshape(4, 4)
    return table


class PoseDataset:
    """The reference's ``PoseDataset`` without ``scene_ds``, on batches: ``make_batch`` is ``make_data_from_obs`` on every frame,
    ``find_valid_data`` (frames without a valid object are skipped) and ``collate_fn``.  A slot is valid when it has a visible
    pixel after the resize, ``(x2 - x1) * (y2 - y1) >= min_area`` on the inclusive modal box (the reference's arithmetic: no + 1)
    and its label is in ``keep_labels_set``; ``return_first_object`` takes the first valid slot instead of a seeded one."""

    def __init__(self, resize: Tuple[int, int] = (480, 640), min_area: Optional[float] = None, apply_rgb_augmentation: bool = True,
                 apply_depth_augmentation: bool = False, apply_background_augmentation: bool = False, return_first_object: bool = False,
                 keep_labels_set: Optional[Set[str]] = None, depth_augmentation_level: int = 1):
        self.resize_transform = A.CropResizeToAspectTransform(resize=resize)
        self.min_area = min_area
        self.background_augmentations = A.make_background_augmentations() if apply_background_augmentation else []
        self.rgb_augmentations = A.make_rgb_augmentations() if apply_rgb_augmentation else []
        self.depth_augmentations = A.make_depth_augmentations(depth_augmentation_level) if apply_depth_augmentation else []
        self.return_first_object = return_first_object
        self.keep_labels_set = keep_labels_set

    def make_batch(self, batch: A.ObservationBatch, object_datas: Sequence[Sequence[Any]], TWC, rng: Optional[np.random.Generator], *,
                   seed: int, row_offset: int = 0) -> BatchPoseData:
        """``batch``: B frames on the device with ``K``; ``object_datas[b]``: the records of frame ``b``; ``TWC [B, 4, 4]``: the
        camera poses; ``rng``: the augmentations' generator (None when every augmentation is off).  Frame ``b`` chooses from
        ``(seed, row_offset + b)``.  Raises ``NoObjectError`` when no frame has a valid object."""
        B, dev = _check_batch(batch, object_datas, "PoseDataset.make_batch")
        if batch.K is None:
            raise ValueError("PoseDataset.make_batch: batch.K [B, 3, 3] is required")
        ids = _unique_ids(object_datas)
        batch = dataclasses.replace(batch, object_ids=ids)
        batch = self.resize_transform(batch, rng)
        # the reference's order: background, rgb, depth
        for chain in (self.background_augmentations, self.rgb_augmentations, self.depth_augmentations):
            if chain:
                if rng is None:
                    raise ValueError("PoseDataset.make_batch: augmentations are on: pass a numpy.random.Generator")
                batch = A.apply_augmentations(chain, batch, rng)
        boxes, n_px = ops.seg_boxes(batch.segmentation, ids)
        max_ids = int(n_px.shape[1])
        count = np.array([len(r) for r in ids], np.int32)
        keep = None
        if self.keep_labels_set is not None:
            table = np.zeros((B, max_ids), np.uint8)
            for b, objs in enumerate(object_datas):
                table[b, :len(objs)] = [_field(o, "label") in self.keep_labels_set for o in objs]
            keep = torch.from_numpy(table).to(dev)
        TWC = torch.as_tensor(np.asarray(TWC.detach().cpu() if isinstance(TWC, torch.Tensor) else TWC, np.float32).reshape(B, 4, 4)).to(dev)
        TWO = torch.from_numpy(_pose_table(object_datas, max_ids)).to(dev)
        chosen, valid, bbox, TCO, dst, _ = ops.pose_batch_select(n_px, boxes, TWC, TWO, count=count, keep=keep, min_area=self.min_area,
                                                                 first=self.return_first_object, seed=seed, row_offset=row_offset)
        picked = chosen.cpu().numpy()  # the one read-back: valid is chosen >= 0, n_valid their number
        frame_ids = [b for b in range(B) if picked[b] >= 0]
        if not frame_ids:
            raise NoObjectError("PoseDataset.make_batch: no frame has a valid object")
        rgbs, depths = ops.batch_gather_chw(batch.rgb, valid, dst, len(frame_ids), depth=batch.depth)
        rows = torch.as_tensor(frame_ids, device=dev)
        K = batch.K.to(device=dev, dtype=torch.float32).reshape(B, 3, 3)
        return BatchPoseData(rgbs=rgbs, object_datas=[object_datas[b][int(picked[b])] for b in frame_ids], bboxes=bbox[rows], TCO=TCO[rows],
                             K=K[rows].contiguous(), depths=depths, frame_ids=frame_ids)


class DetectionDataset:
    """The reference's ``DetectionDataset`` without ``scene_ds``, on batches.  ``make_batch`` returns ``(images, targets)`` as
    ``training.h_maskrcnn`` takes them: ``images [B, H, W, 3]`` uint8 and one dict per frame.

    As in the reference, whatever the flags say: the rgb chain (blur, sharpness, contrast, brightness, color with their own
    probabilities) runs on a frame with probability 0.8 -- ``rgb_augmentation`` and ``gray_augmentation`` are accepted and not
    read -- and the background is replaced with probability 0.3 whenever the batch carries ``background`` frames (the reference
    always loads VOC; ``background_augmentation=True`` here demands them).  Unlike the reference, which always resizes to
    480 x 640, ``resize`` is used.  Objects without a visible pixel after the resize are removed first; of the others those with
    ``(x2 - x1) * (y2 - y1) > min_area`` are kept -- strictly greater, unlike ``PoseDataset``, and again on the inclusive box, so a
    one-pixel object never passes.  A frame that keeps no object stays in the batch with ``g = 0``.

    A target holds ``boxes [g, 4]`` float32, ``labels [g]`` int64, ``masks [g, H, W]`` uint8 (``segmentation == unique_id``: the
    reference compares the 0 / 1 mask with the id once more, which leaves a mask only for ``unique_id == 1``; that line is not
    followed), ``area [g]``, ``image_id [1]`` and ``iscrowd``, zeros with the length of the visible object list BEFORE the area
    filter, as the reference makes it (nothing reads it)."""

    def __init__(self, label_to_category_id: Dict[str, int], min_area: float = 50, resize: Tuple[int, int] = (480, 640),
                 gray_augmentation: bool = False, rgb_augmentation: bool = False, background_augmentation: bool = False):
        self.resize_augmentation = A.CropResizeToAspectTransform(resize=resize)
        self.background_augmentation = background_augmentation
        self.background_augmentations = A.make_background_augmentations()
        # the members of make_rgb_augmentations() without its outer p = 0.8: the reference draws that one with random.random()
        self.rgb_augmentations = [A.SceneObservationAugmentation(A.make_rgb_augmentations()[0].transform)]
        self.label_to_category_id = label_to_category_id
        self.min_area = min_area

    def make_batch(self, batch: A.ObservationBatch, object_datas: Sequence[Sequence[Any]], rng: np.random.Generator,
                   image_ids: Optional[Sequence[int]] = None):
        B, dev = _check_batch(batch, object_datas, "DetectionDataset.make_batch")
        ids = _unique_ids(object_datas)
        batch = dataclasses.replace(batch, object_ids=ids)
        batch = self.resize_augmentation(batch, rng)
        if batch.background is not None:
            batch = A.apply_augmentations(self.background_augmentations, batch, rng)
        elif self.background_augmentation:
            raise ValueError("DetectionDataset.make_batch: background_augmentation needs batch.background")
        gate = rng.random(B) < RGB_CHAIN_P
        for aug in self.rgb_augmentations:
            batch = aug.apply(batch, aug.draw(B, rng), gate)
        seg = batch.segmentation
        H, W = int(seg.shape[1]), int(seg.shape[2])
        boxes_d, n_px_d = ops.seg_boxes(seg, ids)
        max_ids = int(n_px_d.shape[1])
        table = torch.cat([boxes_d, n_px_d[..., None]], dim=2).cpu().numpy().astype(np.int64)  # the one read-back
        id_table = np.zeros((B, max_ids), np.int32)
        slot_row = np.full((B, max_ids), -1, np.int32)
        per_frame, G = [], 0
        for b, objs in enumerate(object_datas):
            id_table[b, :len(objs)] = ids[b]
            visible = [k for k in range(len(objs)) if table[b, k, 4] > 0]
            bx = table[b, visible, :4].reshape(-1, 4)
            area = (bx[:, 3] - bx[:, 1]) * (bx[:, 2] - bx[:, 0])
            keep = area > self.min_area
            kept = [k for k, f in zip(visible, keep) if f]
            slot_row[b, kept] = np.arange(G, G + len(kept), dtype=np.int32)
            per_frame.append((G, kept, bx[keep], area[keep], len(visible)))
            G += len(kept)
        masks = ops.instance_masks(seg, id_table, slot_row, G, count=np.array([len(r) for r in ids], np.int32))
        targets = []
        for b, (g0, kept, bx, area, n_visible) in enumerate(per_frame):
            labels = [self.label_to_category_id[_field(object_datas[b][k], "label")] for k in kept]
            targets.append({
                "boxes": torch.as_tensor(bx.astype(np.float32)).reshape(-1, 4).to(dev),
                "labels": torch.as_tensor(labels, dtype=torch.int64).reshape(-1).to(dev),
                "masks": masks[g0:g0 + len(kept)].reshape(-1, H, W),
                "image_id": torch.tensor([b if image_ids is None else int(image_ids[b])]),
                "area": torch.as_tensor(area.astype(np.int64)).reshape(-1).to(dev),
                "iscrowd": torch.zeros(n_visible, dtype=torch.int64),
            })
        return batch.rgb, targets
