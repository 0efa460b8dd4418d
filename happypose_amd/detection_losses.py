"""The detector's training targets and losses on the device, with gradients (``csrc/det_losses.hip``).

What torchvision 0.14's train-mode ``MaskRCNN.forward`` computes between the networks, under torchvision's names and argument
orders: ``RegionProposalNetwork.assign_targets_to_anchors`` and ``compute_loss`` (``models/detection/rpn.py``),
``RoIHeads.select_training_samples``, ``fastrcnn_loss``, ``project_masks_on_boxes`` and ``maskrcnn_loss``
(``models/detection/roi_heads.py``), over ``Matcher``, ``BalancedPositiveNegativeSampler`` and ``BoxCoder``
(``models/detection/_utils.py``), ``box_iou`` (``ops/boxes.py``) and ``roi_align`` (``ops/roi_align.py``).  Definitions are in
``include/happypose_amd.h``.

torchvision is not available beside this library, so parity with it is **unpinned**: the algorithm is restated from its
published definitions and pinned by the float64 restatement ``tests/det_losses_ref.py``.

Differences from torchvision, all deliberate:

* sampling: the ``k`` rows a class keeps are those with the smallest ``(Philox key, row)`` of an explicit ``seed``; the counts
  ``k`` are torchvision's, torch's ``randperm`` stream is not reproduced;
* only the losses are differentiable, and only with respect to the network outputs (``objectness``, ``pred_bbox_deltas``,
  ``class_logits``, ``box_regression``, ``mask_logits``); targets and labels are data;
* inputs live on one GPU; a CPU tensor raises ``ValueError``: there is no CPU path;
* a non-finite network output in a row makes the loss, and that row's gradient, NaN.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops

__all__ = ["box_encode", "rpn_assign_targets_to_anchors", "rpn_compute_loss", "roi_select_training_samples", "fastrcnn_loss",
           "project_masks_on_boxes", "maskrcnn_loss"]

RPN_FG_IOU, RPN_BG_IOU, RPN_BATCH, RPN_POSITIVE = 0.7, 0.3, 256, 0.5         # torchvision MaskRCNN defaults
BOX_FG_IOU, BOX_BG_IOU, BOX_BATCH, BOX_POSITIVE = 0.5, 0.5, 512, 0.25
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
STREAM_RPN, STREAM_BOX = 1, 2  # word 2 of the Philox counter


class _RpnLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, objectness, pred_deltas, labels, targets, sampled):
        loss, g_obj, g_del = ops.loss_rpn(objectness, pred_deltas, labels, targets, sampled)
        ctx.save_for_backward(g_obj, g_del)
        ctx.shapes = (objectness.shape, objectness.dtype, pred_deltas.shape, pred_deltas.dtype)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        g_obj, g_del = ctx.saved_tensors
        so, do, sd, dd = ctx.shapes
        return (g_obj * grad_loss[0]).reshape(so).to(do), (g_del * grad_loss[1]).reshape(sd).to(dd), None, None, None


class _FastRcnnLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, class_logits, box_regression, labels, targets, num_classes):
        loss, g_cls, g_reg = ops.loss_fastrcnn(class_logits, box_regression, labels, targets, num_classes)
        ctx.save_for_backward(g_cls, g_reg)
        ctx.dtypes = (class_logits.dtype, box_regression.dtype)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        g_cls, g_reg = ctx.saved_tensors
        return (g_cls * grad_loss[0]).to(ctx.dtypes[0]), (g_reg * grad_loss[1]).to(ctx.dtypes[1]), None, None, None


class _MaskLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mask_logits, labels, targets):
        loss, grad = ops.loss_mask(mask_logits, labels, targets)
        ctx.save_for_backward(grad)
        ctx.dtype = mask_logits.dtype
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (grad,) = ctx.saved_tensors
        return (grad * grad_loss[0]).to(ctx.dtype), None, None


# ---- the batch as one table ---------------------------------------------------------------------------------------------------------
def _rows(per_image: Sequence[torch.Tensor], what: str):
    """Per-image row tensors -> ``(all rows, image_of [n] int32, counts)``."""
    dev = ops._on_device(what, **{f"{what}[{i}]": t for i, t in enumerate(per_image)})
    counts = [int(t.shape[0]) for t in per_image]
    image_of = torch.repeat_interleave(torch.arange(len(per_image), dtype=torch.int32, device=dev),
                                       torch.tensor(counts, device=dev))
    return torch.cat(list(per_image)), image_of, counts


def _gt_table(targets: Sequence[Dict[str, torch.Tensor]], what: str):
    """``(gt boxes [G, 4], gt_off [B + 1] (host list), gt labels [G] or None)`` of the batch."""
    boxes = [t["boxes"].reshape(-1, 4).float() for t in targets]
    ops._on_device(what, **{f"targets[{i}].boxes": b for i, b in enumerate(boxes)})
    off = [0]
    for b in boxes:
        off.append(off[-1] + int(b.shape[0]))
    labels = torch.cat([t["labels"].reshape(-1) for t in targets]) if all("labels" in t for t in targets) else None
    return torch.cat(boxes), off, labels


def _encode_match(match: torch.Tensor, image_of: torch.Tensor, gt_off: List[int]) -> torch.Tensor:
    """torchvision encodes against ``gt_boxes[matched_idxs.clamp(min=0)]``: background and discarded rows take the FIRST ground
    truth of their image (the zero box in an image without ground truths)."""
    off = torch.tensor(gt_off, dtype=torch.int32, device=match.device)
    first = off[:-1][image_of.long()]
    first = torch.where(off[1:][image_of.long()] > first, first, torch.full_like(first, -1))
    return torch.where(match >= 0, match, first)


def _split(t: torch.Tensor, counts: List[int]) -> List[torch.Tensor]:
    return list(torch.split(t, counts))


def box_encode(reference_boxes: torch.Tensor, proposals: torch.Tensor, weights=(1.0, 1.0, 1.0, 1.0)) -> torch.Tensor:
    """``BoxCoder(weights).encode_single(reference_boxes, proposals)``: ``[n, 4]`` each -> the regression targets ``[n, 4]``."""
    ops._on_device("box_encode", reference_boxes=reference_boxes, proposals=proposals)
    assert reference_boxes.shape == proposals.shape, "box_encode: one reference box per proposal"
    rows = torch.arange(proposals.shape[0], dtype=torch.int32, device=proposals.device)
    return ops.det_box_encode(proposals, rows, reference_boxes, weights)


# ---- RegionProposalNetwork ------------------------------------------------------------------------------------------------------------
def rpn_assign_targets_to_anchors(anchors: List[torch.Tensor], targets: List[Dict[str, torch.Tensor]], *, fg_iou_thresh: float = RPN_FG_IOU,
                                  bg_iou_thresh: float = RPN_BG_IOU, return_matches: bool = False):
    """``(labels, matched_gt_boxes)`` per image: labels float32 1 (IoU >= ``fg_iou_thresh`` or a low-quality match), 0 (below
    ``bg_iou_thresh``; every anchor of an image without ground truths), -1 (between: not sampled).  ``return_matches``: also the
    ``Matcher``'s indices per image (into the image's own ground truths; -1 / -2 as in torchvision)."""
    all_anchors, image_of, counts = _rows(anchors, "anchors")
    gt, gt_off, _ = _gt_table(targets, "rpn_assign_targets_to_anchors")
    assert len(targets) == len(anchors)
    match, _ = ops.det_assign(all_anchors, image_of, gt, gt_off, fg_iou_thresh, bg_iou_thresh, allow_low_quality=True)
    labels = torch.where(match >= 0, 1.0, torch.where(match == -1, 0.0, -1.0)).to(torch.float32)
    enc = _encode_match(match, image_of, gt_off)
    table = torch.cat([gt, gt.new_zeros(1, 4)])  # row G: the zero box
    matched = table[torch.where(enc >= 0, enc, torch.full_like(enc, gt.shape[0])).long()]
    out = (_split(labels, counts), _split(matched, counts))
    if return_matches:
        off = torch.tensor(gt_off[:-1], dtype=torch.int32, device=match.device)[image_of.long()]
        out += (_split(torch.where(match >= 0, match - off, match), counts),)
    return out


def rpn_compute_loss(objectness: torch.Tensor, pred_bbox_deltas: torch.Tensor, labels: List[torch.Tensor],
                     regression_targets: List[torch.Tensor], *, batch_size_per_image: int = RPN_BATCH,
                     positive_fraction: float = RPN_POSITIVE, seed: int = 0, return_sampled: bool = False):
    """``(loss_objectness, loss_rpn_box_reg)``: ``objectness [sum A]`` (or ``[sum A, 1]``) and ``pred_bbox_deltas [sum A, 4]`` of
    all images in image order, ``labels`` / ``regression_targets`` per image.  Binary cross-entropy over the sampled anchors and
    smooth L1 (``beta = 1 / 9``) over the sampled positives, both divided by the number of sampled anchors.
    ``return_sampled``: also the sampled rows (positives of all images first, as torchvision concatenates them)."""
    lab, image_of, _ = _rows(labels, "labels")
    tgt = torch.cat(list(regression_targets))
    picked = ops.det_sample(lab, image_of, len(labels), batch_size_per_image, positive_fraction, seed, STREAM_RPN)
    sampled = torch.cat([p for p, _ in picked] + [n for _, n in picked])
    loss = _RpnLoss.apply(objectness, pred_bbox_deltas, lab.to(torch.int32), tgt, sampled)
    out = (loss[0], loss[1])
    return out + (sampled,) if return_sampled else out


# ---- RoIHeads -------------------------------------------------------------------------------------------------------------------------
def roi_select_training_samples(proposals: List[torch.Tensor], targets: List[Dict[str, torch.Tensor]], *, fg_iou_thresh: float = BOX_FG_IOU,
                                bg_iou_thresh: float = BOX_BG_IOU, batch_size_per_image: int = BOX_BATCH,
                                positive_fraction: float = BOX_POSITIVE, bbox_reg_weights=BOX_WEIGHTS, seed: int = 0):
    """``(proposals, matched_idxs, labels, regression_targets)`` per image, as ``RoIHeads.select_training_samples``: the ground
    truths are appended to the proposals, matched (no low-quality matches), labelled (0 background, -1 between the thresholds),
    sampled, and the regression targets encoded.  ``matched_idxs`` index the image's own ground truths (clamped at 0)."""
    assert len(proposals) == len(targets)
    gt, gt_off, gt_labels = _gt_table(targets, "roi_select_training_samples")
    assert gt_labels is not None, "roi_select_training_samples: targets need labels"
    props = [torch.cat([p.float(), t["boxes"].reshape(-1, 4).float()]) for p, t in zip(proposals, targets)]  # add_gt_proposals
    rows, image_of, counts = _rows(props, "proposals")
    match, _ = ops.det_assign(rows, image_of, gt, gt_off, fg_iou_thresh, bg_iou_thresh, allow_low_quality=False)
    lab_table = torch.cat([gt_labels.to(torch.int64), gt_labels.new_zeros(1, dtype=torch.int64)])
    labels = lab_table[torch.where(match >= 0, match, torch.full_like(match, gt.shape[0])).long()]
    labels = torch.where(match == -2, torch.full_like(labels, -1), labels)
    picked = ops.det_sample(labels, image_of, len(props), batch_size_per_image, positive_fraction, seed, STREAM_BOX)
    keep = [torch.cat([p, n]).sort().values for p, n in picked]  # torch.where(pos | neg): ascending
    enc = _encode_match(match, image_of, gt_off)
    out_p, out_m, out_l, out_t = [], [], [], []
    for b, k in enumerate(keep):
        out_p.append(rows[k])
        out_m.append((match[k] - gt_off[b]).clamp(min=0).to(torch.int64))
        out_l.append(labels[k])
        out_t.append(ops.det_box_encode(rows[k], enc[k], gt, bbox_reg_weights))
    return out_p, out_m, out_l, out_t


def fastrcnn_loss(class_logits: torch.Tensor, box_regression: torch.Tensor, labels: List[torch.Tensor],
                  regression_targets: List[torch.Tensor], num_classes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(classification_loss, box_loss)``: mean softmax cross-entropy over all rows, and smooth L1 (``beta = 1 / 9``) over the
    regression values of each positive row's own class, divided by the number of rows.  ``num_classes`` (not in torchvision):
    ``class_logits`` may carry padding columns beyond it; they are ignored and receive a zero gradient."""
    lab = torch.cat(list(labels)) if not isinstance(labels, torch.Tensor) else labels
    tgt = torch.cat(list(regression_targets)) if not isinstance(regression_targets, torch.Tensor) else regression_targets
    loss = _FastRcnnLoss.apply(class_logits, box_regression, lab, tgt, num_classes)
    return loss[0], loss[1]


def project_masks_on_boxes(gt_masks: torch.Tensor, boxes: torch.Tensor, matched_idxs: torch.Tensor, M: int) -> torch.Tensor:
    """``roi_align(gt_masks[matched_idxs][:, None], boxes, (M, M), 1.0)[:, 0]``: ``gt_masks [g, H, W]`` uint8 -> ``[n, M, M]``."""
    return ops.det_mask_targets(gt_masks, matched_idxs, boxes, M)


def maskrcnn_loss(mask_logits: torch.Tensor, proposals: List[torch.Tensor], gt_masks: List[torch.Tensor], gt_labels: List[torch.Tensor],
                  mask_matched_idxs: List[torch.Tensor], *, return_targets: bool = False):
    """Mean binary cross-entropy of ``mask_logits[i, label_i]`` ``[n, C, M, M]`` against the ground-truth masks projected on the
    proposals.  No proposals: 0.  ``return_targets``: also ``(labels [n], mask_targets [n, M, M])``."""
    ops._on_device("maskrcnn_loss", mask_logits=mask_logits)
    M = mask_logits.shape[-1]
    labels = torch.cat([gl.reshape(-1)[idx] for gl, idx in zip(gt_labels, mask_matched_idxs)]) if len(gt_labels) else \
        torch.zeros(0, dtype=torch.int64, device=mask_logits.device)
    parts = [project_masks_on_boxes(m, p, i, M) for m, p, i in zip(gt_masks, proposals, mask_matched_idxs) if p.shape[0]]
    mask_targets = torch.cat(parts) if parts else mask_logits.new_zeros(0, M, M, dtype=torch.float32)
    loss = _MaskLoss.apply(mask_logits, labels, mask_targets)[0]
    return (loss, labels, mask_targets) if return_targets else loss
