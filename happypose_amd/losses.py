"""The losses the pose networks are trained and validated on, on the device, with gradients (``csrc/pose_losses.hip``).

Names and argument orders are the reference's (``TB/lib3d/cosypose_ops.py``, ``CP/lib3d/cosypose_ops.py``,
``TB/lib3d/mesh_losses.py``); definitions are in ``include/happypose_amd.h``.  This is the loss layer, not a trainer: what it
gives is the value the reference logs as ``loss_TCO-iter=k`` (with ``-loss_orn``, ``-loss_xy``, ``-loss_z``) and its gradient
with respect to the network's 9-D output (the refiner losses) or the upper 3 x 4 of ``TCO_pred`` (``loss_CO_symmetric``,
``compute_ADD_L1_loss``), and ``renderings_confidence_loss``, the logits loss of MegaPose's coarse classifier
(``MP/training/megapose_forward_loss.py:224-239``), with its gradient with respect to the logits.

Differences from the reference, all deliberate:

* only ``loss`` is differentiable, and only with respect to ``refiner_outputs`` / ``TCO_pred``: the reference detaches
  ``TCO_input`` between iterations and the other inputs are data.  The parts in ``loss_data`` and ``TCO_assign`` come back
  detached (the reference keeps them in the graph but uses them for meters only);
* ``l1_or_l2=l2`` is not offered (no caller of the reference passes it) and raises ``NotImplementedError``;
* inputs are float32 tensors on one GPU (other float dtypes are converted, non-contiguous tensors are made contiguous); a CPU
  tensor raises ``ValueError``: there is no CPU path;
* a row with a non-finite input or a degenerate 6-D rotation part gives NaN for the row's loss, parts and gradient.
"""

from __future__ import annotations

from typing import Dict, Tuple

import torch

from . import ops

__all__ = ["l1", "l2", "loss_CO_symmetric", "compute_ADD_L1_loss", "loss_refiner_CO_disentangled",
           "loss_refiner_CO_disentangled_reference_point", "renderings_confidence_loss"]


def l1(diff):
    return diff.abs()


def l2(diff):
    return diff ** 2


def _only_l1(l1_or_l2) -> None:
    if l1_or_l2 is not l1:
        raise NotImplementedError("happypose_amd.losses: only l1_or_l2=l1 has a kernel")


class _SymmetricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, TCO_pred, TCO_possible_gt, points):
        loss, sym_id, assign = ops.loss_co_symmetric_forward(TCO_possible_gt, TCO_pred, points)
        ctx.save_for_backward(TCO_pred, TCO_possible_gt, points, sym_id)
        ctx.mark_non_differentiable(assign)
        return loss, assign

    @staticmethod
    def backward(ctx, grad_loss, _grad_assign):
        TCO_pred, TCO_possible_gt, points, sym_id = ctx.saved_tensors
        grad = ops.loss_co_symmetric_backward(TCO_possible_gt, TCO_pred, points, sym_id, grad_loss)
        return grad.to(TCO_pred.dtype), None, None


class _RefinerLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, refiner_outputs, TCO_possible_gt, TCO_input, K_crop, points, tCR):
        loss, parts, sym_ids = ops.loss_refiner_forward(TCO_possible_gt, TCO_input, refiner_outputs, K_crop, points, tCR)
        ctx.has_tCR = tCR is not None
        saved = [refiner_outputs, TCO_possible_gt, TCO_input, K_crop, points, sym_ids]
        ctx.save_for_backward(*saved, *([tCR] if ctx.has_tCR else []))
        ctx.mark_non_differentiable(parts)
        return loss, parts

    @staticmethod
    def backward(ctx, grad_loss, _grad_parts):
        refiner_outputs, TCO_possible_gt, TCO_input, K_crop, points, sym_ids = ctx.saved_tensors[:6]
        tCR = ctx.saved_tensors[6] if ctx.has_tCR else None
        grad = ops.loss_refiner_backward(TCO_possible_gt, TCO_input, refiner_outputs, K_crop, points, tCR, sym_ids, grad_loss)
        return grad.to(refiner_outputs.dtype), None, None, None, None, None


class _BCELogitsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, is_positive, temperature):
        loss = ops.loss_bce_logits_forward(logits, is_positive, temperature)
        ctx.save_for_backward(logits, is_positive)
        ctx.temperature = float(temperature)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        logits, is_positive = ctx.saved_tensors
        grad = ops.loss_bce_logits_backward(logits, is_positive, ctx.temperature, grad_loss)
        return grad.to(logits.dtype), None, None


def loss_CO_symmetric(TCO_possible_gt: torch.Tensor, TCO_pred: torch.Tensor, points: torch.Tensor,
                      l1_or_l2=l1) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(loss [B], TCO_assign [B, 4, 4])``: the smallest mean ``|TCO_pred p - TCO_possible_gt[:, s] p|`` over the symmetries
    ``s`` and the ground-truth pose that gave it."""
    _only_l1(l1_or_l2)
    return _SymmetricLoss.apply(TCO_pred, TCO_possible_gt, points)


def compute_ADD_L1_loss(TCO_gt: torch.Tensor, TCO_pred: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """Mean ``|TCO_gt p - TCO_pred p|`` per row: the symmetric loss with one candidate."""
    assert TCO_gt.dim() == 3 and TCO_gt.shape[-2:] == (4, 4) and TCO_pred.shape == TCO_gt.shape
    return _SymmetricLoss.apply(TCO_pred, TCO_gt.unsqueeze(1), points)[0]


def loss_refiner_CO_disentangled(TCO_possible_gt: torch.Tensor, TCO_input: torch.Tensor, refiner_outputs: torch.Tensor,
                                 K_crop: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """CosyPose's disentangled loss of the image-space update: ``loss [B]``."""
    return _RefinerLoss.apply(refiner_outputs, TCO_possible_gt, TCO_input, K_crop, points, None)[0]


def loss_refiner_CO_disentangled_reference_point(TCO_possible_gt: torch.Tensor, TCO_input: torch.Tensor, refiner_outputs: torch.Tensor,
                                                 K_crop: torch.Tensor, points: torch.Tensor,
                                                 tCR: torch.Tensor) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """MegaPose's disentangled loss of the update about the reference point ``tCR``: ``(loss [B], loss_data)`` with
    ``loss_data = {loss_orn, loss_xy, loss_z, loss}``, all ``[B]`` and detached."""
    assert tCR is not None, "loss_refiner_CO_disentangled_reference_point: tCR [B, 3]"
    loss, parts = _RefinerLoss.apply(refiner_outputs, TCO_possible_gt, TCO_input, K_crop, points, tCR)
    return loss, {"loss_orn": parts[:, 0], "loss_xy": parts[:, 1], "loss_z": parts[:, 2], "loss": loss.detach()}


def renderings_confidence_loss(logits: torch.Tensor, is_positive: torch.Tensor, temperature: float = 1.0) -> torch.Tensor:
    """The coarse classifier's rendered-views-logits loss (``MP/training/megapose_forward_loss.py:224-239``):
    ``nn.BCEWithLogitsLoss(reduction="none")(logits / temperature, is_positive)`` per element, in the stable form
    ``max(x, 0) - x y + log1p(exp(-|x|))``; the result has the shape of ``logits``.  Differentiable with respect to ``logits``
    only: ``(sigmoid(x) - y) / temperature``."""
    return _BCELogitsLoss.apply(logits, is_positive, temperature)
