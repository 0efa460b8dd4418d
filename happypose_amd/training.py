"""The trainers' forward-loss step on the device: a batch in, the reference's validation numbers and the gradient at the network's
output out.

Names and argument orders are the reference's: ``h_pose`` (``CP/training/pose_forward_loss.py``), ``megapose_forward_loss``
(``MP/training/megapose_forward_loss.py``), ``add_noise`` (``TB/lib3d/transform_ops.py:70-104``), ``TCO_init_from_boxes`` and
``TCO_init_from_boxes_zup_autodepth`` (``TB/lib3d/cosypose_ops.py:159-283``).  The hypotheses are made by ``csrc/train_hyp.hip``
(``ops.pose_add_noise``, ``ops.tco_init_from_boxes``, ``ops.coarse_hypotheses``) and ``ops.tco_init_autodepth``, the predictor is one
of this library's, the losses are ``happypose_amd.losses``: every input and every intermediate stays on the device.

This is the step, not a trainer.  Each iteration's ``network_outputs["pose"]`` is marked ``requires_grad_()`` before the loss, so
``loss.backward()`` leaves ``dL/dpose`` in its ``.grad`` (``debug_dict["outputs"]["iteration=k"].network_outputs["pose"].grad``):
the hand-over point for whatever trains a head.  The forward-loss functions run no network backward and no optimiser;
``HeadTrainer`` (at the end of this module) is the consumer that does, for the linear heads on a frozen backbone.

Differences from the reference, all deliberate:

* random numbers: the reference draws from the global ``np.random`` stream; here every draw is a function of an explicit ``seed``
  (Philox4x32-10 for the pose noise, ``RandomState(seed)`` for the ids of the loss points) and repeats bit for bit.  The
  reference's stream is not reproduced;
* sequence: the reference reads every meter value back with ``.item()`` -- ``4 n_iterations + 2`` synchronisations a step; here
  the values are collected on the device and read back once, after the loss is formed.  The values and their order of addition
  to the meters are the reference's;
* ``n_hypotheses`` copies of a ground truth are made inside the noise launch, images and intrinsics are indexed per hypothesis
  (``im_ids``) instead of gathered;
* the auto-depth initialisations use the deterministic point subset of the estimators (``MeshStore.point_ids``) where the
  reference samples one at random;
* the coarse classifier's hypotheses (``coarse_classif_multiview_paper``): the reference builds the 104 ``sphere_26views``
  candidates of every image on the host with Panda3D node paths and draws from ``np.random``; here ``ops.coarse_hypotheses``
  draws and evaluates only the selected candidates in one launch.  The look-at is this library's closed form; where the up hint
  is parallel to the viewing direction the header states this library's own rule;
* not built: ``coarse_classif_multiview_SO3_grid`` (raises in the reference too), ``coarse_classif_multiview_paper`` without
  ``cfg.predict_rendered_views_logits`` (the reference asserts the flag), ``n_pose_dims == 7`` (no quaternion loss kernel),
  ``random_ambient_light``, and the bokeh visualisation (``make_visualization=True`` raises).
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import detection_losses, losses, ops

__all__ = ["AverageValueMeter", "TrainingConfig", "CosyPoseTrainingConfig", "DetectorTrainingConfig", "add_noise", "TCO_init_from_boxes",
           "TCO_init_from_boxes_zup_autodepth", "make_hypotheses", "h_pose", "megapose_forward_loss", "h_maskrcnn", "HeadOptimConfig",
           "HeadTrainer"]

MEGAPOSE_METHODS = ("coarse_z_up+auto-depth", "refiner_gt+noise")
COSYPOSE_METHODS = ("fixed", "gt+noise", "fixed+trans_noise")
AUTODEPTH_POINTS = 200  # MP/training/megapose_forward_loss.py:83-85


class AverageValueMeter:
    """What the forward-loss functions need of ``torchnet.meter.AverageValueMeter``: ``add(value, n=1)``, ``value() -> (mean,
    std)``, ``reset()`` and the fields ``n``, ``sum``, ``mean``, ``std``."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self.n, self.sum, self._sq = 0, 0.0, 0.0
        self.mean, self.std = math.nan, math.nan

    def add(self, value: float, n: int = 1) -> None:
        self.n += n
        self.sum += value
        self._sq += value * value
        self.mean = self.sum / self.n
        if self.n == 1:
            self.std = math.inf
        else:  # unbiased, from the running sums
            self.std = math.sqrt(max(self._sq - self.n * self.mean * self.mean, 0.0) / (self.n - 1.0))

    def value(self) -> Tuple[float, float]:
        return self.mean, self.std


@dataclass
class TrainingConfig:
    """The fields ``megapose_forward_loss`` reads, with the defaults of ``MP/training/training_config.py`` -- but for
    ``random_ambient_light`` (reference: True), which this renderer does not offer: True raises."""

    hypotheses_init_method: str = "refiner_gt+noise"
    n_hypotheses: int = 1
    init_euler_deg_std: Tuple[float, float, float] = (15, 15, 15)
    init_trans_std: Tuple[float, float, float] = (0.01, 0.01, 0.05)
    random_ambient_light: bool = False
    n_points_loss: int = 2000
    loss_alpha_pose: float = 1.0
    predict_pose_update: bool = True
    predict_rendered_views_logits: bool = False
    n_rendered_views: int = 1
    renderings_logits_temperature: float = 1.0
    loss_alpha_renderings_confidence: float = 1.0


@dataclass
class CosyPoseTrainingConfig:
    """The fields ``h_pose`` reads, with the values of ``CP/scripts/run_pose_training.py``."""

    n_points_loss: int = 2600
    loss_disentangled: bool = True
    n_pose_dims: int = 9
    init_method: str = "v0"


@dataclass
class DetectorTrainingConfig:
    """The fields ``h_maskrcnn`` reads, with the values of ``CP/scripts/run_detector_training.py:78-82``."""

    rpn_box_reg_alpha: float = 1
    objectness_alpha: float = 1
    classifier_alpha: float = 1
    mask_alpha: float = 1
    box_reg_alpha: float = 1


# ---- primitives -------------------------------------------------------------------------------------------------------------------
def add_noise(TCO: torch.Tensor, euler_deg_std=(15, 15, 15), trans_std=(0.01, 0.01, 0.05), *, seed: int, row_offset: int = 0,
              repeat: int = 1, return_noise: bool = False):
    """``TCO [m, 4, 4]`` on the device -> ``[m * repeat, 4, 4]``: ``R R_noise``, ``t + dt`` with ``R_noise = euler2mat`` (static
    xyz) of normal angles (degrees) and normal ``dt`` (metres).  Row ``i`` is drawn from ``(seed, row_offset + i)`` alone
    (``hp_pose_add_noise`` in ``include/happypose_amd.h`` states the counter layout); a standard deviation of 0 leaves that part
    of the pose bit for bit.  ``return_noise``: also ``[m * repeat, 6]``, the angles in radians and ``dt``."""
    return ops.pose_add_noise(TCO, euler_deg_std, trans_std, seed=seed, row_offset=row_offset, repeat=repeat, return_noise=return_noise)


def TCO_init_from_boxes(z_range, boxes: torch.Tensor, K: torch.Tensor) -> torch.Tensor:
    """Identity rotation at depth ``mean(z_range)`` behind the box centre: ``[B, 4, 4]``."""
    assert len(z_range) == 2
    assert boxes.dim() == 2 and boxes.shape[-1] == 4
    return ops.tco_init_from_boxes(boxes, K, z_range)


def TCO_init_from_boxes_zup_autodepth(boxes_2d: torch.Tensor, store, K: torch.Tensor, *, labels: Sequence[str],
                                      n_points: Optional[int] = None) -> torch.Tensor:
    """z-up rotation, depth from the extent of the object's points against the box (``ops.tco_init_autodepth``).  Where the
    reference takes ``model_points_3d``, this takes the ``MeshStore`` that holds the point table on the device and the
    ``labels`` of the rows; ``n_points``: the deterministic subset of that many points (None: all)."""
    if not isinstance(store, ops.MeshStore):
        raise TypeError("TCO_init_from_boxes_zup_autodepth: the kernel reads the point table of a MeshStore (model.store), "
                        "not a tensor of points")
    ops._on_device("TCO_init_from_boxes_zup_autodepth", boxes_2d=boxes_2d, K=K)
    n = boxes_2d.shape[0]
    assert len(labels) == n and K.shape[0] == n
    ids = torch.arange(n, dtype=torch.int32, device=store.device)
    return ops.tco_init_autodepth(store, boxes_2d, K, ids, store.ids_of(list(labels)), n_points=n_points)


# ---- the batch ----------------------------------------------------------------------------------------------------------------------
def _labels(data) -> List[str]:
    if getattr(data, "object_datas", None) is not None:
        return [o["label"] if isinstance(o, dict) else o.label for o in data.object_datas]
    return [str(l) for l in data.labels]


def _batch(data, what: str) -> Dict[str, Any]:
    """``rgbs`` (uint8 ``[B, 3, H, W]``, or an ``ObservationBatch`` whose ``rgb`` is ``[B, H, W, 3]``), ``depths``, ``K``,
    ``TCO``, ``bboxes`` as float32 tensors on one device, and the labels."""
    rgbs, depths = data.rgbs, getattr(data, "depths", None)
    if hasattr(rgbs, "rgb"):  # ObservationBatch
        depths = rgbs.depth if depths is None else depths
        rgbs = rgbs.rgb.permute(0, 3, 1, 2)
    dev = ops._on_device(what, rgbs=rgbs, depths=depths, K=data.K, TCO=data.TCO, bboxes=data.bboxes)
    assert rgbs.dim() == 4 and rgbs.shape[1] == 3 and rgbs.dtype == torch.uint8, f"{what}: rgbs uint8 [B, 3, H, W]"
    b = rgbs.shape[0]
    labels = _labels(data)
    K, TCO, bboxes = data.K.float(), data.TCO.float(), data.bboxes.float()
    assert K.shape == (b, 3, 3) and TCO.shape == (b, 4, 4) and bboxes.shape == (b, 4) and len(labels) == b, f"{what}: one object per image"
    return dict(rgbs=rgbs, depths=depths, K=K.contiguous(), TCO=TCO.contiguous(), bboxes=bboxes.contiguous(), labels=labels, device=dev, B=b)


def _images(bt, input_depth: bool) -> torch.Tensor:
    """``cast_images``: rgb in [0, 1], the depth (metres) as a fourth channel when the model reads one."""
    images = bt["rgbs"].float() / 255.0
    if input_depth:
        assert bt["depths"] is not None, "the model reads depth: data.depths [B, H, W]"
        d = bt["depths"].float()
        images = torch.cat([images, d.reshape(bt["B"], 1, *images.shape[-2:])], dim=1)
    return images.contiguous()


def _loss_tables(mesh_db, labels, TCO_gt: torch.Tensor, n_points: int, seed: int):
    """``points [B, n_points, 3]`` (a seeded subset of the padded table, the same ids for every object as in the reference) and
    ``TCO_possible_gt [B, S, 4, 4] = TCO_gt @ symmetries``."""
    meshes = mesh_db.select(labels)
    if not isinstance(meshes.points, torch.Tensor) or not meshes.points.is_cuda:
        raise ValueError("mesh_db lives on the host: pass MeshDataBase.from_object_ds(ds).batched().to(device)")
    n_pad = meshes.points.shape[1]
    assert n_points <= n_pad, f"n_points_loss = {n_points} but the objects have {n_pad} points"
    ids = np.random.RandomState(seed & 0xFFFFFFFF).choice(n_pad, size=n_points, replace=False)
    points = meshes.points[:, torch.as_tensor(ids, device=meshes.points.device)].float().contiguous()
    sym = meshes.symmetries.float()
    # T_gt @ S as products and sums of elementwise kernels: a fixed order of additions, no BLAS
    possible = (TCO_gt[:, None, :, :, None] * sym[:, :, None, :, :]).sum(3)
    return points, possible.contiguous()


def _seed(seed: int, stream: int) -> int:
    """One 64-bit Philox key per use of ``seed`` inside a step."""
    return (int(seed) * 0x9E3779B97F4A7C15 + stream) & 0xFFFFFFFFFFFFFFFF


def make_hypotheses(method: str, data, mesh_db, cfg, seed: int, *, store=None, return_labels: bool = False):
    """The initial hypotheses of a step, ``[B, n_hypotheses, 4, 4]`` on the device.  MegaPose's ``cfg.hypotheses_init_method``:
    ``"coarse_z_up+auto-depth"`` (one hypothesis), ``"refiner_gt+noise"``, ``"coarse_classif_multiview_paper"``; CosyPose's
    ``input_generator``: ``"fixed"``, ``"gt+noise"``, ``"fixed+trans_noise"`` (one hypothesis each).  ``store``: the predictor's
    ``MeshStore``, for the auto-depth methods.  ``mesh_db`` is not read by the methods that are built; it keeps the reference's
    place in the argument list.

    ``"coarse_classif_multiview_paper"`` (the coarse classifier; the reference asserts ``cfg.predict_rendered_views_logits`` for
    it): one noisy copy of each ground truth (``add_noise`` with ``cfg.init_euler_deg_std`` / ``cfg.init_trans_std``, key
    ``_seed(seed, 1)``), then ``cfg.n_hypotheses`` of its 104 ``sphere_26views`` candidates (``ops.coarse_hypotheses``, key
    ``_seed(seed, 4)``).  ``return_labels=True`` returns ``(hypotheses, is_positive [B, n_hyp] float32, view_ids [B, n_hyp]
    int32)`` -- ``(hypotheses, None, None)`` for the other methods, whose return type without the keyword is unchanged."""
    if method == "coarse_classif_multiview_SO3_grid":
        raise NotImplementedError  # as in the reference
    if method == "coarse_classif_multiview_paper":
        if not getattr(cfg, "predict_rendered_views_logits", False):
            raise NotImplementedError("coarse_classif_multiview_paper draws the hypotheses of the rendered-views-logits loss: "
                                      "set cfg.predict_rendered_views_logits = True (the reference asserts it)")
        bt = data if isinstance(data, dict) and "B" in data else _batch(data, "make_hypotheses")
        noisy = add_noise(bt["TCO"], cfg.init_euler_deg_std, cfg.init_trans_std, seed=_seed(seed, 1))
        hyp, view_ids, is_positive = ops.coarse_hypotheses(noisy, int(cfg.n_hypotheses), seed=_seed(seed, 4),
                                                           n_rendered_views=int(cfg.n_rendered_views))
        return (hyp, is_positive, view_ids) if return_labels else hyp
    if return_labels:
        return make_hypotheses(method, data, mesh_db, cfg, seed, store=store), None, None
    if method not in MEGAPOSE_METHODS + COSYPOSE_METHODS:
        raise ValueError("Unknown hypotheses method", method)
    bt = data if isinstance(data, dict) and "B" in data else _batch(data, "make_hypotheses")
    B, key = bt["B"], _seed(seed, 1)
    if method == "refiner_gt+noise":
        n_hyp = int(cfg.n_hypotheses)
        return add_noise(bt["TCO"], cfg.init_euler_deg_std, cfg.init_trans_std, seed=key, repeat=n_hyp).view(B, n_hyp, 4, 4)
    if method == "gt+noise":
        return add_noise(bt["TCO"], (15, 15, 15), (0.01, 0.01, 0.05), seed=key).view(B, 1, 4, 4)
    if method == "fixed":
        return TCO_init_from_boxes((1.0, 1.0), bt["bboxes"], bt["K"]).view(B, 1, 4, 4)
    # z-up + auto-depth, then translation noise only
    if method == "coarse_z_up+auto-depth":
        assert cfg.n_hypotheses == 1
        n_points = AUTODEPTH_POINTS
    else:
        assert cfg.init_method == "z-up+auto-depth"
        n_points = int(cfg.n_points_loss)
    if store is None:
        raise ValueError(f"make_hypotheses: {method!r} reads the point table of the predictor's MeshStore: pass store=model.store")
    init = TCO_init_from_boxes_zup_autodepth(bt["bboxes"], store, bt["K"], labels=bt["labels"], n_points=min(n_points, store.n_pad))
    return ops.pose_add_noise(init, (0, 0, 0), (0.01, 0.01, 0.05), seed=key, out=init).view(B, 1, 4, 4)


def _read_back(meters, keyed: List[Tuple[str, torch.Tensor]]) -> None:
    """The step's one read-back: the device scalars in one transfer, then the meters in the reference's order."""
    if keyed:
        for (key, _), v in zip(keyed, torch.stack([v.detach().reshape(()) for _, v in keyed]).tolist()):
            meters[key].add(v)


def _run_model(model, images, K, labels, hyp, n_iterations, **kw):
    B, n_hyp = hyp.shape[:2]
    im_ids = torch.arange(B, dtype=torch.int32, device=hyp.device).repeat_interleave(n_hyp)
    labels_h = [l for l in labels for _ in range(n_hyp)]
    return model(images=images, K=K, labels=labels_h, TCO=hyp.reshape(B * n_hyp, 4, 4), n_iterations=n_iterations, im_ids=im_ids, **kw)


# ---- CosyPose ---------------------------------------------------------------------------------------------------------------------
def h_pose(model, mesh_db, data, meters, cfg, n_iterations: int = 1, input_generator: str = "fixed", *, seed: int = 0,
           debug_dict: Optional[Dict[str, Any]] = None) -> torch.Tensor:
    """One forward-loss step of the CosyPose trainer: fills ``loss_TCO-iter=k``, ``loss_TCO`` and ``loss_total`` and returns the
    loss as a device scalar.  With ``cfg.loss_disentangled`` the gradient arrives at each iteration's
    ``network_outputs["pose"]``; with the ADD-L1 loss at its ``TCO_output``.  ``debug_dict`` (not in the reference) receives
    ``outputs``, ``hypotheses_TCO_init``, ``points`` and ``TCO_possible_gt``."""
    if cfg.loss_disentangled:
        if cfg.n_pose_dims == 7:
            raise NotImplementedError("n_pose_dims == 7: there is no quaternion loss kernel")
        if cfg.n_pose_dims != 9:
            raise ValueError(cfg.n_pose_dims)
    bt = _batch(data, "h_pose")
    images = _images(bt, False)
    points, TCO_possible_gt = _loss_tables(mesh_db, bt["labels"], bt["TCO"], int(cfg.n_points_loss), _seed(seed, 0))
    hyp = make_hypotheses(input_generator, bt, mesh_db, cfg, seed, store=getattr(model, "store", None))
    outputs = _run_model(model, images, bt["K"], bt["labels"], hyp, n_iterations)

    keyed, losses_TCO_iter = [], []
    for n in range(n_iterations):
        it = outputs[f"iteration={n + 1}"]
        if cfg.loss_disentangled:
            pose = it.network_outputs["pose"].requires_grad_()
            loss_TCO_iter = losses.loss_refiner_CO_disentangled(TCO_possible_gt=TCO_possible_gt, TCO_input=it.TCO_input,
                                                                refiner_outputs=pose, K_crop=it.K_crop, points=points)
        else:
            loss_TCO_iter = losses.compute_ADD_L1_loss(TCO_possible_gt[:, 0], it.TCO_output.requires_grad_(), points)
        keyed.append((f"loss_TCO-iter={n + 1}", loss_TCO_iter.mean()))
        losses_TCO_iter.append(loss_TCO_iter)
    loss_TCO = torch.cat(losses_TCO_iter).mean()
    loss = loss_TCO
    keyed += [("loss_TCO", loss_TCO), ("loss_total", loss)]
    _read_back(meters, keyed)
    if debug_dict is not None:
        debug_dict.update(outputs=outputs, hypotheses_TCO_init=hyp, points=points, TCO_possible_gt=TCO_possible_gt)
    return loss


# ---- MegaPose ---------------------------------------------------------------------------------------------------------------------
def megapose_forward_loss(model, cfg, data, meters, mesh_db, n_iterations: int, debug_dict: Optional[Dict[str, Any]],
                          make_visualization: bool = False, train: bool = True, is_notebook: bool = False, *,
                          seed: int = 0) -> torch.Tensor:
    """One forward-loss step of the MegaPose trainer: fills ``loss_TCO-iter=k``, ``loss_TCO-iter=k-loss_orn|loss_xy|loss_z``,
    ``time_render``, ``loss_TCO`` and ``loss_total`` and returns the loss as a device scalar; the gradient arrives at each
    iteration's ``network_outputs["pose"]``.  ``debug_dict`` receives the reference's ``outputs`` and ``time_render`` and, beyond
    them, ``hypotheses_TCO_init [B, n_hypotheses, 4, 4]``, ``points`` and ``TCO_possible_gt`` (per hypothesis row).  ``train``
    is accepted and, as in the reference, not read.

    The coarse classifier (``cfg.predict_rendered_views_logits`` with ``"coarse_classif_multiview_paper"``, one iteration, one
    rendered view): ``losses.renderings_confidence_loss`` of ``network_outputs["renderings_logits"]`` against the draw's
    ``is_positive`` fills ``loss_renderings_confidence`` (after ``loss_TCO``, before ``loss_total``) and its gradient arrives at
    ``network_outputs["renderings_logits"].grad``; ``debug_dict`` also receives ``is_hypothesis_positive`` and
    ``views_permutation`` (the candidate ids).  With ``cfg.predict_pose_update = False`` there is no pose loss and no
    ``loss_TCO*`` meter; with both flags both groups are filled."""
    if make_visualization:
        raise NotImplementedError("megapose_forward_loss: the bokeh visualisation is not built")
    if cfg.random_ambient_light:
        raise NotImplementedError("megapose_forward_loss: random_ambient_light is not built (set cfg.random_ambient_light = False)")
    method = cfg.hypotheses_init_method
    if method not in MEGAPOSE_METHODS and not method.startswith("coarse_classif_multiview"):
        raise ValueError(method)
    logits_loss = bool(cfg.predict_rendered_views_logits)
    if logits_loss:
        if method != "coarse_classif_multiview_paper":
            raise ValueError(f"megapose_forward_loss: the rendered-views-logits loss needs the labels of "
                             f"coarse_classif_multiview_paper, not {method!r}")
        assert cfg.n_rendered_views == 1 and n_iterations == 1  # as the reference asserts
    bt = _batch(data, "megapose_forward_loss")
    images = _images(bt, bool(getattr(model, "input_depth", False)))
    B, n_hyp = bt["B"], int(cfg.n_hypotheses)
    hyp, is_positive, view_ids = make_hypotheses(method, bt, mesh_db, cfg, seed, store=getattr(model, "store", None), return_labels=True)
    outputs = _run_model(model, images, bt["K"], bt["labels"], hyp, n_iterations, random_ambient_light=False)

    points, TCO_possible_gt = _loss_tables(mesh_db, bt["labels"], bt["TCO"], int(cfg.n_points_loss), _seed(seed, 0))
    TCO_possible_gt = TCO_possible_gt.repeat_interleave(n_hyp, dim=0)
    points = points.repeat_interleave(n_hyp, dim=0)

    keyed, list_losses_pose, time_render = [], [], 0.0
    for n in range(n_iterations):
        it = outputs[f"iteration={n + 1}"]
        if cfg.predict_pose_update:
            pose = it.network_outputs["pose"].requires_grad_()
            loss_TCO_iter, loss_data = losses.loss_refiner_CO_disentangled_reference_point(
                TCO_possible_gt=TCO_possible_gt, TCO_input=it.TCO_input, refiner_outputs=pose, K_crop=it.K_crop, points=points, tCR=it.tCR)
            loss_TCO_iter = loss_TCO_iter.view(B, n_hyp)
            keyed.append((f"loss_TCO-iter={n + 1}", loss_TCO_iter.mean()))
            list_losses_pose.append(loss_TCO_iter)
            for key, val in loss_data.items():
                if key != "loss":
                    keyed.append((f"loss_TCO-iter={n + 1}-{key}", val.view(B, n_hyp).mean()))
        time_render += it.timing_dict["render"]

    loss_hypotheses = torch.zeros((B, n_hyp, n_iterations), device=bt["device"], dtype=torch.float32)
    if cfg.predict_pose_update:
        losses_pose = torch.stack(list_losses_pose).permute(1, 2, 0)
        loss_hypotheses = loss_hypotheses + cfg.loss_alpha_pose * losses_pose
        keyed.append(("loss_TCO", losses_pose.mean(dim=(-1, -2)).mean()))
    if logits_loss:
        logits = outputs["iteration=1"].network_outputs["renderings_logits"].requires_grad_()
        assert logits.shape == (B * n_hyp, 1), "megapose_forward_loss: the model has no rendered-views-logits head of one view"
        loss_renderings_confidence = losses.renderings_confidence_loss(logits.view(B, n_hyp), is_positive,
                                                                       cfg.renderings_logits_temperature)
        keyed.append(("loss_renderings_confidence", loss_renderings_confidence.mean()))
        loss_hypotheses = loss_hypotheses + cfg.loss_alpha_renderings_confidence * loss_renderings_confidence[..., None]
    loss = loss_hypotheses.mean()
    keyed.append(("loss_total", loss))

    # the reference's order: the iterations' meters, time_render, loss_TCO, loss_renderings_confidence, loss_total
    n_iter_keys = len(keyed) - 1 - int(bool(cfg.predict_pose_update)) - int(logits_loss)
    values = torch.stack([v.detach().reshape(()) for _, v in keyed]).tolist()  # the step's one read-back
    for (key, _), v in list(zip(keyed, values))[:n_iter_keys]:
        meters[key].add(v)
    meters["time_render"].add(time_render)
    for (key, _), v in list(zip(keyed, values))[n_iter_keys:]:
        meters[key].add(v)
    if debug_dict is not None:
        debug_dict.update(outputs=outputs, time_render=time_render, hypotheses_TCO_init=hyp, points=points, TCO_possible_gt=TCO_possible_gt)
        if logits_loss:
            debug_dict.update(is_hypothesis_positive=is_positive, views_permutation=view_ids)
    return loss


# ---- Mask R-CNN -------------------------------------------------------------------------------------------------------------------
RPN_TRAIN_TOP_N = (2000, 2000)  # torchvision MaskRCNN: rpn_pre_nms_top_n_train, rpn_post_nms_top_n_train
MASK_SIZE = 28


def _grid_anchors(model, maps) -> torch.Tensor:
    """``AnchorGenerator`` for one image of the network's canvas: ``[A, 4]`` in torchvision's ``(level, y, x, a)`` order."""
    dev, out = model.device, []
    for l in range(5):
        gh, gw = maps[5 + l].shape[1:3]
        sy = torch.arange(gh, dtype=torch.int32, device=dev) * (model.padded[0] // gh)
        sx = torch.arange(gw, dtype=torch.int32, device=dev) * (model.padded[1] // gw)
        y, x = torch.meshgrid(sy, sx, indexing="ij")
        shifts = torch.stack([x, y, x, y], -1).reshape(-1, 1, 4).float()
        out.append((shifts + torch.as_tensor(model._base[l], device=dev).reshape(1, -1, 4)).reshape(-1, 4))
    return torch.cat(out)


def h_maskrcnn(data, model, meters, cfg, *, seed: int = 0, debug_dict: Optional[Dict[str, Any]] = None) -> torch.Tensor:
    """One forward-loss step of the detector trainer (``CP/training/maskrcnn_forward_loss.py``): the train-mode forward of
    ``detector.MaskRCNN`` -- torchvision 0.14's ``MaskRCNN.forward`` with targets, restated from its published definitions
    (parity with torchvision is unpinned: ``happypose_amd.detection_losses``).  ``data = (images, targets)``: uint8 images
    ``[H, W, 3]`` on the device, one dict ``boxes [g, 4]``, ``labels [g]``, ``masks [g, H, W]`` per image.  Fills
    ``loss_rpn_box_reg``, ``loss_objectness``, ``loss_box_reg``, ``loss_classifier`` and ``loss_mask`` with one read-back and
    returns their weighted sum as a device scalar.

    This is the step, not a trainer: the objectness maps, the delta maps, ``class_logits``, ``box_regression`` and
    ``mask_logits`` are marked ``requires_grad_()`` and left in ``debug_dict`` (not in the reference); after ``loss.backward()``
    their ``.grad`` is the hand-over point.  No network backward, no optimiser.  The sampler draws from ``seed``; the images must
    have the network's own size (targets are not resized)."""
    images, targets = data
    dev = model.device
    images = torch.stack(list(images)) if not isinstance(images, torch.Tensor) else images
    ops._on_device("h_maskrcnn", images=images)
    assert images.dim() == 4 and images.shape[-1] == 3 and images.dtype == torch.uint8, "h_maskrcnn: images uint8 [H, W, 3]"
    B, H, W = images.shape[:3]
    if (H, W) != tuple(model.orig_size) or tuple(model.size) != tuple(model.orig_size):
        raise NotImplementedError(f"h_maskrcnn: images of {H} x {W} on a network that resizes {model.orig_size} to {model.size}: "
                                  "targets are not resized")
    assert len(targets) == B, "h_maskrcnn: one target per image"
    for t in targets:
        ops._on_device("h_maskrcnn", boxes=t["boxes"], labels=t["labels"], masks=t["masks"])
        g = t["boxes"].shape[0]
        assert t["labels"].shape == (g,) and t["masks"].shape == (g, H, W), "h_maskrcnn: boxes [g, 4], labels [g], masks [g, H, W]"
    x = (images.permute(0, 3, 1, 2).float() / 255).contiguous()

    # 1. the backbone, FPN and RPN head
    mb = model.backbone.max_batch
    chunks = [model.backbone.forward_nhwc(x[s:s + mb]) for s in range(0, B, mb)]
    maps = [torch.cat([c[i] for c in chunks]) for i in range(15)]
    objectness_maps = [m.requires_grad_() for m in maps[5:10]]   # [B, h, w, 4]: anchors 0 .. 2, one padding channel
    delta_maps = [m.requires_grad_() for m in maps[10:15]]       # [B, h, w, 12] = (anchor, 4)
    maps_d = [m.detach() for m in maps]

    # 2. the RPN losses on all anchors
    objectness = torch.cat([m[..., :3].reshape(B, -1) for m in objectness_maps], 1).reshape(-1)
    pred_deltas = torch.cat([m.reshape(B, -1, 4) for m in delta_maps], 1).reshape(-1, 4)
    anchors = _grid_anchors(model, maps)
    rpn_labels, rpn_gt_boxes, rpn_matches = detection_losses.rpn_assign_targets_to_anchors([anchors] * B, targets, return_matches=True)
    rpn_targets = [detection_losses.box_encode(g, anchors, (1.0, 1.0, 1.0, 1.0)) for g in rpn_gt_boxes]
    seeds = dict(rpn=_seed(seed, 2), box=_seed(seed, 3))
    loss_objectness, loss_rpn_box_reg, rpn_sampled = detection_losses.rpn_compute_loss(
        objectness, pred_deltas, rpn_labels, rpn_targets, seed=seeds["rpn"], return_sampled=True)

    # 3. - 5. proposals with the training top-n, the ground truths appended, matched, sampled and encoded
    with torch.no_grad():
        rpn_proposals = [model._proposals(maps_d, b, *RPN_TRAIN_TOP_N)[0] for b in range(B)]
    proposals, matched_idxs, labels, regression_targets = detection_losses.roi_select_training_samples(rpn_proposals, targets, seed=seeds["box"])

    # 6. the box head
    def rois_of(boxes):
        return torch.cat([torch.cat([torch.full((p.shape[0], 1), float(b), device=dev), p], 1) for b, p in enumerate(boxes)])

    C_, c4 = model.num_classes, model._c4
    with torch.no_grad():
        rois = rois_of(proposals)
        n = rois.shape[0]
        pooled = model._roi_align(maps_d, rois, 7)
        cls, reg = model.box_net.run(pooled) if n else (torch.zeros((0, c4), device=dev), torch.zeros((0, 4 * C_), device=dev))
    class_logits = cls.reshape(n, -1).clone().requires_grad_()       # [n, c4]: the classes, then padding columns
    box_regression = reg.reshape(n, -1).clone().requires_grad_()
    loss_classifier, loss_box_reg = detection_losses.fastrcnn_loss(class_logits, box_regression, labels, regression_targets, num_classes=C_)

    # 7. the mask head on the positive samples
    pos = [torch.where(l > 0)[0] for l in labels]
    mask_proposals = [p[i] for p, i in zip(proposals, pos)]
    pos_matched_idxs = [m[i] for m, i in zip(matched_idxs, pos)]
    with torch.no_grad():
        mrois = rois_of(mask_proposals)
        nm = mrois.shape[0]
        if nm:
            ml = model.mask_net.run(model._roi_align(maps_d, mrois, 14))[0]      # [nm, 14, 56, c4] = (i, (j, a, b), class)
            ml = ml.reshape(nm, 14, 14, 2, 2, -1).permute(0, 5, 1, 3, 2, 4).reshape(nm, -1, MASK_SIZE, MASK_SIZE)[:, :C_]
        else:
            ml = torch.zeros((0, C_, MASK_SIZE, MASK_SIZE), device=dev)
    mask_logits = ml.contiguous().clone().requires_grad_()
    loss_mask, mask_labels, mask_targets = detection_losses.maskrcnn_loss(
        mask_logits, mask_proposals, [t["masks"] for t in targets], [t["labels"] for t in targets], pos_matched_idxs, return_targets=True)

    loss = (cfg.rpn_box_reg_alpha * loss_rpn_box_reg + cfg.objectness_alpha * loss_objectness + cfg.box_reg_alpha * loss_box_reg
            + cfg.classifier_alpha * loss_classifier + cfg.mask_alpha * loss_mask)
    _read_back(meters, [("loss_rpn_box_reg", loss_rpn_box_reg), ("loss_objectness", loss_objectness), ("loss_box_reg", loss_box_reg),
                        ("loss_classifier", loss_classifier), ("loss_mask", loss_mask)])
    if debug_dict is not None:
        debug_dict.update(objectness_maps=objectness_maps, delta_maps=delta_maps, class_logits=class_logits, box_regression=box_regression,
                          mask_logits=mask_logits, anchors=anchors, rpn_labels=rpn_labels, rpn_matched_idxs=rpn_matches,
                          rpn_regression_targets=rpn_targets, rpn_sampled=rpn_sampled, rpn_proposals=rpn_proposals, proposals=proposals,
                          matched_idxs=matched_idxs, labels=labels, regression_targets=regression_targets, mask_proposals=mask_proposals,
                          mask_matched_idxs=pos_matched_idxs, mask_labels=mask_labels, mask_targets=mask_targets, seeds=seeds,
                          losses=dict(loss_rpn_box_reg=loss_rpn_box_reg, loss_objectness=loss_objectness, loss_box_reg=loss_box_reg,
                                      loss_classifier=loss_classifier, loss_mask=loss_mask))
    return loss


# ---- training the linear heads on a frozen backbone ------------------------------------------------------------------------------
@dataclass
class HeadOptimConfig:
    """The optimiser recipe of the reference's trainers.  Both construct ``torch.optim.Adam(lr=3e-4, weight_decay=0.0)`` -- L2,
    not decoupled -- with torch's default ``betas`` and ``eps`` (``CP/training/train_pose.py:374-378``,
    ``MP/training/utils.py:115-135`` with ``MP/training/training_config.py:113-118``), clip the total gradient norm
    (``clip_grad_norm``: 1000.0 in ``training_config.py:115``, the default here; 0.5 in ``CP/scripts/run_pose_training.py:70``:
    :meth:`cosypose`) and warm the learning rate up linearly over ``n_epochs_warmup = 50`` epochs of
    ``epoch_size // batch_size = 115200 // 16`` batches with a ``LambdaLR``: step ``t = 1, 2, ...`` runs at
    ``lr min(t / n_warmup_steps, 1)`` (``train_pose.py:387-392``, ``(batch + 1) / n_batches_warmup``; MegaPose's
    ``max(batch, 1) / n_batches_warmup`` repeats the first value once).  ``n_warmup_steps = 0``: no warm-up.  The decay by 10
    every ``lr_epoch_decay`` epochs belongs to a loop over a dataset and is not here.  ``clip_grad_norm = None``: no clipping."""

    lr: float = 3e-4
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    weight_decay: float = 0.0
    decoupled: bool = False
    clip_grad_norm: Optional[float] = 1000.0
    n_warmup_steps: int = 50 * (115200 // 16)

    @classmethod
    def cosypose(cls, **kw) -> "HeadOptimConfig":
        return cls(**{"clip_grad_norm": 0.5, **kw})

    def lr_at(self, step: int) -> float:
        """The learning rate of step ``step`` (counted from 1)."""
        if self.n_warmup_steps <= 0:
            return float(self.lr)
        return float(self.lr) * min(step / self.n_warmup_steps, 1.0)


class _WithFeatures:
    """A predictor whose calls ask for the head input features; everything else is the predictor's."""

    def __init__(self, model):
        self._model = model

    def __getattr__(self, name):
        return getattr(self._model, name)

    def __call__(self, **kw):
        return self._model(return_features=True, **kw)


class HeadTrainer:
    """Fine-tunes the linear heads of a pose network on its frozen backbone: the pose rows, the rendered-view logits rows (their
    gradient is ``renderings_logits.grad`` where the rendered-views-logits loss ran, zero otherwise) and, on the
    torchvision-ResNet path, the 512 x 512 ``fc`` in front of them.  A network with a logits head and no pose head (the coarse
    classifier, ``pose_dim == 0``) is trained on its logits rows alone.

    fp32 master copies of these tensors live in one flat device buffer ``p`` beside the gradient ``g`` and Adam's ``m`` / ``v``.
    :meth:`step` is ``megapose_forward_loss`` / ``h_pose``, ``loss.backward()`` (which leaves ``dL/dpose`` at every iteration's
    network output), then ``ops.head_backward`` per iteration -- summed with ``accumulate`` --, ``ops.fc_backward``,
    ``ops.grad_sq_norm``, ``ops.adamw_step`` and ``ops.Net.set_param_device``: between ``backward()`` and the weight write
    there are only launches and device-to-device copies on one stream, no host synchronisation.  The backbone's own backward
    (and train-mode BatchNorm) is not built: ``d_feat`` of ``ops.head_backward`` is where it would attach."""

    ORDER = ("pose_fc.weight", "views_logits_head.weight", "pose_fc.bias", "views_logits_head.bias", "backbone.fc.weight", "backbone.fc.bias")

    def __init__(self, model, mesh_db, cfg, optim_cfg: Optional[HeadOptimConfig] = None, kind: str = "megapose"):
        if kind not in ("megapose", "cosypose"):
            raise ValueError(kind)
        net = getattr(model, "backbone", None)
        if not isinstance(net, ops.Net):
            raise TypeError("HeadTrainer: the model must be a single-lane predictor of this library (model.backbone an ops.Net)")
        if not net.pose_dim and not net.n_logits:
            raise ValueError("HeadTrainer: the network has neither a pose head nor a logits head")
        if optim_cfg is None:
            optim_cfg = HeadOptimConfig() if kind == "megapose" else HeadOptimConfig.cosypose()
        self.model, self.mesh_db, self.cfg, self.optim_cfg, self.kind = model, mesh_db, cfg, optim_cfg, kind
        self.net, self.device = net, net.device
        self.pose_dim, self.n_logits, self.n_features = int(net.pose_dim), int(net.n_logits), int(net.n_features)
        shapes = net.head_param_shapes()
        self.has_fc = "backbone.fc.weight" in shapes
        self.shapes = {k: shapes[k] for k in self.ORDER if k in shapes}
        n = sum(int(np.prod(sh)) for sh in self.shapes.values())
        f = dict(dtype=torch.float32, device=self.device)
        self.p, self.g = torch.empty(n, **f), torch.zeros(n, **f)
        self.m, self.v = torch.zeros(n, **f), torch.zeros(n, **f)
        self.n_steps = 0
        self.params, self.grads = self._views(self.p), self._views(self.g)
        for name, view in self.params.items():
            net.get_param_device(name, out=view)
        # the heads as ONE matrix [O, C] and one bias [O]: ORDER puts the pose rows and the logits rows next to each other
        O, C = self.pose_dim + self.n_logits, self.n_features
        self._W, self._gW, self._gb = self.p[:O * C].view(O, C), self.g[:O * C].view(O, C), self.g[O * C:O * C + O]
        self._sq_norm = torch.zeros(1, **f)
        clip = optim_cfg.clip_grad_norm
        self._max_norm = None if clip is None else torch.full((1,), float(clip), **f)

    def _views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        out, at = {}, 0
        for name, shape in self.shapes.items():
            k = int(np.prod(shape))
            out[name] = flat[at:at + k].view(shape)
            at += k
        return out

    def _forward_loss(self, batch, meters, n_iterations: int, seed: int, debug_dict, **kw) -> torch.Tensor:
        model = _WithFeatures(self.model)
        if self.kind == "megapose":
            return megapose_forward_loss(model, self.cfg, batch, meters, self.mesh_db, n_iterations, debug_dict, seed=seed, **kw)
        if not self.cfg.loss_disentangled:
            raise NotImplementedError("HeadTrainer: the ADD-L1 loss leaves its gradient at TCO_output; the backward of the pose "
                                      "update is not built (cfg.loss_disentangled = True)")
        return h_pose(model, self.mesh_db, batch, meters, self.cfg, n_iterations, seed=seed, debug_dict=debug_dict, **kw)

    def step(self, batch, meters, n_iterations: int = 1, seed: int = 0, *, debug_dict: Optional[Dict[str, Any]] = None, **kw) -> torch.Tensor:
        """One optimiser step on ``batch``; returns ``loss_total`` of the forward (a device scalar, before the update) and adds
        ``grad_norm`` (the total norm before clipping, as ``clip_grad_norm_`` returns it) and ``lr`` to ``meters`` beside the
        forward-loss function's own.  ``debug_dict`` receives what the forward-loss function leaves there; ``kw`` goes to it
        (``input_generator=`` for ``h_pose``)."""
        dbg: Dict[str, Any] = {} if debug_dict is None else debug_dict
        loss = self._forward_loss(batch, meters, n_iterations, seed, dbg, **kw)
        loss.backward()
        # from here to the weight write: launches and device-to-device copies on the current stream only
        for k in range(n_iterations):
            out = dbg["outputs"][f"iteration={k + 1}"].network_outputs
            d_pose = out["pose"].grad if "pose" in out else None
            d_logits = out["renderings_logits"].grad if "renderings_logits" in out else None
            assert d_pose is not None or d_logits is not None, "the loss reached none of this iteration's network outputs"
            assert d_pose is not None or not self.pose_dim or not getattr(self.cfg, "predict_pose_update", True), \
                "the loss did not reach this iteration's pose output"
            if d_pose is None and self.pose_dim:  # a pose head that no loss reads (cfg.predict_pose_update = False)
                d_pose = torch.zeros((out["features"].shape[0], self.pose_dim), dtype=torch.float32, device=self.device)
            res = ops.head_backward(out["features"], None if d_pose is None else d_pose.contiguous(), self._W,
                                    d_logits=None if d_logits is None else d_logits.contiguous(), n_logits=self.n_logits,
                                    dW=self._gW, db=self._gb, accumulate=k > 0, return_d_feat=self.has_fc)
            if self.has_fc:
                ops.fc_backward(res[2], out["pooled"], dW=self.grads["backbone.fc.weight"], db=self.grads["backbone.fc.bias"],
                                accumulate=k > 0)
        ops.grad_sq_norm(self.g, out=self._sq_norm)
        self.n_steps += 1
        oc = self.optim_cfg
        lr = oc.lr_at(self.n_steps)
        ops.adamw_step(self.p, self.g, self.m, self.v, lr=lr, betas=oc.betas, eps=oc.eps, weight_decay=oc.weight_decay, step=self.n_steps,
                       decoupled=oc.decoupled, sq_norm=self._sq_norm if self._max_norm is not None else None, max_norm=self._max_norm)
        self._write_heads()
        meters["grad_norm"].add(math.sqrt(float(self._sq_norm)))  # the step's second read-back, after the weights are written
        meters["lr"].add(lr)
        return loss.detach()

    def _write_heads(self) -> None:
        for name, view in self.params.items():
            self.net.set_param_device(name, view)

    def state_dict(self) -> Dict[str, Any]:
        """The head tensors under the reference's parameter names (update a checkpoint's ``state_dict`` with them and the model
        loaders read the fine-tuned network) and the optimiser state under ``"optimizer"``: ``step`` and, per parameter name,
        ``exp_avg`` / ``exp_avg_sq``.  Everything is a copy."""
        m, v = self._views(self.m), self._views(self.v)
        out: Dict[str, Any] = {name: t.clone() for name, t in self.params.items()}
        out["optimizer"] = dict(step=self.n_steps, exp_avg={k: t.clone() for k, t in m.items()},
                                exp_avg_sq={k: t.clone() for k, t in v.items()})
        return out

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        """The inverse of :meth:`state_dict`; the heads go into the network too.  Without ``"optimizer"`` the moments restart."""
        missing = [k for k in self.shapes if k not in state]
        if missing:
            raise KeyError(f"HeadTrainer.load_state_dict: missing {missing}")
        m, v = self._views(self.m), self._views(self.v)
        for name, view in self.params.items():
            src = torch.as_tensor(state[name])
            assert tuple(src.shape) == tuple(view.shape), f"{name}: {tuple(src.shape)} for {tuple(view.shape)}"
            view.copy_(src)
        opt = state.get("optimizer")
        if opt is None:
            self.m.zero_(), self.v.zero_()
            self.n_steps = 0
        else:
            self.n_steps = int(opt["step"])
            for name in self.shapes:
                m[name].copy_(torch.as_tensor(opt["exp_avg"][name]))
                v[name].copy_(torch.as_tensor(opt["exp_avg_sq"][name]))
        self._write_heads()
