"""Pose-error metrics and the pose-error meter of the evaluation, on the device.

Drop-in for ``TB/lib3d/distances.py`` (``dists_add``, ``dists_add_symmetric``, ``dists_add_symmetries``),
``CP/lib3d/symmetric_distances.py::chamfer_dist`` and ``CP/evaluation/meters/pose_meters.py::PoseErrorMeter`` with the helpers of
``CP/evaluation/meters/utils.py``; ``mssd`` / ``mspd`` are BOP's two further pose errors, which the reference leaves to
``bop_toolkit``.  All errors come from ONE kernel family (``ops.pose_errors``, ``csrc/pose_errors.hip``): the nearest-neighbour
search of ADD-S is tiled, so nothing of size ``P x P`` is ever allocated and a whole evaluation batch is one launch.

Differences from the reference, all on the host side:
  * no xarray: ``PoseErrorMeter.summary()`` returns ``gt`` / ``matches`` / ``preds`` / ``ap`` as pandas DataFrames with the
    reference's variable names as columns; the array-valued variables (``xyz``, ``TCO_xyz``, ``TXO_pred``) are object columns
    holding one numpy array per row, and the per-object AUC table is ``gt.attrs["AUC/objects"]``;
  * no scikit-learn: the average precision is :func:`average_precision`;
  * ``errors_bsz`` is accepted and ignored: it bounded the reference's ``[b, P, P, 3]`` temporary, and there is none to bound --
    ``exact_meshes=True`` therefore no longer needs ``errors_bsz == 1``.
"""

from __future__ import annotations

from collections import OrderedDict, defaultdict
from typing import Dict, Optional, Sequence

import numpy as np
import pandas as pd
import torch

from . import ops
from .tensor_collection import PandasTensorCollection

GROUP_KEYS = ("scene_id", "view_id", "label")
ERROR_TYPES = ("ADD", "ADD-S", "ADD(-S)", "ADD-SYM", "MSSD", "MSPD")
_MAX_ERRORS = ("MSSD", "MSPD")  # the metric is the largest per-point distance, not the mean


# ---- distances on explicit point sets (TB/lib3d/distances.py) --------------------------------------------------------------------
def _transform_pts(T: torch.Tensor, pts: torch.Tensor) -> torch.Tensor:
    out = pts @ T[..., :3, :3].transpose(-1, -2)
    out += T[..., None, :3, 3]
    return out


def _rows_on_points(mode: str, TXO_pred, TXO_gt, points, symmetries=None, **kw):
    """One row per batch entry, each with its own point set (and symmetry set): the tables have one 'object' per row."""
    b, n_pts = points.shape[0], points.shape[1]
    dev = points.device
    if symmetries is None:
        symmetries = torch.eye(4, dtype=torch.float32, device=dev).expand(b, 1, 4, 4)
    ids = torch.arange(b, dtype=torch.int32)
    return ops.pose_errors_tables(ids, ids, ids, np.full(b, ops.POSE_ERR_MODES[mode], np.int32), TXO_pred, TXO_gt, points, symmetries,
                                  torch.full((b,), symmetries.shape[1], dtype=torch.int32, device=dev),
                                  torch.full((b,), n_pts, dtype=torch.int32, device=dev), **kw)


def dists_add(TXO_pred: torch.Tensor, TXO_gt: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """``T_gt p - T_pred p`` for every point: ``[b, P, 3]``."""
    return _transform_pts(TXO_gt, points) - _transform_pts(TXO_pred, points)


def dists_add_symmetric(TXO_pred: torch.Tensor, TXO_gt: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """For every ground-truth point the difference to its nearest predicted point: ``[b, P, 3]``.  The neighbours come from the
    tiled kernel (``assign``); the only temporaries are ``[b, P]`` and ``[b, P, 3]``."""
    if points.shape[0] == 0:
        return points.new_zeros(points.shape)
    assign = _rows_on_points("ADD-S", TXO_pred, TXO_gt, points, return_assign=True)["assign"].long()
    picked = torch.gather(_transform_pts(TXO_pred, points), 1, assign.unsqueeze(-1).expand(-1, -1, 3))
    dists = _transform_pts(TXO_gt, points)
    dists -= picked
    return dists


def dists_add_symmetries(TXO_pred: torch.Tensor, TXO_gt_possible: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """``TXO_gt_possible [b, S, 4, 4]``: the ground truth under each symmetry.  Differences for the one with the smallest mean
    norm: ``[b, P, 3]``."""
    b = TXO_pred.shape[0]
    if b == 0:
        return points.new_zeros(points.shape)
    eye = torch.eye(4, dtype=torch.float32, device=points.device).expand(b, 4, 4)
    sym_id = _rows_on_points("ADD-SYM", TXO_pred, eye, points, symmetries=TXO_gt_possible)["sym_id"].long()
    TXO_gt = TXO_gt_possible[torch.arange(b, device=sym_id.device), sym_id]
    return _transform_pts(TXO_gt, points) - _transform_pts(TXO_pred, points)


# ---- distances on a mesh database ------------------------------------------------------------------------------------------------
def _rows_on_meshes(mode: str, T_pred, T_gt, labels, mesh_db, K=None, exact_meshes=False):
    ids = torch.arange(len(labels), dtype=torch.int32)
    return ops.pose_errors(ids, ids, mesh_db.ids_of(labels), np.full(len(labels), ops.POSE_ERR_MODES[mode], np.int32), T_pred, T_gt,
                           mesh_db, K=K, exact_meshes=exact_meshes)


def chamfer_dist(T1: torch.Tensor, T2: torch.Tensor, labels, mesh_db):
    """``(dists [b], None)``: mean distance from every point of the object under ``T1`` to the nearest point under ``T2``, over
    the padded point table like the reference."""
    bsz = T1.shape[0]
    assert T1.shape == (bsz, 4, 4) and T2.shape == (bsz, 4, 4) and len(labels) == bsz
    if bsz == 0:
        return torch.empty(0, dtype=T1.dtype, device=T1.device), None
    return _rows_on_meshes("ADD-S", T2, T1, labels, mesh_db)["norm_avg"], None


def mssd(TXO_pred: torch.Tensor, TXO_gt: torch.Tensor, labels, mesh_db, exact_meshes: bool = True) -> torch.Tensor:
    """Maximum symmetry-aware surface distance (BOP): ``min_S max_j |T_pred p_j - T_gt S p_j|``, ``[b]`` metres."""
    return _rows_on_meshes("MSSD", TXO_pred, TXO_gt, labels, mesh_db, exact_meshes=exact_meshes)["norm_max"]


def mspd(TXO_pred: torch.Tensor, TXO_gt: torch.Tensor, K: torch.Tensor, labels, mesh_db, exact_meshes: bool = True) -> torch.Tensor:
    """Maximum symmetry-aware projection distance (BOP): as :func:`mssd` with both sides projected by ``K [b, 3, 3]``, pixels."""
    return _rows_on_meshes("MSPD", TXO_pred, TXO_gt, labels, mesh_db, K=K, exact_meshes=exact_meshes)["norm_max"]


# ---- bookkeeping of the meter (CP/evaluation/meters/utils.py) ---------------------------------------------------------------------
def add_inst_num(infos: pd.DataFrame, group_keys=GROUP_KEYS, key: str = "pred_inst_num") -> pd.DataFrame:
    """Number the rows of every group 0, 1, ... in row order (column ``key``, added in place)."""
    infos[key] = infos.groupby(list(group_keys), sort=False).cumcount().to_numpy(dtype=int)
    return infos


def get_top_n_ids(infos: pd.DataFrame, group_keys=GROUP_KEYS, top_key: str = "score", n_top: int = -1, targets=None):
    """Row positions of the best rows of every group by descending ``top_key``: ``n_top`` of them if positive, else the group's
    ``inst_count`` in ``targets`` (0 for a group that is no target), else all.  Groups in sorted key order."""
    keys = list(group_keys)
    counts = None
    if n_top <= 0 and targets is not None:
        counts = {k: targets.loc[ids[0], "inst_count"] for k, ids in targets.groupby(keys).groups.items()}
    position = pd.Series(np.arange(len(infos)), index=infos.index)
    keep = []
    for k, ids in infos.groupby(keys).groups.items():
        ranked = infos.loc[ids].sort_values(top_key, ascending=False)
        n = n_top if n_top > 0 else (counts.get(k, 0) if counts is not None else len(ranked))
        keep.append(position.loc[ranked.index].to_numpy()[:n])
    return np.concatenate(keep) if keep else []


def add_valid_gt(gt_infos: pd.DataFrame, group_keys=GROUP_KEYS, visib_gt_min: float = -1, targets=None) -> pd.DataFrame:
    """Column ``valid``: visible enough (``visib_fract >= visib_gt_min``, and a target label) when a minimum is given; else the
    most visible ``inst_count`` instances of every target group; else everything."""
    if visib_gt_min > 0:
        valid = (gt_infos["visib_fract"] >= visib_gt_min).to_numpy()
        if targets is not None:
            valid = valid & np.isin(gt_infos["label"], targets["label"])
        gt_infos["valid"] = valid
    elif targets is not None:
        valid = np.zeros(len(gt_infos), dtype=bool)
        ids = get_top_n_ids(gt_infos, group_keys=group_keys, top_key="visib_fract", targets=targets)
        valid[np.asarray(ids, dtype=int)] = True
        gt_infos["valid"] = valid
    else:
        gt_infos["valid"] = True
    return gt_infos


def get_candidate_matches(pred_infos: pd.DataFrame, gt_infos: pd.DataFrame, group_keys=GROUP_KEYS, only_valids: bool = True):
    """Every (prediction, ground truth) pair of one group: the inner join on the group keys with ``pred_id`` / ``gt_id`` (row
    positions, added to both frames in place) and ``cand_id``."""
    pred_infos["pred_id"] = np.arange(len(pred_infos))
    gt_infos["gt_id"] = np.arange(len(gt_infos))
    cands = pred_infos.merge(gt_infos, on=list(group_keys))
    if only_valids:
        cands = cands[cands["valid"]].reset_index(drop=True)
    cands["cand_id"] = np.arange(len(cands))
    return cands


def match_poses(cand_infos: pd.DataFrame, group_keys=GROUP_KEYS) -> pd.DataFrame:
    """Greedy one-to-one matching inside every group: predictions by descending score, each takes the still-free ground truth
    with the smallest finite ``error`` (the first one on a tie)."""
    assert "error" in cand_infos
    if len(cand_infos) == 0:
        return cand_infos
    chosen = []
    for _, group in cand_infos.groupby(list(group_keys)):
        order = group.drop_duplicates("pred_id").sort_values("score", ascending=False)["pred_id"]
        taken = set()
        for pred_id in order:
            free = group[(group["pred_id"] == pred_id) & ~group["gt_id"].isin(taken) & (group["error"] < np.inf)]
            if len(free):
                best = free["error"].idxmin()
                taken.add(free.loc[best, "gt_id"])
                chosen.append(best)
    return cand_infos.loc[chosen].reset_index(drop=True)


def compute_auc_posecnn(errors) -> float:
    """Area under the accuracy-threshold curve up to 0.1 m, as the YCB-Video toolbox computes it (PoseCNN), scaled to 0..1."""
    d = np.sort(np.array(errors, dtype=float))
    accuracy = np.cumsum(np.ones(len(d))) / max(len(d), 1)
    inside = np.isfinite(d) & ~(d > 0.1)
    if not inside.any():
        return np.nan
    d, accuracy = d[inside], accuracy[inside]
    mrec = np.concatenate(([0], d, [0.1]))
    mpre = np.maximum.accumulate(np.concatenate(([0], accuracy, [accuracy[-1]])))
    steps = np.where(mrec[1:] != mrec[:-1])[0] + 1
    return ((mrec[steps] - mrec[steps - 1]) * mpre[steps]).sum() * 10


def average_precision(y_true, y_score) -> float:
    """``sum_n (R_n - R_{n-1}) P_n`` over the distinct score thresholds in descending order -- what
    ``sklearn.metrics.average_precision_score`` computes for binary labels.  0 without a positive."""
    y_true, y_score = np.asarray(y_true, dtype=float), np.asarray(y_score, dtype=float)
    if y_true.sum() == 0:
        return 0.0
    order = np.argsort(-y_score, kind="mergesort")
    y_true, y_score = y_true[order], y_score[order]
    last_of_threshold = np.r_[np.where(np.diff(y_score))[0], len(y_score) - 1]
    tps = np.cumsum(y_true)[last_of_threshold]
    precision = tps / (last_of_threshold + 1)
    recall = tps / tps[-1]
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


# ---- the meter -------------------------------------------------------------------------------------------------------------------
_FILL = {"norm": np.inf, "0.1d": False, "xyz": np.inf, "TCO_xyz": np.inf, "TCO_norm": np.inf, "obj_diameter": np.nan,
         "TXO_pred": np.nan, "score": np.nan, "iou": np.nan, "iou_valid": False}
_ARRAY_COLUMNS = {"xyz": (3,), "TCO_xyz": (3,), "TXO_pred": (4, 4)}


def _left_join(left: pd.DataFrame, right: pd.DataFrame, on: Sequence[str]) -> pd.DataFrame:
    """The reference's ``xr_merge``: every column of ``right`` that is not a key is added to a copy of ``left``, taken from the
    row of ``right`` with equal keys and filled per ``_FILL`` (NaN otherwise) where there is none.  One row per left row."""
    on = list(on)
    idx = left[on].merge(right[on].assign(_row=np.arange(len(right))), on=on, how="left")
    assert len(idx) == len(left), "join keys are not unique"
    src = idx["_row"].to_numpy(dtype=float)
    have = np.isfinite(src)
    src = src[have].astype(int)
    out = left.copy()
    for col in right.columns:
        if col in on:
            continue
        fill = _FILL.get(col, np.nan)
        if col in _ARRAY_COLUMNS:
            values = _array_column([np.full(_ARRAY_COLUMNS[col], fill) for _ in range(len(left))])
            taken = right[col].to_numpy()
            for i, j in zip(np.where(have)[0], src):
                values[i] = taken[j]
        else:
            values = np.full(len(left), fill, dtype=np.array(fill).dtype)
            values[have] = right[col].to_numpy()[src]
        out[col] = values
    return out


def _array_column(a) -> np.ndarray:
    """Object column with one array per row (numpy would otherwise stack equal shapes into one array)."""
    col = np.empty(len(a), dtype=object)
    for i, v in enumerate(a):
        col[i] = v
    return col


class PoseErrorMeter:
    """The reference's meter with its constructor arguments.  ``error_type``: ``ADD``, ``ADD-S``, ``ADD(-S)`` (ADD-S for the
    labels whose ``infos[label]["is_symmetric"]`` is true, ADD for the rest -- one launch), and beyond the reference ``ADD-SYM``,
    ``MSSD`` and ``MSPD``.  MSPD reads ``gt_data.K [n, 3, 3]`` and, being in pixels, compares the error with ``match_threshold``
    and the ``0.1d`` flag with ``match_threshold`` itself instead of a fraction of the diameter.

    ``mesh_db``: a ``MeshDataBase`` (batched here) or its ``batched()`` tables.  ``errors_bsz`` is kept for compatibility and
    does not bound memory any more: every candidate of an :meth:`add` call is scored in one ``ops.pose_errors`` launch."""

    def __init__(self, mesh_db, error_type="ADD", report_AP=False, report_error_AUC=False, report_error_stats=False,
                 sample_n_points=None, errors_bsz=1, match_threshold=0.1, exact_meshes=True, spheres_overlap_check=True,
                 consider_all_predictions=False, targets=None, visib_gt_min=-1, n_top=-1, device="cuda"):
        self.sample_n_points = sample_n_points
        self.mesh_db = (mesh_db.batched() if hasattr(mesh_db, "batched") else mesh_db).to(device).float()
        self.device = device
        self.error_type = error_type.upper()
        if self.error_type not in ERROR_TYPES:
            raise ValueError("Error not supported", self.error_type)
        self.errors_bsz = errors_bsz
        self.n_top = n_top
        self.exact_meshes = exact_meshes
        self.visib_gt_min = visib_gt_min
        self.targets = targets
        self.match_threshold = match_threshold
        self.spheres_overlap_check = spheres_overlap_check
        self.consider_all_predictions = consider_all_predictions
        self.report_AP = report_AP
        self.report_error_stats = report_error_stats
        self.report_error_AUC = report_error_AUC
        self.reset()
        if self.exact_meshes:
            assert sample_n_points is None

    def reset(self):
        self.datas = defaultdict(list)

    # -- errors --------------------------------------------------------------------------------------------------------------------
    def _row_modes(self, labels) -> np.ndarray:
        if self.error_type == "ADD(-S)":
            names = ["ADD-S" if self.mesh_db.infos[label]["is_symmetric"] else "ADD" for label in labels]
        else:
            names = [self.error_type] * len(labels)
        return np.asarray([ops.POSE_ERR_MODES[m] for m in names], dtype=np.int32)

    def _device_errors(self, modes, TXO_pred, TXO_gt, labels, K) -> Dict[str, torch.Tensor]:
        """The one device call of the meter: rows (pred n, gt n, object of label n)."""
        ids = torch.arange(len(labels), dtype=torch.int32)
        obj_ids = self.mesh_db.ids_of(labels)
        if self.sample_n_points is not None:  # non-exact only: the reference's deterministic subset of the padded table
            t = self.mesh_db.device_tables
            pick = torch.as_tensor(ops.sample_point_ids(t["points"].shape[1], self.sample_n_points)).to(t["points"].device)
            points = t["points"][:, pick].contiguous()
            n_pts = torch.full((points.shape[0],), points.shape[1], dtype=torch.int32, device=points.device)
            return ops.pose_errors_tables(ids, ids, obj_ids, modes, TXO_pred, TXO_gt, points, t["symmetries"], t["n_sym"], n_pts, K=K)
        return ops.pose_errors(ids, ids, obj_ids, modes, TXO_pred, TXO_gt, self.mesh_db, K=K, exact_meshes=self.exact_meshes)

    def compute_errors(self, TXO_pred, TXO_gt, labels, K=None):
        """``norm_avg [b]``, ``xyz_avg [b, 3]``, ``TCO_xyz [b, 3]``, ``TCO_norm [b]`` as in the reference, plus ``norm_max [b]`` and
        ``sym_id [b]``; any batch size, exact meshes included."""
        if len(labels) == 0:
            return {"norm_avg": torch.empty(0, dtype=torch.float), "xyz_avg": torch.empty(0, 3, dtype=torch.float),
                    "norm_max": torch.empty(0, dtype=torch.float), "sym_id": torch.empty(0, dtype=torch.int32),
                    "TCO_xyz": torch.empty((0, 3), dtype=torch.float), "TCO_norm": torch.empty(0, dtype=torch.float)}
        if self.error_type == "MSPD" and K is None:
            raise ValueError("MSPD needs the camera intrinsics K [b, 3, 3]")
        return self._device_errors(self._row_modes(labels), TXO_pred, TXO_gt, np.asarray(labels), K if self.error_type == "MSPD" else None)

    def compute_errors_batch(self, TXO_pred, TXO_gt, labels, K=None):
        """The reference cut the candidates into batches of ``errors_bsz``; one launch scores them all."""
        return self.compute_errors(TXO_pred, TXO_gt, labels, K=K)

    # -- accumulation --------------------------------------------------------------------------------------------------------------
    def add(self, pred_data, gt_data):
        keys = list(GROUP_KEYS)
        pred_data, gt_data = pred_data.float(), gt_data.float()
        diameter = lambda labels: np.asarray([self.mesh_db.infos[k]["diameter_m"] for k in labels], dtype=float)  # noqa: E731

        # predictions of the scenes and views the ground truth covers
        gt_views = gt_data.infos.loc[:, ["scene_id", "view_id"]].drop_duplicates().reset_index(drop=True)
        targets = self.targets
        if targets is not None:
            targets = gt_views.merge(targets)
        pred_data.infos["batch_pred_id"] = np.arange(len(pred_data))
        pred_data = pred_data[gt_views.merge(pred_data.infos)["batch_pred_id"].to_numpy()]

        pred_data.infos = add_inst_num(pred_data.infos, key="pred_inst_id", group_keys=keys)
        gt_data.infos = add_inst_num(gt_data.infos, key="gt_inst_id", group_keys=keys)

        # BOP: the best n predictions of a group
        if not self.consider_all_predictions:
            top = get_top_n_ids(pred_data.infos, group_keys=keys, top_key="score", targets=targets, n_top=self.n_top)
            kept = pred_data.clone()[np.asarray(top, dtype=int)]
        else:
            kept = pred_data.clone()

        gt_data.infos = add_valid_gt(gt_data.infos, group_keys=keys, targets=targets, visib_gt_min=self.visib_gt_min)
        cands = get_candidate_matches(kept.infos, gt_data.infos, group_keys=keys, only_valids=True)

        # candidates whose bounding spheres do not even overlap are dropped before any error is computed
        if self.spheres_overlap_check:
            dt = kept.poses[cands["pred_id"].to_numpy(), :3, -1] - gt_data.poses[cands["gt_id"].to_numpy(), :3, -1]
            overlap = torch.norm(dt, dim=-1) < torch.as_tensor(diameter(cands["label"])).to(dt.dtype).to(dt.device)
            cands = cands.iloc[np.where(overlap.cpu().numpy())[0]].reset_index(drop=True)
            cands["cand_id"] = np.arange(len(cands))

        pred_ids, gt_ids = cands["pred_id"].to_numpy(), cands["gt_id"].to_numpy()
        K = gt_data.K[gt_ids] if self.error_type == "MSPD" else None
        errors = self.compute_errors_batch(kept.poses[pred_ids], gt_data.poses[gt_ids], cands["label"].to_numpy(), K=K)
        errors = {k: v.cpu().numpy() for k, v in errors.items()}
        metric = errors["norm_max" if self.error_type in _MAX_ERRORS else "norm_avg"]

        # BOP: only errors within the threshold can be matches
        cands["error"] = metric
        cands["obj_diameter"] = diameter(cands["label"])
        in_pixels = self.error_type == "MSPD"
        limit = self.match_threshold if in_pixels else self.match_threshold * cands["obj_diameter"]
        cands = cands[cands["error"] <= limit].reset_index(drop=True)
        matches = match_poses(cands, group_keys=keys)

        gt_keys = [*keys, "gt_inst_id", "valid"] + (["visib_fract"] if "visib_fract" in gt_views else [])
        gt = gt_data.infos.loc[:, gt_keys].reset_index(drop=True)
        preds = pred_data.infos.loc[:, [*keys, "pred_inst_id", "score"]].reset_index(drop=True)
        matches = matches.loc[:, [*keys, "pred_inst_id", "gt_inst_id", "cand_id"]].reset_index(drop=True)

        cand_id = matches["cand_id"].to_numpy(dtype=int)
        matches["obj_diameter"] = diameter(matches["label"])
        matches["norm"] = metric[cand_id]
        matches["0.1d"] = metric[cand_id] < (self.match_threshold if in_pixels else 0.1 * matches["obj_diameter"].to_numpy())
        matches["xyz"] = _array_column(errors["xyz_avg"][cand_id])
        matches["TCO_xyz"] = _array_column(errors["TCO_xyz"][cand_id])
        matches["TCO_norm"] = errors["TCO_norm"][cand_id]
        preds["TXO_pred"] = _array_column(pred_data.poses.cpu().numpy())

        matches = _left_join(matches, preds, [*keys, "pred_inst_id"])
        gt = _left_join(gt, matches, [*keys, "gt_inst_id"])
        preds["0.1d"] = _left_join(preds, matches, [*keys, "pred_inst_id"])["0.1d"].to_numpy()

        self.datas["gt_df"].append(gt)
        self.datas["pred_df"].append(preds)
        self.datas["matches_df"].append(matches)

    def summary(self):
        gt_df = pd.concat(self.datas["gt_df"], ignore_index=True)
        matches_df = pd.concat(self.datas["matches_df"], ignore_index=True)
        pred_df = pd.concat(self.datas["pred_df"], ignore_index=True)

        valid_df = gt_df[gt_df["valid"].to_numpy(dtype=bool)]
        AUC = OrderedDict()
        for label, group in valid_df.groupby("label"):
            errors = group["norm"].to_numpy()
            assert np.all(~np.isnan(errors))
            AUC[label] = compute_auc_posecnn(errors)
        gt_df.attrs["AUC/objects"] = pd.Series(AUC, dtype=float)
        gt_df.attrs["AUC/objects/mean"] = float(np.nanmean(list(AUC.values()))) if np.isfinite(list(AUC.values())).any() else np.nan
        gt_df.attrs["AUC"] = compute_auc_posecnn(valid_df["norm"].to_numpy())

        # ground truths per label that count for AP / mAP at 0.1 d
        valid_k = "0.1d"
        keys = list(GROUP_KEYS)
        if self.n_top > 0:
            per_group = gt_df[[*keys, "valid"]].groupby(keys).sum().reset_index()
            per_group["gt_count"] = np.minimum(self.n_top, per_group["valid"])
            n_gts = {label: group["gt_count"].sum() for label, group in per_group.groupby("label")}
        else:
            n_gts = gt_df[["label", "valid"]].groupby("label")["valid"].sum().to_dict()

        def compute_ap(label_df, label_n_gt):
            label_df = label_df.sort_values("score", ascending=False).reset_index(drop=True)
            label_df["n_tp"] = np.cumsum(label_df[valid_k].to_numpy().astype(float))
            label_df["prec"] = label_df["n_tp"] / (np.arange(len(label_df)) + 1)
            label_df["recall"] = label_df["n_tp"] / label_n_gt
            y_true = label_df[valid_k].to_numpy(dtype=bool)
            ap = average_precision(y_true, label_df["score"]) * y_true.sum() / label_n_gt
            label_df["AP"] = ap
            label_df["n_gt"] = label_n_gt
            return ap, label_df

        ap_dfs = {}
        df = pred_df[["label", valid_k, "score"]].set_index("label")
        for label, label_n_gt in n_gts.items():
            if label in df.index:  # the reference's `df.index.contains(label)`, which pandas removed in 1.0
                label_df = df.loc[[label]]
                if label_df[valid_k].sum() > 0:
                    _, ap_dfs[label] = compute_ap(label_df, label_n_gt)
        if ap_dfs:
            mAP = np.mean([np.unique(ap_df["AP"]).item() for ap_df in ap_dfs.values()])
            AP, ap_dfs["all"] = compute_ap(df.reset_index(), sum(n_gts.values()))
        else:
            AP, mAP = 0.0, 0.0
        n_gt_valid = int(sum(n_gts.values()))

        summary = {
            "n_gt": len(gt_df),
            "n_gt_valid": n_gt_valid,
            "n_pred": len(pred_df),
            "n_matched": len(matches_df),
            "matched_gt_ratio": len(matches_df) / n_gt_valid,
            "pred_matched_ratio": len(pred_df) / max(len(matches_df), 1),
            "0.1d": float(valid_df[valid_k].sum()) / n_gt_valid,
        }
        if self.report_error_stats:
            mean_of = lambda col: np.mean(np.stack(list(matches_df[col])), axis=0).tolist() if len(matches_df) else [np.nan] * 3  # noqa: E731
            summary.update({"norm": float(matches_df["norm"].mean()), "xyz": mean_of("xyz"), "TCO_xyz": mean_of("TCO_xyz"),
                            "TCO_norm": float(matches_df["TCO_norm"].mean())})
        if self.report_AP:
            summary.update({"AP": AP, "mAP": mAP})
        if self.report_error_AUC:
            summary.update({"AUC/objects/mean": gt_df.attrs["AUC/objects/mean"], "AUC": gt_df.attrs["AUC"]})
        return summary, {"gt": gt_df, "matches": matches_df, "preds": pred_df, "ap": ap_dfs}


# ---- the ModelNet meter (MP/evaluation/meters/modelnet_meters.py) ------------------------------------------------------------------
def one_to_one_matching(pred_infos: pd.DataFrame, gt_infos: pd.DataFrame, keys=("scene_id", "view_id"),
                        allow_pred_missing: bool = False) -> pd.DataFrame:
    """``MP/evaluation/meters/utils.py:23-41``: predictions joined to ground truths on ``keys``; a key met by more than one pair,
    or (unless ``allow_pred_missing``) a ground truth without exactly one prediction, is an ``AssertionError``."""
    keys = list(keys)
    pred_infos["pred_id"] = np.arange(len(pred_infos))
    gt_infos["gt_id"] = np.arange(len(gt_infos))
    matches = pred_infos.merge(gt_infos, on=keys, suffixes=("", "_gt"))
    assert not matches.duplicated(keys).any(), "one_to_one_matching: more than one (prediction, ground truth) pair for a key"
    if not allow_pred_missing:
        assert len(matches) == len(gt_infos), "one_to_one_matching: a ground truth without a prediction"
    return matches


def angular_distance_deg(R_gt: np.ndarray, R_pred: np.ndarray, eps: float = 1e-7) -> np.ndarray:
    """``angular_distance`` of the unit quaternions of two rotations (``MP/evaluation/meters/lf_utils.py:30-40``), in degrees:
    ``2 acos(min(|q_gt . q_pred|, 1 - eps))`` with ``|q_gt . q_pred| = sqrt(max(trace(R_gt^T R_pred) + 1, 0)) / 2``, in float64
    on the host.  ``[n, 3, 3]`` each."""
    R_gt, R_pred = np.asarray(R_gt, np.float64).reshape(-1, 3, 3), np.asarray(R_pred, np.float64).reshape(-1, 3, 3)
    trace = np.einsum("nij,nij->n", R_gt, R_pred)
    dot = np.sqrt(np.maximum(trace + 1.0, 0.0)) / 2.0
    return np.rad2deg(2.0 * np.arccos(np.minimum(dot, 1.0 - eps)))


class ModelNetErrorMeter:
    """The reference's ModelNet meter: ``add0.1d``, ``5deg_5cm`` and ``proj2d_5px`` over one-to-one matched frames.

    ``mesh_db``: a ``MeshDataBase``, batched here with ``resample_n_points=sample_n_points`` (points drawn uniformly from each
    surface on the device), or tables that are already batched.  The reference scores one match per :meth:`add`; here every
    match of a call goes through ONE ``hp_pose_errors`` launch: an ADD row (``norm_avg`` = ``add``, ``TCO_norm`` = ``trans_dist``)
    and an MSPD row against an identity-only symmetry table (``norm_avg`` = the mean reprojection distance under ``gt.K``) per
    match.  ``summary()`` returns pandas, not xarray, like the other meters."""

    def __init__(self, mesh_db, sample_n_points=None, device="cuda"):
        batched = mesh_db.batched(resample_n_points=sample_n_points) if hasattr(mesh_db, "batched") else mesh_db
        # the norm of the extent of each object's own points, in float32 like the reference's tensors
        pts = np.asarray(batched.points.cpu() if isinstance(batched.points, torch.Tensor) else batched.points, dtype=np.float32)
        self.diameters = {}
        for o, label in enumerate(batched.labels):
            own = pts[o, :batched.infos[label]["n_points"]]
            self.diameters[label] = float(np.linalg.norm(own.max(0) - own.min(0)))
        self.mesh_db = batched.to(device).float()
        self.device = device
        self.reset()

    def reset(self):
        self.datas = defaultdict(list)

    def is_data_valid(self, data) -> bool:
        return hasattr(data, "K")

    def compute_errors(self, TXO_pred: torch.Tensor, TXO_gt: torch.Tensor, labels, K: torch.Tensor) -> Dict[str, np.ndarray]:
        """``add``, ``proj_error`` and ``trans_dist`` ``[n]`` of ``n`` (prediction, ground truth) pairs: one launch of ``2 n`` rows."""
        n = len(labels)
        if n == 0:
            return {k: np.zeros(0) for k in ("add", "proj_error", "trans_dist")}
        t = self.mesh_db.device_tables
        dev = t["points"].device
        n_obj = t["points"].shape[0]
        ids = np.tile(np.arange(n, dtype=np.int32), 2)
        obj_ids = np.tile(self.mesh_db.ids_of(labels), 2)
        modes = np.repeat(np.asarray([ops.POSE_ERR_MODES["ADD"], ops.POSE_ERR_MODES["MSPD"]], np.int32), n)
        identity = torch.eye(4, dtype=torch.float32, device=dev).expand(n_obj, 1, 4, 4).contiguous()
        n_pts = torch.as_tensor(np.asarray([self.mesh_db.infos[label]["n_points"] for label in self.mesh_db.labels], np.int32)).to(dev)
        K2 = torch.cat([K, K]).to(dev)
        out = ops.pose_errors_tables(ids, ids, obj_ids, modes, TXO_pred, TXO_gt, t["points"], identity,
                                     torch.ones(n_obj, dtype=torch.int32, device=dev), n_pts, K=K2)
        norm_avg, tco_norm = out["norm_avg"].cpu().numpy().astype(np.float64), out["TCO_norm"].cpu().numpy().astype(np.float64)
        return {"add": norm_avg[:n], "proj_error": norm_avg[n:], "trans_dist": tco_norm[:n]}

    def add(self, pred_data, gt_data):
        pred_data, gt_data = pred_data.float(), gt_data.float()
        matches = one_to_one_matching(pred_data.infos, gt_data.infos, keys=("scene_id", "view_id"), allow_pred_missing=False)
        pred_ids, gt_ids = matches["pred_id"].to_numpy(), matches["gt_id"].to_numpy()
        labels = matches["label"].to_numpy()  # the prediction's label, as in the reference
        TXO_pred, TXO_gt = pred_data.poses[pred_ids], gt_data.poses[gt_ids]
        errors = self.compute_errors(TXO_pred, TXO_gt, labels, gt_data.K[gt_ids])
        df = matches.reset_index(drop=True)
        df["add"] = errors["add"]
        df["diameter"] = np.asarray([self.diameters[label] for label in labels], dtype=np.float64)
        df["proj_error"] = errors["proj_error"]
        df["angular_dist"] = angular_distance_deg(TXO_gt[:, :3, :3].cpu().numpy(), TXO_pred[:, :3, :3].cpu().numpy())
        df["trans_dist"] = errors["trans_dist"]
        self.datas["df"].append(df)

    def summary(self):
        df = pd.concat(self.datas["df"], ignore_index=True)
        df.index.name = "match_id"
        add = df["add"].to_numpy() < 0.1 * df["diameter"].to_numpy()
        rot_trans = np.logical_and(df["trans_dist"].to_numpy() < 0.05, df["angular_dist"].to_numpy() < 5)
        proj_2d = df["proj_error"].to_numpy() < 5
        return {"add0.1d": add.mean(), "5deg_5cm": rot_trans.mean(), "proj2d_5px": proj_2d.mean()}, df


# ---- visible-surface discrepancy (BOP's third pose error) ------------------------------------------------------------------------
BOP_VSD_DELTA = 0.015                                                 # metres
BOP_VSD_TAUS = tuple(round(0.05 * k, 2) for k in range(1, 11))        # 0.05 ... 0.50, fractions of the diameter
BOP_VSD_THRESHOLDS = tuple(round(0.05 * k, 2) for k in range(1, 11))  # an estimate is correct when its error is below these


def _store_of(renderer):
    """The ``ops.MeshStore`` of a ``SceneRenderer`` / ``BatchRenderer``, or the store itself."""
    return renderer if isinstance(renderer, ops.MeshStore) else renderer.store


def _distinct_layers(poses: np.ndarray, labels, frames: np.ndarray):
    """Layer index of every row and the first row of every layer: rows with the same (label, frame, pose bits) share a render."""
    index, first, layer = {}, [], np.empty(len(labels), dtype=np.int64)
    for r in range(len(labels)):
        key = (labels[r], int(frames[r]), poses[r].tobytes())
        if key not in index:
            index[key] = len(first)
            first.append(r)
        layer[r] = index[key]
    return layer, np.asarray(first, dtype=np.int64)


def vsd(TXO_pred: torch.Tensor, TXO_gt: torch.Tensor, labels, depth: torch.Tensor, K: torch.Tensor, renderer, frame_ids=None,
        delta: float = BOP_VSD_DELTA, taus=BOP_VSD_TAUS, normalized_by_diameter: bool = True, layer_budget_bytes: Optional[int] = None,
        return_details: bool = False):
    """BOP's visible-surface discrepancy (BOP19 visibility rule, ``step`` cost; the definition is in ``include/happypose_amd.h``):
    ``errors [n, n_tau]`` for the candidate pairs ``(TXO_pred[i], TXO_gt[i])`` of object ``labels[i]`` seen in frame
    ``frame_ids[i]`` of ``depth [n_frames, H, W]`` (metres, 0 = no measurement) with intrinsics ``K [n_frames, 3, 3]``.
    ``frame_ids=None``: pair ``i`` belongs to frame ``i``, or every pair to the only frame.

    ``renderer``: a ``SceneRenderer``, a ``BatchRenderer`` or an ``ops.MeshStore``; the diameters are its mesh database's.  The
    DISTINCT estimated and ground-truth poses (a ground truth shared by several candidates once) are rendered depth-only at the
    frame's resolution in the single-sample state (``msaa=False, aniso=False, render_rgb=False``), at most
    ``layer_budget_bytes`` of layers at a time (default: the renderer's, else ``scene.DEFAULT_LAYER_BUDGET_BYTES``), and every chunk is
    compared by ONE ``hp_vsd`` launch enqueued behind its render: nothing synchronises with the host between the two.

    ``return_details``: also a dict with ``cost`` / ``counts`` (``ops.vsd_tables``) and, for inspection, the rendered
    ``depth_layers [L, H, W]`` with the ``est_layer`` / ``gt_layer`` / ``frame`` columns that index them."""
    from .scene import DEFAULT_LAYER_BUDGET_BYTES

    store = _store_of(renderer)
    dev = store.device
    labels = np.asarray(labels)
    n = len(labels)
    taus = np.asarray(taus, dtype=np.float32).reshape(-1)
    assert TXO_pred.shape == (n, 4, 4) and TXO_gt.shape == (n, 4, 4), "vsd: one predicted and one ground-truth pose per label"
    assert depth.dim() == 3 and K.shape == (depth.shape[0], 3, 3), "vsd: depth [n_frames, H, W] and K [n_frames, 3, 3]"
    n_frames, h, w = depth.shape
    if frame_ids is None:
        assert n_frames in (1, n), "vsd: frame_ids is needed unless there is one frame, or one per pair"
        frames = np.zeros(n, dtype=np.int64) if n_frames == 1 else np.arange(n, dtype=np.int64)
    else:
        frames = np.asarray(torch.as_tensor(frame_ids).cpu(), dtype=np.int64)
        assert frames.shape == (n,) and (n == 0 or (frames.min() >= 0 and frames.max() < n_frames)), "vsd: frame_ids outside depth"
    depth, K = depth.to(dev, torch.float32).contiguous(), K.to(dev, torch.float32).contiguous()
    errors = torch.empty((n, len(taus)), dtype=torch.float32, device=dev)
    details = {"cost": torch.empty((n, len(taus)), dtype=torch.int32, device=dev),
               "counts": torch.empty((n, ops.VSD_COUNT_FIELDS), dtype=torch.int32, device=dev),
               "est_layer": np.empty(n, dtype=np.int64), "gt_layer": np.empty(n, dtype=np.int64), "frame": frames}
    rendered: list = []
    if n:
        # the poses decide which renders are shared: they are read on the host once, before anything is enqueued
        pred_h = np.ascontiguousarray(TXO_pred.detach().to("cpu", torch.float32).numpy())
        gt_h = np.ascontiguousarray(TXO_gt.detach().to("cpu", torch.float32).numpy())
        infos = store.mesh_db.infos
        diameter = np.asarray([infos[label]["diameter_m"] for label in labels], dtype=np.float32)
        gt_layer, _ = _distinct_layers(gt_h, labels, frames)
        budget = int(layer_budget_bytes if layer_budget_bytes is not None else getattr(renderer, "layer_budget_bytes", DEFAULT_LAYER_BUDGET_BYTES))
        max_layers = max(2, budget // (h * w * 4))
        order = np.argsort(gt_layer, kind="stable")  # the candidates of one ground truth side by side: one render, one chunk
        key = lambda T, r: (labels[r], int(frames[r]), T[r].tobytes())  # noqa: E731
        chunks, held = [[]], set()
        for r in order:  # the longest runs of rows whose distinct renders fit the budget (a row needs both its layers in its chunk)
            new = {key(pred_h, r), key(gt_h, r)} - held
            if chunks[-1] and len(held) + len(new) > max_layers:
                chunks.append([])
                held, new = set(), {key(pred_h, r), key(gt_h, r)}
            chunks[-1].append(r)
            held |= new
        n_done = 0
        for rows in chunks:
            rows = np.asarray(rows, dtype=np.int64)
            m = len(rows)
            layer, first = _distinct_layers(np.concatenate([pred_h[rows], gt_h[rows]]), np.concatenate([labels[rows]] * 2),
                                            np.concatenate([frames[rows]] * 2))
            poses = np.concatenate([pred_h[rows], gt_h[rows]])[first]
            l_frames = np.concatenate([frames[rows]] * 2)[first]
            l_labels = np.concatenate([labels[rows]] * 2)[first]
            _, _, dep, _ = ops.rasterize(store, store.ids_of(list(l_labels)), torch.as_tensor(poses), K[torch.as_tensor(l_frames, device=dev)],
                                         (h, w), render_depth=True, render_rgb=False, msaa=False, aniso=False)
            out = ops.vsd_tables(layer[:m].astype(np.int32), layer[m:].astype(np.int32), frames[rows].astype(np.int32), diameter[rows], depth,
                                 dep, K, delta, taus, normalized_by_diameter)
            idx = torch.as_tensor(rows, device=dev)
            errors[idx] = out["errors"]
            if return_details:
                details["cost"][idx], details["counts"][idx] = out["cost"], out["counts"]
                details["est_layer"][rows], details["gt_layer"][rows] = layer[:m] + n_done, layer[m:] + n_done
                rendered.append(dep[:, 0])
            n_done += len(first)
    if not return_details:
        return errors
    details["depth_layers"] = torch.cat(rendered) if rendered else torch.empty((0, h, w), dtype=torch.float32, device=dev)
    return errors, details


def bop_average_recall(ar_vsd: float, ar_mssd: float, ar_mspd: float) -> float:
    """BOP's score of a method on a dataset: the mean of the three average recalls."""
    return (float(ar_vsd) + float(ar_mssd) + float(ar_mspd)) / 3.0


class VsdMeter:
    """Average recall under VSD (``AR_VSD`` of the BOP challenge): the fraction of valid ground-truth instances matched by an
    estimate whose VSD error at misalignment tolerance ``tau`` is below the correctness threshold ``theta``, averaged over all
    ``(tau, theta)`` of ``taus x correct_ths``.

    ``renderer``: what :func:`vsd` accepts; ``mesh_db`` (a ``MeshDataBase`` or its ``batched()`` tables) names the objects a
    prediction may carry.  ``targets`` / ``visib_gt_min`` / ``n_top`` select ground truths and predictions as in
    :class:`PoseErrorMeter`; the matching is its ``get_candidate_matches`` / ``match_poses``, run once per ``(tau, theta)``."""

    def __init__(self, renderer, mesh_db=None, delta: float = BOP_VSD_DELTA, taus=BOP_VSD_TAUS, correct_ths=BOP_VSD_THRESHOLDS,
                 normalized_by_diameter: bool = True, targets=None, visib_gt_min=-1, n_top=-1, device="cuda"):
        self.renderer = renderer
        self.mesh_db = mesh_db
        self.delta = float(delta)
        self.taus = tuple(float(t) for t in taus)
        self.correct_ths = tuple(float(t) for t in correct_ths)
        assert 1 <= len(self.taus) <= ops.VSD_MAX_TAUS and len(self.correct_ths) >= 1
        self.normalized_by_diameter = bool(normalized_by_diameter)
        self.targets = targets
        self.visib_gt_min = visib_gt_min
        self.n_top = n_top
        self.device = device
        self.reset()

    def reset(self):
        self.n_gt_valid = 0
        self.n_matched = np.zeros((len(self.taus), len(self.correct_ths)), dtype=np.int64)
        self.datas = defaultdict(list)

    def compute_errors(self, TXO_pred, TXO_gt, labels, depth, K, frame_ids) -> np.ndarray:
        """The one device call of the meter: ``[n, n_tau]`` VSD errors of the candidate pairs."""
        if len(labels) == 0:
            return np.empty((0, len(self.taus)), dtype=np.float32)
        return vsd(TXO_pred, TXO_gt, labels, depth, K, self.renderer, frame_ids=frame_ids, delta=self.delta, taus=self.taus,
                   normalized_by_diameter=self.normalized_by_diameter).cpu().numpy()

    def add(self, pred_data, gt_data, depth, K, frames=None):
        """``pred_data`` / ``gt_data``: collections with ``poses [n, 4, 4]`` and ``infos`` (``scene_id``, ``view_id``, ``label``;
        predictions also ``score``, 1 when absent).  ``depth [n_frames, H, W]`` and ``K [n_frames, 3, 3]`` are the measured
        frames; ``frames`` lists their ``(scene_id, view_id)`` in that order (default: the views of ``gt_data`` in order of
        first appearance)."""
        keys = list(GROUP_KEYS)
        pred_data, gt_data = pred_data.float(), gt_data.float()
        if "score" not in pred_data.infos:
            pred_data.infos["score"] = 1.0
        if self.mesh_db is not None:
            unknown = sorted(set(pred_data.infos["label"]) - set(self.mesh_db.infos))
            assert not unknown, f"VsdMeter: labels {unknown} are not in mesh_db"
        gt_views = gt_data.infos.loc[:, ["scene_id", "view_id"]].drop_duplicates().reset_index(drop=True)
        if frames is None:
            frames = list(zip(gt_views["scene_id"], gt_views["view_id"]))
        frame_of = {(s, v): i for i, (s, v) in enumerate(frames)}
        assert len(frame_of) == len(frames) == depth.shape[0] == K.shape[0], "VsdMeter: one distinct (scene_id, view_id) per frame of depth and K"
        targets = self.targets
        if targets is not None:
            targets = gt_views.merge(targets)
        pred_data.infos["batch_pred_id"] = np.arange(len(pred_data))
        pred_data = pred_data[gt_views.merge(pred_data.infos)["batch_pred_id"].to_numpy()]
        pred_data.infos = add_inst_num(pred_data.infos, key="pred_inst_id", group_keys=keys)
        gt_data.infos = add_inst_num(gt_data.infos, key="gt_inst_id", group_keys=keys)
        top = get_top_n_ids(pred_data.infos, group_keys=keys, top_key="score", targets=targets, n_top=self.n_top)
        kept = pred_data.clone()[np.asarray(top, dtype=int)]
        gt_data.infos = add_valid_gt(gt_data.infos, group_keys=keys, targets=targets, visib_gt_min=self.visib_gt_min)
        cands = get_candidate_matches(kept.infos, gt_data.infos, group_keys=keys, only_valids=True)

        pred_ids, gt_ids = cands["pred_id"].to_numpy(), cands["gt_id"].to_numpy()
        frame_ids = np.asarray([frame_of[(s, v)] for s, v in zip(cands["scene_id"], cands["view_id"])], dtype=np.int64)
        errors = np.asarray(self.compute_errors(kept.poses[pred_ids], gt_data.poses[gt_ids], cands["label"].to_numpy(), depth, K, frame_ids))
        assert errors.shape == (len(cands), len(self.taus))

        self.n_gt_valid += int(gt_data.infos["valid"].sum())
        for ti in range(len(self.taus)):
            cands["error"] = errors[:, ti]
            for ci, th in enumerate(self.correct_ths):  # BOP: an estimate is correct when its error is BELOW the threshold
                self.n_matched[ti, ci] += len(match_poses(cands[cands["error"] < th].reset_index(drop=True), group_keys=keys))
        cands = cands.drop(columns="error")
        for ti, tau in enumerate(self.taus):
            cands[f"vsd_{tau:g}"] = errors[:, ti]
        self.datas["cand_df"].append(cands)

    def summary(self):
        """``(summary, dfs)``: ``summary["AR_VSD"]`` and the counts; ``dfs["recall"]`` has one row per ``(tau, threshold)`` with
        ``n_matched`` and ``recall``, ``dfs["cands"]`` every candidate pair with its errors."""
        recall = self.n_matched / self.n_gt_valid if self.n_gt_valid else np.zeros(self.n_matched.shape)
        table = pd.DataFrame([{"tau": tau, "threshold": th, "n_matched": int(self.n_matched[ti, ci]), "recall": float(recall[ti, ci])}
                              for ti, tau in enumerate(self.taus) for ci, th in enumerate(self.correct_ths)])
        cands = pd.concat(self.datas["cand_df"], ignore_index=True) if self.datas["cand_df"] else pd.DataFrame()
        summary = {"n_gt_valid": int(self.n_gt_valid), "n_cand": len(cands), "AR_VSD": float(recall.mean())}
        return summary, {"recall": table, "cands": cands}


# ---- detections and instance masks (CP/evaluation/meters/detection_meters.py; COCO average precision) ----------------------------
# The IoU definitions and the matching rule are restated in include/happypose_amd.h (csrc/det_eval.hip).  CocoMeter is the PUBLISHED
# definition of COCO's average precision (pycocotools 2.0: COCOeval.evaluateImg / accumulate / summarize, without area ranges and
# crowd regions) restated here: pycocotools is not a dependency, so nothing below could be pinned against it.
COCO_IOU_THRESHOLDS = tuple(round(0.5 + 0.05 * k, 2) for k in range(10))  # 0.50 : 0.05 : 0.95
COCO_RECALL_POINTS = np.linspace(0.0, 1.0, 101)


def _all_pairs(n1: int, n2: int):
    return np.repeat(np.arange(n1, dtype=np.int32), n2), np.tile(np.arange(n2, dtype=np.int32), n1)


def box_iou(boxes1: torch.Tensor, boxes2: torch.Tensor) -> torch.Tensor:
    """``torchvision.ops.box_iou``: ``[n1, n2]`` IoU of xyxy boxes on the device (0 / 0 is NaN, as there)."""
    n1, n2 = boxes1.shape[0], boxes2.shape[0]
    if n1 * n2 == 0:
        return torch.empty((n1, n2), dtype=torch.float32, device=boxes1.device)
    i, j = _all_pairs(n1, n2)
    return ops.det_iou(i, j, boxes_pred=boxes1, boxes_gt=boxes2)["box_iou"].reshape(n1, n2)


def mask_iou(masks1: torch.Tensor, masks2: torch.Tensor) -> torch.Tensor:
    """``[n1, n2]`` IoU of ``[n, H, W]`` bool / uint8 masks on the device; 0 where both masks are empty.  Each mask is bit-packed
    once; no ``[n1, n2, H, W]`` temporary exists."""
    n1, n2 = masks1.shape[0], masks2.shape[0]
    assert masks1.shape[1:] == masks2.shape[1:], "mask_iou: one resolution"
    if n1 * n2 == 0:
        return torch.empty((n1, n2), dtype=torch.float32, device=masks1.device)
    i, j = _all_pairs(n1, n2)
    return ops.det_iou(i, j, packed_pred=ops.mask_pack(masks1), packed_gt=ops.mask_pack(masks2))["mask_iou"].reshape(n1, n2)


def plan_detection_rows(pred_infos: pd.DataFrame, gt_infos: pd.DataFrame, max_dets: Optional[int] = None, group_keys=GROUP_KEYS):
    """The rows of a detection evaluation, on the host alone.  A group is one value of ``group_keys`` present in either frame
    (groups in sorted key order).  Inside a group the detections are ordered by descending ``score`` (stable: equal scores keep
    their row order) and capped at ``max_dets``; the ground truths by ``ignore`` (column of ``gt_infos``, all False when absent),
    the non-ignored ones first, stable.  Returns a dict:

    ``groups``     DataFrame: the keys, ``n_det``, ``n_gt`` and the starts ``row_off`` / ``det_off`` / ``gt_off`` of every group;
    ``det_order``  row positions in ``pred_infos`` of the kept detections, group after group, with ``det_group`` (their group);
    ``gt_order``   row positions in ``gt_infos`` likewise, with ``gt_group`` and ``gt_ignore``;
    ``pred_idx`` / ``gt_idx``  the rows for ``ops.det_iou``: every group's ``n_det x n_gt`` pairs, detection-major, as row positions
                   in the two frames -- what ``ops.det_match`` expects as its dense matrices."""
    keys = list(group_keys)
    score = pred_infos["score"].to_numpy(dtype=float) if len(pred_infos) else np.zeros(0)
    ignore = gt_infos["ignore"].to_numpy(dtype=bool) if "ignore" in gt_infos else np.zeros(len(gt_infos), dtype=bool)
    members: Dict[tuple, list] = {}
    for side, infos in enumerate((pred_infos, gt_infos)):
        cols = [infos[k].tolist() for k in keys] if len(infos) else [[] for _ in keys]
        for row, key in enumerate(zip(*cols)):
            members.setdefault(key, ([], []))[side].append(row)
    table, det_order, gt_order, det_group, gt_group, pred_idx, gt_idx = [], [], [], [], [], [], []
    row_off = det_off = gt_off = 0
    for g, key in enumerate(sorted(members)):
        dets, gts = (np.asarray(m, dtype=np.int64) for m in members[key])
        dets = dets[np.argsort(-score[dets], kind="mergesort")]
        if max_dets is not None:
            dets = dets[:max_dets]
        gts = gts[np.argsort(ignore[gts], kind="mergesort")]
        table.append((*key, len(dets), len(gts), row_off, det_off, gt_off))
        det_order.append(dets), gt_order.append(gts)
        det_group.append(np.full(len(dets), g)), gt_group.append(np.full(len(gts), g))
        pred_idx.append(np.repeat(dets, len(gts))), gt_idx.append(np.tile(gts, len(dets)))
        row_off, det_off, gt_off = row_off + len(dets) * len(gts), det_off + len(dets), gt_off + len(gts)
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)  # noqa: E731
    gt_order = cat(gt_order)
    return {"groups": pd.DataFrame(table, columns=[*keys, "n_det", "n_gt", "row_off", "det_off", "gt_off"]),
            "det_order": cat(det_order), "det_group": cat(det_group), "gt_order": gt_order, "gt_group": cat(gt_group),
            "gt_ignore": ignore[gt_order], "pred_idx": cat(pred_idx), "gt_idx": cat(gt_idx)}


def _device_iou(iou_type: str, plan, pred_data, gt_data) -> Dict[str, torch.Tensor]:
    """The one ``hp_det_iou`` launch of an ``add`` call: the plan's rows on the boxes (``bbox``) or on the masks, packed once
    each (``segm``)."""
    if iou_type == "bbox":
        return ops.det_iou(plan["pred_idx"], plan["gt_idx"], boxes_pred=pred_data.bboxes.float(), boxes_gt=gt_data.bboxes.float())
    return ops.det_iou(plan["pred_idx"], plan["gt_idx"], packed_pred=ops.mask_pack(pred_data.masks), packed_gt=ops.mask_pack(gt_data.masks))


def _check_iou_type(iou_type: str) -> str:
    if iou_type not in ("bbox", "segm"):
        raise ValueError("iou_type must be 'bbox' or 'segm'", iou_type)
    return iou_type


class DetectionMeter:
    """The reference's ``DetectionMeter`` with its constructor arguments, plus ``iou_type``: ``"bbox"`` scores ``bboxes [n, 4]``
    (xyxy) with torchvision's ``box_iou``, ``"segm"`` scores ``masks [n, H, W]`` (bool) with the mask IoU.  ``add`` and ``summary``
    follow the reference step by step; every candidate pair of an ``add`` call goes through ONE ``hp_det_iou`` launch, so
    ``errors_bsz`` is kept for compatibility and ignored.  ``summary()`` returns the reference's keys and pandas frames instead
    of xarray datasets, like :class:`PoseErrorMeter`."""

    def __init__(self, iou_threshold=0.5, errors_bsz=512, consider_all_predictions=False, targets=None, visib_gt_min=-1, n_top=-1,
                 iou_type="bbox"):
        self.iou_threshold = iou_threshold
        self.consider_all_predictions = consider_all_predictions
        self.targets = targets
        self.visib_gt_min = visib_gt_min
        self.errors_bsz = errors_bsz
        self.n_top = n_top
        self.iou_type = _check_iou_type(iou_type)
        self.reset()

    def reset(self):
        self.datas = defaultdict(list)

    def add(self, pred_data, gt_data):
        keys = list(GROUP_KEYS)
        # predictions of the scenes and views the ground truth covers
        gt_views = gt_data.infos.loc[:, ["scene_id", "view_id"]].drop_duplicates().reset_index(drop=True)
        targets = self.targets
        if targets is not None:
            targets = gt_views.merge(targets)
        pred_data.infos["batch_pred_id"] = np.arange(len(pred_data))
        pred_data = pred_data[gt_views.merge(pred_data.infos)["batch_pred_id"].to_numpy()]

        pred_data.infos = add_inst_num(pred_data.infos, key="pred_inst_id", group_keys=keys)
        gt_data.infos = add_inst_num(gt_data.infos, key="gt_inst_id", group_keys=keys)

        # BOP: the best n predictions of a group
        if not self.consider_all_predictions:
            top = get_top_n_ids(pred_data.infos, group_keys=keys, top_key="score", targets=targets, n_top=self.n_top)
            kept = pred_data.clone()[np.asarray(top, dtype=int)]
        else:
            kept = pred_data.clone()

        gt_data.infos = add_valid_gt(gt_data.infos, group_keys=keys, targets=targets, visib_gt_min=self.visib_gt_min)
        cands = get_candidate_matches(kept.infos, gt_data.infos, group_keys=keys, only_valids=True)

        # the candidates are the rows of the plan over the valid ground truths: one launch, rows sorted by group
        valid_rows = np.where(gt_data.infos["valid"].to_numpy(dtype=bool))[0]
        plan = plan_detection_rows(kept.infos, gt_data.infos.iloc[valid_rows].drop(columns="ignore", errors="ignore"), group_keys=keys)
        plan["gt_idx"] = valid_rows[plan["gt_idx"]]
        out = _device_iou(self.iou_type, plan, kept, gt_data)
        iou_rows = out["box_iou" if self.iou_type == "bbox" else "mask_iou"].cpu().numpy().astype(np.float64)
        n_gt_rows = max(len(gt_data.infos), 1)
        pair = plan["pred_idx"] * n_gt_rows + plan["gt_idx"]
        sorter = np.argsort(pair, kind="stable")
        want = cands["pred_id"].to_numpy(dtype=np.int64) * n_gt_rows + cands["gt_id"].to_numpy(dtype=np.int64)
        assert len(want) == len(pair) and np.array_equal(pair[sorter], np.sort(want)), "plan and candidates name different pairs"
        ious = iou_rows[sorter[np.searchsorted(pair[sorter], want)]] if len(want) else np.zeros(0)

        # matches can only be candidates within the threshold
        cands["iou"] = ious
        cands = cands[cands["iou"] >= self.iou_threshold].reset_index(drop=True)
        cands["error"] = -cands["iou"]
        matches = match_poses(cands, group_keys=keys)

        gt_keys = [*keys, "gt_inst_id", "valid"] + (["visib_fract"] if "visib_fract" in gt_views else [])
        gt = gt_data.infos.loc[:, gt_keys].reset_index(drop=True)
        preds = pred_data.infos.loc[:, [*keys, "pred_inst_id", "score"]].reset_index(drop=True)
        matches = matches.loc[:, [*keys, "pred_inst_id", "gt_inst_id", "cand_id"]].reset_index(drop=True)
        match_iou = ious[matches["cand_id"].to_numpy(dtype=int)]
        matches["iou"] = match_iou
        matches["iou_valid"] = match_iou >= self.iou_threshold

        matches = _left_join(matches, preds, [*keys, "pred_inst_id"])
        gt = _left_join(gt, matches, [*keys, "gt_inst_id"])
        preds["iou_valid"] = _left_join(preds, matches, [*keys, "pred_inst_id"])["iou_valid"].to_numpy()

        self.datas["gt_df"].append(gt)
        self.datas["pred_df"].append(preds)
        self.datas["matches_df"].append(matches)

    def summary(self):
        gt_df = pd.concat(self.datas["gt_df"], ignore_index=True)
        matches_df = pd.concat(self.datas["matches_df"], ignore_index=True)
        pred_df = pd.concat(self.datas["pred_df"], ignore_index=True)
        valid_df = gt_df[gt_df["valid"].to_numpy(dtype=bool)]

        # AP / mAP at the IoU threshold
        valid_k = "iou_valid"
        keys = list(GROUP_KEYS)
        if self.n_top > 0:
            per_group = gt_df[[*keys, "valid"]].groupby(keys).sum().reset_index()
            per_group["gt_count"] = np.minimum(self.n_top, per_group["valid"])
            n_gts = {label: group["gt_count"].sum() for label, group in per_group.groupby("label")}
        else:
            n_gts = gt_df[["label", "valid"]].groupby("label")["valid"].sum().to_dict()

        def compute_ap(label_df, label_n_gt):
            label_df = label_df.sort_values("score", ascending=False).reset_index(drop=True)
            label_df["n_tp"] = np.cumsum(label_df[valid_k].to_numpy().astype(float))
            label_df["prec"] = label_df["n_tp"] / (np.arange(len(label_df)) + 1)
            label_df["recall"] = label_df["n_tp"] / label_n_gt
            y_true = label_df[valid_k].to_numpy(dtype=bool)
            ap = average_precision(y_true, label_df["score"]) * y_true.sum() / label_n_gt
            label_df["AP"] = ap
            label_df["n_gt"] = label_n_gt
            return ap, label_df

        ap_dfs = {}
        df = pred_df[["label", valid_k, "score"]].set_index("label")
        for label, label_n_gt in n_gts.items():
            if label in df.index:  # the reference's `df.index.contains(label)`, which pandas removed in 1.0
                label_df = df.loc[[label]]
                if label_df[valid_k].sum() > 0:
                    _, ap_dfs[label] = compute_ap(label_df, label_n_gt)
        if ap_dfs:
            mAP = np.mean([np.unique(ap_df["AP"]).item() for ap_df in ap_dfs.values()])
            AP, ap_dfs["all"] = compute_ap(df.reset_index(), sum(n_gts.values()))
        else:
            AP, mAP = 0.0, 0.0
        n_gt_valid = int(sum(n_gts.values()))

        summary = {
            "n_gt": len(gt_df),
            "n_gt_valid": n_gt_valid,
            "n_pred": len(pred_df),
            "n_matched": len(matches_df),
            "matched_gt_ratio": len(matches_df) / n_gt_valid,
            "pred_matched_ratio": len(pred_df) / max(len(matches_df), 1),
            "iou_valid_recall": float(valid_df[valid_k].sum()) / n_gt_valid,
            "AP": AP,
            "mAP": mAP,
        }
        return summary, {"gt": gt_df, "matches": matches_df, "preds": pred_df, "ap": ap_dfs}


def coco_accumulate(det_label, det_score, det_match, det_ignore, gt_label, gt_ignore, iou_thresholds=COCO_IOU_THRESHOLDS):
    """COCO's ``accumulate`` and ``summarize`` on match tables, in numpy float64.  ``det_match`` / ``det_ignore`` are
    ``[n_thr, n_det]`` (match >= 0: matched), the other arguments one entry per detection / ground truth; detections are taken in
    the order given (frame after frame).  Per (label, threshold): sort by descending score (mergesort), cumulative true and false
    positives without the ignored detections, ``recall = tp / n_gt_not_ignored``, ``precision = tp / (tp + fp + eps)`` made
    monotone from the right and sampled at the 101 recall points with ``searchsorted(side="left")``.  A label without a
    non-ignored ground truth is left out.  Returns ``(summary, per_label)``: ``AP`` (mean over labels, thresholds and recall
    points), ``AP50`` / ``AP75`` (-1 when the threshold is not evaluated), ``AR`` (mean final recall), -1 throughout when no label
    counts; ``per_label`` has one row per counted label."""
    thr = np.asarray(iou_thresholds, dtype=np.float64).reshape(-1)
    det_label, gt_label = np.asarray(det_label, dtype=object), np.asarray(gt_label, dtype=object)
    det_score = np.asarray(det_score, dtype=np.float64)
    matched = np.asarray(det_match).reshape(len(thr), -1) >= 0
    det_ignore = np.asarray(det_ignore, dtype=bool).reshape(len(thr), -1)
    gt_ignore = np.asarray(gt_ignore, dtype=bool)
    eps = np.spacing(1.0)
    rows, precisions, recalls = [], [], []
    for label in sorted(set(gt_label.tolist())):
        n_gt = int(np.sum((gt_label == label) & ~gt_ignore))
        if n_gt == 0:
            continue
        of_label = np.where(det_label == label)[0]
        order = of_label[np.argsort(-det_score[of_label], kind="mergesort")]
        tps, fps = matched[:, order] & ~det_ignore[:, order], ~matched[:, order] & ~det_ignore[:, order]
        tp_sum, fp_sum = np.cumsum(tps, axis=1).astype(np.float64), np.cumsum(fps, axis=1).astype(np.float64)
        precision, recall = np.zeros((len(thr), len(COCO_RECALL_POINTS))), np.zeros(len(thr))
        for t in range(len(thr)):
            tp, fp = tp_sum[t], fp_sum[t]
            if len(tp) == 0:
                continue
            rc = tp / n_gt
            pr = tp / (fp + tp + eps)
            recall[t] = rc[-1]
            pr = np.maximum.accumulate(pr[::-1])[::-1]
            at = np.searchsorted(rc, COCO_RECALL_POINTS, side="left")
            inside = at < len(pr)
            precision[t, inside] = pr[at[inside]]
        precisions.append(precision), recalls.append(recall)
        rows.append({"label": label, "n_gt": n_gt, "n_det": len(order), "AP": float(precision.mean()), "AR": float(recall.mean())})
    if not rows:
        nothing = {"AP": -1.0, "AP50": -1.0, "AP75": -1.0, "AR": -1.0}
        return nothing, pd.DataFrame(rows, columns=["label", "n_gt", "n_det", "AP", "AR"])
    precisions, recalls = np.stack(precisions), np.stack(recalls)  # [labels, thr, 101], [labels, thr]

    def at_threshold(value):
        t = np.where(np.isclose(thr, value))[0]
        return float(precisions[:, t[0]].mean()) if len(t) else -1.0

    per_label = pd.DataFrame(rows)
    for name, value in (("AP50", 0.5), ("AP75", 0.75)):
        t = np.where(np.isclose(thr, value))[0]
        per_label[name] = precisions[:, t[0]].mean(axis=1) if len(t) else -1.0
    return {"AP": float(precisions.mean()), "AP50": at_threshold(0.5), "AP75": at_threshold(0.75), "AR": float(recalls.mean())}, per_label


class CocoMeter:
    """BOP's score of its 2D detection (``iou_type="bbox"``) and 2D segmentation (``"segm"``) tasks: COCO average precision over
    ``iou_thresholds``, at most ``max_dets`` detections per frame and label.  This is the PUBLISHED definition (pycocotools 2.0
    without area ranges and crowd regions) restated here -- pycocotools is not a dependency and nothing was pinned against it.

    ``add(pred_data, gt_data)`` reads ``infos`` (``scene_id``, ``view_id``, ``label``; ``score`` on predictions) and ``bboxes
    [n, 4]`` xyxy or ``masks [n, H, W]`` bool.  A ground truth is ignored when its ``ignore`` column is set, or when
    ``visib_gt_min`` is given and its ``visib_fract`` is below it; BOP's own visibility cut-off is NOT built in -- pass it.  Every
    prediction counts, also on a frame without ground truth.  ``add`` packs the masks, scores all pairs of a frame and label in one
    ``hp_det_iou`` launch and matches them in one ``hp_det_match`` launch; only the match tables come to the host.
    ``summary()`` is :func:`coco_accumulate` over everything added: ``AP``, ``AP50``, ``AP75``, ``AR`` (recall at ``max_dets``)
    and the frames ``labels`` (per label), ``dets`` and ``gts`` (the match tables, one ``match_<thr>`` column per threshold)."""

    def __init__(self, iou_type="bbox", iou_thresholds=COCO_IOU_THRESHOLDS, max_dets=100, visib_gt_min=None):
        self.iou_type = _check_iou_type(iou_type)
        self.iou_thresholds = tuple(float(t) for t in iou_thresholds)
        assert len(self.iou_thresholds) >= 1
        self.max_dets = int(max_dets)
        self.visib_gt_min = visib_gt_min
        self.reset()

    def reset(self):
        self.datas = defaultdict(list)

    def add(self, pred_data, gt_data):
        keys = list(GROUP_KEYS)
        pred_infos, gt_infos = pred_data.infos.reset_index(drop=True), gt_data.infos.reset_index(drop=True).copy()
        ignore = gt_infos["ignore"].to_numpy(dtype=bool) if "ignore" in gt_infos else np.zeros(len(gt_infos), dtype=bool)
        if self.visib_gt_min is not None:
            ignore = ignore | (gt_infos["visib_fract"].to_numpy(dtype=float) < self.visib_gt_min)
        gt_infos["ignore"] = ignore
        plan = plan_detection_rows(pred_infos, gt_infos, max_dets=self.max_dets, group_keys=keys)
        n_thr = len(self.iou_thresholds)
        if len(plan["pred_idx"]):
            out = _device_iou(self.iou_type, plan, pred_data, gt_data)
            iou = out["box_iou" if self.iou_type == "bbox" else "mask_iou"]
            tables = ops.det_match(iou, plan["groups"]["n_det"].to_numpy(), plan["groups"]["n_gt"].to_numpy(), plan["gt_ignore"],
                                   self.iou_thresholds)
            tables = {k: v.cpu().numpy() for k, v in tables.items()}
        else:  # nothing to compare: every detection is unmatched
            tables = {"det_match": np.full((n_thr, len(plan["det_order"])), -1, dtype=np.int32),
                      "det_ignore": np.zeros((n_thr, len(plan["det_order"])), dtype=bool),
                      "gt_match": np.full((n_thr, len(plan["gt_order"])), -1, dtype=np.int32)}
        dets = pred_infos.iloc[plan["det_order"]][[*keys, "score"]].reset_index(drop=True)
        gts = gt_infos.iloc[plan["gt_order"]][[*keys, "ignore"]].reset_index(drop=True)
        self.datas["dets"].append(dets), self.datas["gts"].append(gts)
        for k, v in tables.items():
            self.datas[k].append(v)

    def summary(self):
        keys = list(GROUP_KEYS)
        dets = pd.concat(self.datas["dets"], ignore_index=True) if self.datas["dets"] else pd.DataFrame(columns=[*keys, "score"])
        gts = pd.concat(self.datas["gts"], ignore_index=True) if self.datas["gts"] else pd.DataFrame(columns=[*keys, "ignore"])
        n_thr = len(self.iou_thresholds)
        cat = lambda k, dtype: np.concatenate(self.datas[k], axis=1) if self.datas[k] else np.zeros((n_thr, 0), dtype=dtype)  # noqa: E731
        det_match, det_ignore, gt_match = cat("det_match", np.int32), cat("det_ignore", bool), cat("gt_match", np.int32)
        summary, per_label = coco_accumulate(dets["label"].to_numpy(), dets["score"].to_numpy(), det_match, det_ignore,
                                             gts["label"].to_numpy(), gts["ignore"].to_numpy(), self.iou_thresholds)
        for t, thr in enumerate(self.iou_thresholds):
            dets[f"match_{thr:g}"], dets[f"ignore_{thr:g}"], gts[f"match_{thr:g}"] = det_match[t], det_ignore[t], gt_match[t]
        summary.update({"n_pred": len(dets), "n_gt": len(gts), "n_gt_not_ignored": int((~gts["ignore"].to_numpy(dtype=bool)).sum())})
        return summary, {"labels": per_label, "dets": dets, "gts": gts}


def bop_box_to_xyxy(boxes) -> np.ndarray:
    """BOP's inclusive ``(x, y, w, h)`` (the box covers pixels ``x .. x + w - 1``) as the xyxy box ``(x, y, x + w, y + h)`` of the
    pixel AREA, whose width is ``w``: what ``box_iou`` measures."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    return np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], axis=1)


def scene_ground_truth(scene_renderer, object_datas, camera_datas, frames) -> PandasTensorCollection:
    """Ground-truth detections of a rendered scene, for datasets without mask files: one row per (camera, object) with at least
    one visible pixel.  ``frames`` lists the ``(scene_id, view_id)`` of every camera.  ``masks`` [n, H, W] bool are the pixels the
    object wins in its camera's composed id map, ``bboxes`` [n, 4] the xyxy form of BOP's ``bbox_visib``, and ``infos`` carries
    ``scene_id``, ``view_id``, ``label``, ``cam_id``, ``obj_id``, ``px_count_all``, ``px_count_visib`` and ``visib_fract``.  All
    cameras must share one resolution.  Built on ``render_scene_tensors`` and ``ops.scene_visibility``."""
    from .scene import _object_data

    objects = [_object_data(o) for o in object_datas]
    assert len(frames) == len(camera_datas), "scene_ground_truth: one (scene_id, view_id) per camera"
    groups = scene_renderer.render_scene_tensors(objects, camera_datas, [], render_depth=True, keep_layer_depth=True)
    assert len(groups) == 1, "scene_ground_truth: the cameras must share one resolution"
    (g,) = groups
    table = ops.scene_visibility(g["layer_off"], g["layer_depth"], g["ids"]).cpu().numpy()
    n_obj = len(objects)
    layer_object = g["layer_object"].cpu().numpy()
    local_cam = np.repeat(np.arange(len(g["cameras"])), n_obj)
    keep = np.where(table[:, 1] > 0)[0]
    dev = g["ids"].device
    masks = g["ids"][torch.as_tensor(local_cam[keep], device=dev)] == torch.as_tensor(layer_object[keep], device=dev, dtype=torch.int32)[:, None, None]
    t = table[keep]
    boxes = bop_box_to_xyxy(np.stack([t[:, 6], t[:, 7], t[:, 8] - t[:, 6] + 1, t[:, 9] - t[:, 7] + 1], axis=1)) if len(keep) else np.zeros((0, 4), np.float32)
    cams = [g["cameras"][c] for c in local_cam[keep]]
    infos = pd.DataFrame({"scene_id": [frames[c][0] for c in cams], "view_id": [frames[c][1] for c in cams],
                          "label": [objects[j].label for j in layer_object[keep]], "cam_id": cams, "obj_id": layer_object[keep].astype(int),
                          "px_count_all": t[:, 0].astype(int), "px_count_visib": t[:, 1].astype(int),
                          "visib_fract": t[:, 1] / np.maximum(t[:, 0], 1)})
    return PandasTensorCollection(infos, masks=masks, bboxes=torch.as_tensor(boxes, device=dev))
