"""Host side of the pose-error evaluation (happypose_amd/evaluation.py) without a GPU: the restated bookkeeping functions against
the reference's recorded outputs (tests/golden/g12_pose_errors.npz), and PoseErrorMeter on a case worked out by hand, with the
one device call replaced by the float64 helper (tests/pose_errors_ref.py)."""

import re
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pose_errors_ref as R  # noqa: E402

from happypose_amd import evaluation as E  # noqa: E402
from happypose_amd import ops  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
KEYS = ["scene_id", "view_id", "label"]


@pytest.fixture(scope="module")
def g12(golden_dir):
    return np.load(golden_dir / "g12_pose_errors.npz")


def _frame(g, name, last):
    return pd.DataFrame({"scene_id": g[f"{name}/scene_id"], "view_id": g[f"{name}/view_id"],
                         "label": [f"obj_{i:06d}" for i in g[f"{name}/label_id"]], last: g[f"{name}/{last}"]})


@pytest.fixture()
def tables(g12):
    return _frame(g12, "pred", "score"), _frame(g12, "gt", "visib_fract"), _frame(g12, "targets", "inst_count")


def test_constants_follow_the_header():
    text = (ROOT / "include" / "happypose_amd.h").read_text()
    defs = {k: int(v) for k, v in re.findall(r"#define HP_POSE_ERR_([A-Z_]+) (\d+)", text)}
    assert ops.POSE_ERR_PRED_TILE == defs.pop("PRED_TILE") and ops.POSE_ERR_GT_BLOCK == defs.pop("GT_BLOCK")
    assert {k.replace("-", "_"): v for k, v in ops.POSE_ERR_MODES.items()} == defs
    assert set(R.MODES) == set(ops.POSE_ERR_MODES)


def test_add_inst_num(g12, tables):
    pred, gt, _ = tables
    assert np.array_equal(E.add_inst_num(pred, key="pred_inst_id", group_keys=KEYS)["pred_inst_id"], g12["host/pred_inst_id"])
    assert np.array_equal(E.add_inst_num(gt, key="gt_inst_id", group_keys=KEYS)["gt_inst_id"], g12["host/gt_inst_id"])


def test_get_top_n_ids(g12, tables):
    pred, _, targets = tables
    assert np.array_equal(E.get_top_n_ids(pred.copy(), group_keys=KEYS, top_key="score"), g12["host/top_all"])
    assert np.array_equal(E.get_top_n_ids(pred.copy(), group_keys=KEYS, top_key="score", n_top=2), g12["host/top_2"])
    assert np.array_equal(E.get_top_n_ids(pred.copy(), group_keys=KEYS, top_key="score", targets=targets), g12["host/top_targets"])
    assert len(g12["host/top_targets"]) < len(g12["host/top_2"]) < len(g12["host/top_all"])
    assert len(E.get_top_n_ids(pred.iloc[:0].copy(), group_keys=KEYS)) == 0


def test_add_valid_gt(g12, tables):
    _, gt, targets = tables
    assert np.array_equal(E.add_valid_gt(gt.copy(), group_keys=KEYS)["valid"], g12["host/valid_all"])
    assert np.array_equal(E.add_valid_gt(gt.copy(), group_keys=KEYS, visib_gt_min=0.1)["valid"], g12["host/valid_visib"])
    assert np.array_equal(E.add_valid_gt(gt.copy(), group_keys=KEYS, visib_gt_min=0.1, targets=targets)["valid"],
                          g12["host/valid_visib_targets"])
    assert np.array_equal(E.add_valid_gt(gt.copy(), group_keys=KEYS, targets=targets)["valid"], g12["host/valid_targets"])
    assert 0 < g12["host/valid_targets"].sum() < g12["host/valid_visib"].sum() < len(gt)


def test_candidates_and_matching(g12, tables):
    pred, gt, targets = tables
    gt = E.add_valid_gt(gt, group_keys=KEYS, targets=targets)
    for tag, only in (("cand", True), ("cand_all", False)):
        cands = E.get_candidate_matches(pred.copy(), gt.copy(), group_keys=KEYS, only_valids=only)
        assert np.array_equal(cands["pred_id"], g12[f"host/{tag}_pred_id"]) and np.array_equal(cands["gt_id"], g12[f"host/{tag}_gt_id"])
        assert np.array_equal(cands["cand_id"], np.arange(len(cands)))
    cands = E.get_candidate_matches(pred.copy(), gt.copy(), group_keys=KEYS, only_valids=True)
    cands["error"] = g12["host/cand_error"]
    matches = E.match_poses(cands, group_keys=KEYS)
    for k in ("cand_id", "pred_id", "gt_id"):
        assert np.array_equal(matches[k], g12[f"host/match_{k}"]), k
    assert len(set(matches["gt_id"])) == len(matches) == len(set(matches["pred_id"]))
    assert len(E.match_poses(cands.iloc[:0].copy(), group_keys=KEYS)) == 0


def test_compute_auc_posecnn(g12):
    for errors, ref in zip(g12["host/auc_errors"], g12["host/auc"]):
        assert abs(E.compute_auc_posecnn(errors) - ref) <= 1e-12
    assert np.isnan(g12["host/auc_none"]) and np.isnan(E.compute_auc_posecnn(np.full(5, 0.2)))
    assert np.isnan(E.compute_auc_posecnn(np.zeros(0)))


def test_average_precision_against_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rs = np.random.RandomState(0)
    for n in (1, 2, 7, 50, 400):
        y = rs.rand(n) < 0.4
        y[0] = True
        s = np.round(rs.rand(n), 1 if n > 7 else 3)  # one decimal: many tied scores
        assert abs(E.average_precision(y, s) - metrics.average_precision_score(y, s)) <= 1e-12, n
    assert E.average_precision([False, False], [0.3, 0.2]) == 0.0


# ---- the meter on a case worked out by hand ------------------------------------------------------------------------------------------
def shifted(T, dx):
    T = T.copy()
    T[0, 3] += dx
    return T


def hand_case():
    """One view.  ``mv_2``: ground truths A and B, 0.6 m apart; predictions p0 = A + 2 mm (score 0.9), p1 = A + 5 mm (0.8), p2 = B +
    0.3 d (0.7).  ``mv_3``: ground truth C, prediction p3 = C + 0.9 d (0.6).  ADD of a pure shift is the shift.  With
    match_threshold 0.5: p0 takes A (best score first), p1 finds A taken and stays unmatched, p2 takes B at 0.3 d (a match, but not
    within 0.1 d), p3 overlaps C's sphere (0.9 d < d) but misses the threshold."""
    from happypose_amd.mesh_store import MeshDataBase
    from happypose_amd.synthetic import make_multiview_objects

    db = MeshDataBase.from_object_ds(make_multiview_objects())
    d2, d3 = db.obj_dict["mv_2"].diameter_meters, db.obj_dict["mv_3"].diameter_meters
    A = np.eye(4)
    A[:3, 3] = (0.0, 0.0, 0.8)
    B, C = shifted(A, 0.6), shifted(A, -0.6)
    gt = (pd.DataFrame({"scene_id": 1, "view_id": 5, "label": ["mv_2", "mv_3", "mv_2"]}), np.stack([A, C, B]))
    pred = (pd.DataFrame({"scene_id": 1, "view_id": 5, "label": ["mv_2", "mv_3", "mv_2", "mv_2"], "score": [0.8, 0.6, 0.9, 0.7]}),
            np.stack([shifted(A, 0.005), shifted(C, 0.9 * d3), shifted(A, 0.002), shifted(B, 0.3 * d2)]))
    return db, d2, d3, gt, pred


def float64_device_call(meter):
    from happypose_amd.mesh_store import MeshDataBase  # noqa: F401

    host = meter.mesh_db
    names = {v: k for k, v in ops.POSE_ERR_MODES.items()}

    def call(modes, TXO_pred, TXO_gt, labels, K):
        n_pts = [host.infos[label]["n_points"] for label in host.labels]
        res = R.errors_batch([names[int(m)] for m in modes], TXO_pred.numpy(), TXO_gt.numpy(), host.ids_of(labels), np.asarray(host.points),
                             np.asarray(host.symmetries), host.n_sym, n_pts, None if K is None else K.numpy())
        return {k: torch.as_tensor(v) for k, v in res.items()}

    return call


HAND_K = np.array([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]], np.float32)


def run_hand_case(device_call=None, error_type="ADD", match_threshold=0.5, **kw):
    """The hand case through ``add`` and ``summary``; the ground truth carries ``K`` (read by MSPD only)."""
    from happypose_amd.tensor_collection import PandasTensorCollection

    db, d2, d3, gt, pred = hand_case()
    meter = E.PoseErrorMeter(db, error_type=error_type, match_threshold=match_threshold, report_AP=True, report_error_AUC=True,
                             report_error_stats=True, **kw)
    if device_call is not None:
        meter._device_errors = device_call(meter)
    dev = meter.mesh_db.points.device
    meter.add(PandasTensorCollection(pred[0], poses=torch.as_tensor(pred[1], dtype=torch.float32).to(dev)),
              PandasTensorCollection(gt[0], poses=torch.as_tensor(gt[1], dtype=torch.float32).to(dev),
                                     K=torch.as_tensor(np.tile(HAND_K, (len(gt[1]), 1, 1))).to(dev)))
    return meter.summary(), d2, d3


def check_hand_case(summary, dfs, d2, d3, tol):
    e0, e2 = 0.002, 0.3 * d2
    assert 0.1 * d2 < e2 < 0.1  # a match outside 0.1 d that still counts for the AUC (below 0.1 m)
    assert {k: summary[k] for k in ("n_gt", "n_gt_valid", "n_pred", "n_matched")} == {"n_gt": 3, "n_gt_valid": 3, "n_pred": 4, "n_matched": 2}
    assert summary["matched_gt_ratio"] == 2 / 3 and summary["pred_matched_ratio"] == 2.0 and summary["0.1d"] == 1 / 3
    matches = dfs["matches"].sort_values("pred_inst_id")
    # pred_inst_id numbers the mv_2 predictions in row order (0.8 -> 0, 0.9 -> 1, 0.7 -> 2); gt_inst_id: A -> 0, B -> 1
    assert matches["pred_inst_id"].tolist() == [1, 2] and matches["gt_inst_id"].tolist() == [0, 1]
    assert matches["label"].tolist() == ["mv_2", "mv_2"] and matches["0.1d"].tolist() == [True, False]
    assert np.allclose(matches["norm"], [e0, e2], rtol=0, atol=tol) and np.allclose(matches["score"], [0.9, 0.7])
    assert np.allclose(np.stack(list(matches["xyz"])), [[e0, 0, 0], [e2, 0, 0]], rtol=0, atol=tol)
    gt = dfs["gt"]
    assert gt["valid"].all() and np.isinf(gt["norm"][gt["label"] == "mv_3"]).all() and np.isnan(gt["score"][gt["label"] == "mv_3"]).all()
    assert dfs["preds"]["0.1d"].tolist() == [False, False, True, False]
    assert abs(summary["norm"] - (e0 + e2) / 2) <= tol and abs(summary["TCO_norm"] - (e0 + e2) / 2) <= 1e-6
    # AUC (PoseCNN): sorted errors e0 < e2 < inf, accuracy 1/3, 2/3: area up to 0.1 m, times 10
    auc_all = (e0 * (1 / 3) + (e2 - e0) * (2 / 3) + (0.1 - e2) * (2 / 3)) * 10
    auc_mv2 = (e0 * (1 / 2) + (e2 - e0) * 1.0 + (0.1 - e2) * 1.0) * 10
    assert abs(summary["AUC"] - auc_all) <= 10 * tol
    assert abs(dfs["gt"].attrs["AUC/objects"]["mv_2"] - auc_mv2) <= 10 * tol and np.isnan(dfs["gt"].attrs["AUC/objects"]["mv_3"])
    assert abs(summary["AUC/objects/mean"] - auc_mv2) <= 10 * tol  # the mean skips the object without a finite error, as xarray's does
    # AP at 0.1 d: mv_2 has one true positive, ranked first, of 2 ground truths: 1.0 * 1 / 2; mv_3 has none and is left out of the
    # mean; over all labels: 1.0 * 1 / 3
    assert summary["mAP"] == 0.5 and abs(summary["AP"] - 1 / 3) <= 1e-12
    assert set(dfs["ap"]) == {"mv_2", "all"} and dfs["ap"]["mv_2"]["n_tp"].tolist() == [1.0, 1.0, 1.0]


def test_meter_hand_case():
    (summary, dfs), d2, d3 = run_hand_case(float64_device_call, device="cpu")
    # the poses are float32: a translation below 0.8 m is rounded by up to 3e-8 (half an ulp), a difference of two by 6e-8
    check_hand_case(summary, dfs, d2, d3, tol=1e-7)


def test_meter_error_types_and_modes():
    db, *_ = hand_case()
    meter = E.PoseErrorMeter(db, error_type="add(-s)", device="cpu")
    assert meter._row_modes(["mv_0", "mv_1", "mv_2"]).tolist() == [1, 1, 0]  # mv_0 / mv_1 carry symmetries
    assert E.PoseErrorMeter(db, error_type="MSSD", device="cpu")._row_modes(["mv_0"]).tolist() == [3]
    with pytest.raises(ValueError):
        E.PoseErrorMeter(db, error_type="VSD", device="cpu")
    E.PoseErrorMeter(db, error_type="ADD-S", errors_bsz=64, device="cpu")  # exact meshes with any errors_bsz


def test_meter_hand_case_mspd():
    """MSPD through the meter: errors in pixels, compared with ``match_threshold`` itself (50 px here).  A shift of dx at depth
    0.8 m moves the projection by about 600 dx / 0.8 px: 1.5 px (p0), 3.75 px (p1), 38 px (p2, a match), 141 px (p3, none)."""
    (summary, dfs), d2, d3 = run_hand_case(float64_device_call, error_type="MSPD", match_threshold=50.0, device="cpu")
    assert summary["n_matched"] == 2 and summary["0.1d"] == 2 / 3  # for MSPD the flag is `error < match_threshold`
    matches = dfs["matches"].sort_values("pred_inst_id")
    assert matches["pred_inst_id"].tolist() == [1, 2] and matches["gt_inst_id"].tolist() == [0, 1]
    depth = 0.8 - 0.5 * d2  # no point of mv_2 is nearer to the camera than half a diameter in front of its centre
    for norm, dx in zip(matches["norm"], (0.002, 0.3 * d2)):
        assert 600 * dx / 0.8 < norm < 600 * dx / depth, (norm, dx)
    with pytest.raises(ValueError):
        E.PoseErrorMeter(hand_case()[0], error_type="MSPD", device="cpu").compute_errors(torch.eye(4)[None], torch.eye(4)[None], ["mv_2"])
