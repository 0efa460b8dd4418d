"""Host-side checks of the detection / segmentation scoring: the hand cases of tests/det_eval_ref.py, the row plan, the COCO
accumulation of the package against the reference, the thresholds, DetectionMeter's average precision against scikit-learn and
the box conversion of scene_ground_truth.  No GPU."""

import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import det_eval_ref as R  # noqa: E402


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_hand_cases_of_the_reference(name):
    case = R.HAND_CASES[name]
    got = R.coco_evaluate(case["preds"], case["gts"], "bbox")
    print(name, got)
    assert abs(got["AP"] - case["AP"]) < 1e-12 and abs(got["AR"] - case["AR"]) < 1e-12
    assert abs(got["AP50"] - case["AP"]) < 1e-12 and abs(got["AP75"] - case["AP"]) < 1e-12


def test_reference_matching_rules():
    thr = [0.5]
    # a tie goes to the later ground truth
    m, ig, g = R.coco_match([[0.75, 0.75]], [False, False], thr)
    assert m.tolist() == [[1]] and g.tolist() == [[-1, 0]]
    # an ignored ground truth is taken only when no other qualifies, and the detection is then ignored
    m, ig, _ = R.coco_match([[0.6, 0.9]], [False, True], thr)
    assert m.tolist() == [[0]] and ig.tolist() == [[False]]
    m, ig, _ = R.coco_match([[0.4, 0.9]], [False, True], thr)
    assert m.tolist() == [[1]] and ig.tolist() == [[True]]
    # a matched ground truth is not reused; IoU equal to the threshold matches; NaN never does
    m, _, _ = R.coco_match([[0.9], [0.8]], [False], thr)
    assert m.tolist() == [[0, -1]]
    assert R.coco_match([[0.5]], [False], thr)[0].tolist() == [[0]]
    assert R.coco_match([[np.nan]], [False], thr)[0].tolist() == [[-1]]


def _frames():
    pred = pd.DataFrame({"scene_id": [0, 0, 0, 0, 0, 1, 0], "view_id": [1, 1, 1, 1, 2, 0, 1], "label": ["a", "a", "a", "b", "a", "a", "a"],
                         "score": [0.5, 0.9, 0.5, 0.3, 0.2, 0.1, 0.9]})
    gt = pd.DataFrame({"scene_id": [0, 0, 0, 0, 0], "view_id": [1, 1, 1, 1, 3], "label": ["a", "a", "a", "b", "b"],
                       "ignore": [True, False, True, False, False]})
    return pred, gt


def test_plan_detection_rows():
    from happypose_amd.evaluation import plan_detection_rows

    pred, gt = _frames()
    plan = plan_detection_rows(pred, gt)
    g = plan["groups"]
    assert [tuple(r) for r in g[["scene_id", "view_id", "label"]].to_numpy()] == [(0, 1, "a"), (0, 1, "b"), (0, 2, "a"), (0, 3, "b"), (1, 0, "a")]
    assert g["n_det"].tolist() == [4, 1, 1, 0, 1] and g["n_gt"].tolist() == [3, 1, 0, 1, 0]  # frames without ground truth, groups without predictions
    assert g["row_off"].tolist() == [0, 12, 13, 13, 13] and g["det_off"].tolist() == [0, 4, 5, 6, 6] and g["gt_off"].tolist() == [0, 3, 4, 4, 5]
    # descending score, equal scores in row order (1 before 6, 0 before 2)
    assert plan["det_order"].tolist() == [1, 6, 0, 2, 3, 4, 5]
    # non-ignored first, each class in row order
    assert plan["gt_order"].tolist() == [1, 0, 2, 3, 4] and plan["gt_ignore"].tolist() == [False, True, True, False, False]
    assert plan["det_group"].tolist() == [0, 0, 0, 0, 1, 2, 4] and plan["gt_group"].tolist() == [0, 0, 0, 1, 3]
    assert plan["pred_idx"].tolist() == [1, 1, 1, 6, 6, 6, 0, 0, 0, 2, 2, 2, 3] and plan["gt_idx"].tolist() == [1, 0, 2] * 4 + [3]
    # the cap keeps the best, the stable order decides among equals
    capped = plan_detection_rows(pred, gt, max_dets=3)
    assert capped["det_order"].tolist() == [1, 6, 0, 3, 4, 5] and capped["groups"]["n_det"].tolist() == [3, 1, 1, 0, 1]
    assert capped["pred_idx"].tolist() == [1, 1, 1, 6, 6, 6, 0, 0, 0, 3]
    # no ignore column: nothing is ignored; empty frames
    assert not plan_detection_rows(pred, gt.drop(columns="ignore"))["gt_ignore"].any()
    empty = plan_detection_rows(pred.iloc[:0], gt.iloc[:0])
    assert len(empty["groups"]) == 0 and len(empty["pred_idx"]) == 0 and len(empty["det_order"]) == 0
    only_pred = plan_detection_rows(pred, gt.iloc[:0])
    assert only_pred["groups"]["n_gt"].sum() == 0 and len(only_pred["pred_idx"]) == 0 and len(only_pred["det_order"]) == len(pred)


@pytest.mark.parametrize("seed", range(6))
def test_coco_accumulate_against_the_reference(seed):
    from happypose_amd.evaluation import coco_accumulate

    rs = np.random.RandomState(seed)
    n_det, n_gt, T = rs.randint(0, 60), rs.randint(1, 30), len(R.COCO_IOU_THRESHOLDS)
    labels = ["a", "b", "c", "d"]
    det_label = rs.choice(labels, n_det).tolist()
    gt_label = rs.choice(labels[:3], n_gt).tolist()
    det_score = (rs.randint(0, 12, n_det) / 12.0).tolist()  # equal scores occur: the mergesort decides
    det_match = np.where(rs.rand(T, n_det) < 0.6, rs.randint(0, 5, (T, n_det)), -1)
    det_ignore = (rs.rand(T, n_det) < 0.15) & (det_match >= 0)
    gt_ignore = (rs.rand(n_gt) < 0.3).tolist()
    got, per_label = coco_accumulate(det_label, det_score, det_match, det_ignore, gt_label, gt_ignore)
    want = R.coco_accumulate(det_label, det_score, det_match, det_ignore, gt_label, gt_ignore)
    print(got, want)
    for k in ("AP", "AP50", "AP75", "AR"):
        assert abs(got[k] - want[k]) < 1e-12, k
    counted = {lab for lab, ig in zip(gt_label, gt_ignore) if not ig}
    assert set(per_label["label"]) == counted  # a label without a non-ignored ground truth is left out


def test_coco_accumulate_without_a_counted_label():
    from happypose_amd.evaluation import coco_accumulate

    got, per_label = coco_accumulate(["a"], [0.5], np.full((10, 1), -1), np.zeros((10, 1), bool), ["a"], [True])
    assert got == {"AP": -1.0, "AP50": -1.0, "AP75": -1.0, "AR": -1.0} and len(per_label) == 0
    assert got == R.coco_accumulate(["a"], [0.5], np.full((10, 1), -1), np.zeros((10, 1), bool), ["a"], [True])


def test_thresholds_are_capped_and_float32():
    from happypose_amd import evaluation, ops

    assert evaluation.COCO_IOU_THRESHOLDS == R.COCO_IOU_THRESHOLDS == (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95)
    got = ops.coco_thresholds(list(R.COCO_IOU_THRESHOLDS) + [1.0, 2.0])
    assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
    want = np.asarray([np.float32(min(t, 1 - 1e-10)) for t in list(R.COCO_IOU_THRESHOLDS) + [1.0, 2.0]], dtype=np.float32)
    assert np.array_equal(got, want) and np.array_equal(got, R.coco_thresholds(list(R.COCO_IOU_THRESHOLDS) + [1.0, 2.0]))
    assert got[0] == np.float32(0.5) and got[-1] == np.float32(1.0) == got[-2]  # 1 - 1e-10 rounds to 1 in float32


def test_detection_meter_summary_matches_scikit_learn():
    """DetectionMeter.summary from recorded frames (no device): its AP / mAP are scikit-learn's average_precision_score times
    the found fraction, as in the reference."""
    sklearn_metrics = pytest.importorskip("sklearn.metrics")
    from happypose_amd.evaluation import DetectionMeter

    rs = np.random.RandomState(3)
    n_pred, n_gt = 40, 25
    preds = pd.DataFrame({"scene_id": 0, "view_id": rs.randint(0, 4, n_pred), "label": rs.choice(["a", "b", "c"], n_pred),
                          "pred_inst_id": np.arange(n_pred), "score": rs.randint(0, 15, n_pred) / 15.0, "iou_valid": rs.rand(n_pred) < 0.4})
    preds.loc[preds["label"] == "c", "iou_valid"] = False  # a label without a true positive has no AP entry
    gt = pd.DataFrame({"scene_id": 0, "view_id": rs.randint(0, 4, n_gt), "label": rs.choice(["a", "b", "c"], n_gt), "gt_inst_id": np.arange(n_gt),
                       "valid": True, "iou_valid": rs.rand(n_gt) < 0.4})
    meter = DetectionMeter()
    meter.datas["gt_df"].append(gt)
    meter.datas["pred_df"].append(preds)
    meter.datas["matches_df"].append(preds[preds["iou_valid"]])
    summary, dfs = meter.summary()
    assert set(summary) == {"n_gt", "n_gt_valid", "n_pred", "n_matched", "matched_gt_ratio", "pred_matched_ratio", "iou_valid_recall", "AP", "mAP"}

    def ap(df, n):
        return sklearn_metrics.average_precision_score(df["iou_valid"], df["score"]) * df["iou_valid"].sum() / n

    n_gts = gt.groupby("label").size().to_dict()
    want = {label: ap(preds[preds["label"] == label], n_gts[label]) for label in ("a", "b")}
    assert set(dfs["ap"]) == {"a", "b", "all"}
    for label, value in want.items():
        assert abs(dfs["ap"][label]["AP"].iloc[0] - value) < 1e-12
    assert abs(summary["mAP"] - np.mean(list(want.values()))) < 1e-12
    assert abs(summary["AP"] - ap(preds, n_gt)) < 1e-12
    assert summary["n_gt_valid"] == n_gt and summary["iou_valid_recall"] == gt["iou_valid"].sum() / n_gt
    # the reference's own average precision agrees as well
    assert abs(R.average_precision(preds["iou_valid"].tolist(), preds["score"].tolist())
               - sklearn_metrics.average_precision_score(preds["iou_valid"], preds["score"])) < 1e-12


def test_bop_box_becomes_xyxy():
    """BOP's inclusive (x, y, w, h) covers the pixels x .. x + w - 1: the xyxy box of that area is (x, y, x + w, y + h), so a box
    one pixel wide has width 1 and two boxes that share no pixel have IoU 0."""
    from happypose_amd.evaluation import bop_box_to_xyxy

    got = bop_box_to_xyxy([(3, 5, 1, 1), (0, 0, 160, 120), (4, 5, 2, 7)])
    assert got.dtype == np.float32 and got.tolist() == [[3, 5, 4, 6], [0, 0, 160, 120], [4, 5, 6, 12]]
    assert R.box_iou(got[:1], got[2:])[0, 0] == 0.0  # pixel column 3 against columns 4 .. 5
    inclusive = np.array([7, 2, 11, 9])  # x_min, y_min, x_max, y_max as hp_scene_visibility reports them
    xywh = (inclusive[0], inclusive[1], inclusive[2] - inclusive[0] + 1, inclusive[3] - inclusive[1] + 1)
    assert bop_box_to_xyxy([xywh]).tolist() == [[7, 2, 12, 10]]
