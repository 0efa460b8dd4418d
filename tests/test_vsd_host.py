"""Host-side tests of the visible-surface discrepancy: the float64 reference on hand cases, the argument checks of ``hp_vsd``
(no GPU is touched: every call returns before a launch), the proof that the inputs of tests/test_gpu_vsd.py stay clear of
the float32 decision boundaries, and the bookkeeping of ``VsdMeter`` on given errors."""

import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import vsd_ref as R  # noqa: E402

from happypose_amd import evaluation as E  # noqa: E402
from happypose_amd import ops  # noqa: E402


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_reference_hand_cases(name):
    inputs, counts, cost, errors = R.hand_cases()[name]
    ref = R.vsd_rows(**inputs)
    assert ref["counts"][0].tolist() == counts and ref["cost"][0].tolist() == cost
    assert np.allclose(ref["errors"][0], errors, rtol=0, atol=1e-15)
    assert ref["amb_counts"].sum() == 0 and ref["amb_cost"].sum() == 0


def test_argument_errors_without_gpu():
    from happypose_amd import _ffi

    lib = _ffi.lib()
    taus = (C.c_float * 16)(*([0.1] * 16))
    p = C.c_void_p(4096)  # never dereferenced: every call below returns before a launch

    def call(n_rows=1, ptrs=p, n_frames=1, n_layers=2, h=4, w=5, n_tau=2, taus=taus, norm=1, diameter=p, ws=p, ws_bytes=1 << 20):
        return lib.hp_vsd(n_rows, ptrs, ptrs, ptrs, diameter, ptrs, n_frames, ptrs, n_layers, ptrs, h, w, 0.015, n_tau, taus, norm, ptrs,
                          ptrs, ptrs, ws, ws_bytes, None)

    bad = [dict(n_rows=-1), dict(n_layers=-1), dict(n_frames=-2), dict(h=0), dict(w=-3), dict(h=65536, w=32768), dict(n_tau=0),
           dict(n_tau=17), dict(taus=None), dict(ptrs=None), dict(diameter=None), dict(ws=None), dict(ws_bytes=79),
           dict(h=46341, w=46341, n_rows=0)]
    for kw in bad:
        assert call(**kw) == -1 and b"hp_vsd" in lib.hp_last_error(), kw
    with pytest.raises(AssertionError):
        _ffi.check(call(n_tau=17), "hp_vsd")
    assert call(n_rows=0, ptrs=None, ws=None, ws_bytes=0) == 0  # nothing to do: no launch, no pointer looked at
    assert ops.VSD_MAX_TAUS == 16 and ops.VSD_COUNT_FIELDS == len(ops.VSD_COUNT_COLUMNS) == len(R.COUNT_COLUMNS) == 4
    # one record of (4 + 16) int32 per workgroup of 4096 pixels
    assert ops.vsd_workspace_bytes(1, 4, 5) == 80 and ops.vsd_workspace_bytes(3, 480, 640) == 3 * 75 * 80
    assert ops.vsd_workspace_bytes(0, 480, 640) == 0 and lib.hp_vsd_workspace_bytes(-1, 4, 5) == -1
    assert lib.hp_vsd_workspace_bytes(1, 65536, 32768) == -1


@pytest.mark.parametrize("name", R.SYNTHETIC)
def test_synthetic_inputs_have_no_ambiguous_pixel(name):
    """tests/test_gpu_vsd.py demands exact integer equality on these inputs: no comparison of theirs may be within the float32
    error bound of its threshold -- and they must exercise what they claim to."""
    case = R.synthetic_case(name)
    for norm in (True, False):
        ref = case["ref"][norm]
        assert ref["amb_counts"].sum() == 0 and ref["amb_cost"].sum() == 0, (name, norm)
    ref = case["ref"][True]
    counts, cost = ref["counts"], ref["cost"]
    if name == "odd":
        assert counts[5].tolist() == [0, 0, 0, 0] and (ref["errors"][5] == 1).all()          # both layers empty
        assert (ref["errors"][6] == 0).all() and counts[6, 0] == counts[6, 1] > 100          # the ground truth against itself
        assert counts[2, 2] == counts[2, 1] > 0                                              # wholly behind: visible only where rescued
        assert counts[4, 3] == 0 and counts[4, 2] > 0                                        # an empty ground truth
        assert (counts[:3, 3] == counts[0, 3]).all() and counts[0, 3] < (case["depth_layers"][0] > 0).sum()  # occluded in part
        assert ((case["depth_test"] == 0).sum(axis=(1, 2)) > 50).all()
    for norm in (True, False):
        c = case["ref"][norm]["cost"][min(1, len(cost) - 1)]  # the estimate that is off by centimetres and, in its lower half, decimetres
        assert c[0] > 0 and (len(c) == 1 or c[0] > c[-1])  # the taus see different pixels
    assert 0 < cost[0, 0] < counts[0, 1]


def test_rendered_inputs_stay_under_the_ambiguity_cap(golden_dir):
    """The rendered case of tests/test_gpu_vsd.py with the CPU rasteriser's depth maps (the kernel's are the same numbers): at
    most 0.5 % of a row's union may be ambiguous, which is what that test grants the kernel."""
    from happypose_amd.mesh_store import PackedMeshes
    from oracle import native

    s = R.rendered_scene()
    packed = PackedMeshes(R.rendered_dataset(golden_dir))
    T = np.concatenate([s["TXO_pred"], s["TXO_gt"]])
    obj = np.array([packed.label_to_id[label] for label in list(s["labels"]) + list(R.RENDER_LABELS)], np.int32)
    dep = native.rasterize(packed, obj, T, np.tile(s["K"], (len(T), 1, 1)), R.RENDER_RES, render_depth=True)["depths"][:, 0]
    n = len(s["TXO_pred"])
    test = R.rendered_test_depth(dep[n:])
    from happypose_amd.mesh_store import MeshDataBase

    infos = MeshDataBase.from_object_ds(R.rendered_dataset(golden_dir)).infos
    diameter = [infos[label]["diameter_m"] for label in s["labels"]]
    ref = R.vsd_rows(np.arange(n), n + s["gt_of"], np.zeros(n, int), diameter, test, dep, s["K"], R.DELTA, E.BOP_VSD_TAUS)
    n_u = ref["counts"][:, 0]
    assert (n_u > 300).all(), n_u
    assert (ref["amb_counts"].max(axis=1) <= 0.005 * n_u).all() and (ref["amb_cost"].max(axis=1) <= 0.005 * n_u).all(), (ref["amb_counts"], ref["amb_cost"])
    assert (ref["errors"][4:] == 0).all()                       # the perfect estimates
    assert (ref["errors"][[0, 2], -1] < ref["errors"][[1, 3], -1]).all()  # the small perturbations beat the large ones
    assert (ref["counts"][:, 3] < (dep[n + s["gt_of"]] > 0).sum(axis=(1, 2))).all()  # the occluder hides part of every ground truth


# ---- the meter on given errors ---------------------------------------------------------------------------------------------------
def _collection(labels, scores=None, view=5):
    from happypose_amd.tensor_collection import PandasTensorCollection

    infos = pd.DataFrame({"scene_id": 1, "view_id": view, "label": labels})
    if scores is not None:
        infos["score"] = scores
    poses = torch.eye(4).repeat(len(labels), 1, 1)
    poses[:, 0, 3] = torch.arange(len(labels), dtype=torch.float32)  # the row's own index: what the stub looks the errors up by
    return PandasTensorCollection(infos, poses=poses)


def _stub_meter(table, **kw):
    """A ``VsdMeter`` whose device call is replaced by a look-up in ``table [n_pred, n_gt, n_tau]``."""
    meter = E.VsdMeter(renderer=None, device="cpu", **kw)
    calls = []

    def compute_errors(TXO_pred, TXO_gt, labels, depth, K, frame_ids):
        calls.append((len(labels), np.asarray(frame_ids).tolist()))
        return table[TXO_pred[:, 0, 3].long().numpy(), TXO_gt[:, 0, 3].long().numpy()]

    meter.compute_errors = compute_errors
    return meter, calls


def test_meter_hand_case():
    """Two ground truths A, B of one label and three predictions.  tau 0: p0-A 0.2, p1-A 0.1, p1-B 0.5, everything else 0.9; tau 1:
    p0-A 0.4, p1-A 0.3, p1-B 0.7, else 1.  Below 0.3: tau 0 lets p0 (best score) take A and leaves p1 nothing: 1 of 2; tau 1 has
    no candidate (0.3 is not below 0.3).  Below 0.6: tau 0 matches p0-A and p1-B: 2 of 2; tau 1 p0-A only: 1 of 2."""
    table = np.full((3, 2, 2), 0.9)
    table[:, :, 1] = 1.0
    table[0, 0], table[1, 0], table[1, 1] = (0.2, 0.4), (0.1, 0.3), (0.5, 0.7)
    meter, calls = _stub_meter(table, taus=(0.1, 0.2), correct_ths=(0.3, 0.6))
    depth, K = torch.zeros(1, 4, 5), torch.eye(3)[None]
    meter.add(_collection(["x", "x", "x"], [0.9, 0.8, 0.7]), _collection(["x", "x"]), depth, K)
    summary, dfs = meter.summary()
    assert calls == [(6, [0] * 6)]
    rec = dfs["recall"]
    assert rec[["tau", "threshold"]].values.tolist() == [[0.1, 0.3], [0.1, 0.6], [0.2, 0.3], [0.2, 0.6]]
    assert rec["n_matched"].tolist() == [1, 2, 0, 1] and rec["recall"].tolist() == [0.5, 1.0, 0.0, 0.5]
    assert summary == {"n_gt_valid": 2, "n_cand": 6, "AR_VSD": 0.5}
    assert sorted(dfs["cands"]["vsd_0.1"].tolist()) == sorted(table[:, :, 0].reshape(-1).tolist())


def test_meter_bookkeeping():
    """Views are looked up in the frame table, predictions of views without ground truth are dropped, ``n_top`` keeps the best
    prediction of a group, ``add`` accumulates, an unknown label is refused."""
    table = np.zeros((4, 2, 1))
    table[1, 0] = 0.9  # view 7: the prediction with the higher score is the bad one
    meter, calls = _stub_meter(table, taus=(0.2,), correct_ths=(0.5,), n_top=1)
    from happypose_amd.tensor_collection import PandasTensorCollection

    pred = pd.DataFrame({"scene_id": 1, "view_id": [7, 7, 8, 9], "label": "x", "score": [0.2, 0.9, 0.5, 0.5]})
    gt = pd.DataFrame({"scene_id": 1, "view_id": [7, 8], "label": "x"})
    poses = lambda n: torch.eye(4).repeat(n, 1, 1) + torch.arange(n, dtype=torch.float32)[:, None, None] * torch.eye(4)[0][None, :, None] * torch.eye(4)[3][None, None, :]  # noqa: E731
    depth, K = torch.zeros(2, 4, 5), torch.eye(3).repeat(2, 1, 1)
    meter.add(PandasTensorCollection(pred, poses=poses(4)), PandasTensorCollection(gt, poses=poses(2)), depth, K, frames=[(1, 8), (1, 7)])
    assert calls == [(2, [1, 0])]  # (pred 1, gt 0) in view 7 = frame 1, (pred 2, gt 1) in view 8 = frame 0
    summary, dfs = meter.summary()
    assert summary["n_gt_valid"] == 2 and dfs["recall"]["n_matched"].tolist() == [1] and summary["AR_VSD"] == 0.5
    meter.add(_collection(["x"], [1.0], view=8), _collection(["x"], view=8), depth[:1], K[:1])
    assert meter.summary()[0] == {"n_gt_valid": 3, "n_cand": 3, "AR_VSD": 2 / 3}
    with pytest.raises(AssertionError):
        meter.add(_collection(["x"], [1.0]), _collection(["x"]), depth, K)  # two frames, one view

    class Db:
        infos = {"x": {}}

    strict, _ = _stub_meter(table, mesh_db=Db(), taus=(0.2,), correct_ths=(0.5,))
    with pytest.raises(AssertionError, match="not in mesh_db"):
        strict.add(_collection(["y"], [1.0]), _collection(["y"]), depth[:1], K[:1])


def test_bop_average_recall():
    assert E.bop_average_recall(0.5, 0.7, 0.9) == pytest.approx(0.7)
    assert E.BOP_VSD_TAUS == E.BOP_VSD_THRESHOLDS == (0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5) and E.BOP_VSD_DELTA == 0.015
