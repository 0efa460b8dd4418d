"""GPU tests of the visible-surface discrepancy (csrc/vsd.hip, ``ops.vsd_tables``, ``evaluation.vsd``, ``VsdMeter``) against
the float64 restatement of tests/vsd_ref.py.

The synthetic inputs keep every comparison away from its threshold (tests/test_vsd_host.py proves it), so every integer the
kernel returns must EQUAL the reference.  On rendered depth maps a count may differ by at most the number of pixels the
reference itself calls ambiguous for that row and quantity."""

import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import vsd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _run(case, dev, norm=True, order=None):
    from happypose_amd import ops

    o = slice(None) if order is None else order
    out = ops.vsd_tables(case["est_layer"][o], case["gt_layer"][o], case["frame"][o], case["diameter"][o],
                         torch.as_tensor(case["depth_test"], device=dev), torch.as_tensor(case["depth_layers"], device=dev),
                         torch.as_tensor(case["K"]), case["delta"], case["taus"], norm)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _one_rounding(errors, counts, cost):
    """``errors`` is the float32 nearest to (c + n_U - n_I) / n_U (computed here in float64: the integers are exact), 1 where
    n_U == 0."""
    n_u = counts[:, :1].astype(np.float64)
    want = np.where(n_u > 0, (cost + n_u - counts[:, 1:2]) / np.maximum(n_u, 1), 1.0)
    return np.array_equal(errors, want.astype(np.float32))


def _assert_equal(got, ref):
    print("counts", got["counts"].tolist(), "cost", got["cost"].tolist())
    assert got["counts"].dtype == np.int32 and got["cost"].dtype == np.int32 and got["errors"].dtype == np.float32
    assert np.array_equal(got["counts"], ref["counts"]), (got["counts"] - ref["counts"]).tolist()
    assert np.array_equal(got["cost"], ref["cost"]), (got["cost"] - ref["cost"]).tolist()
    assert _one_rounding(got["errors"], got["counts"], got["cost"])


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_hand_cases(dev, name):
    inputs, counts, cost, errors = R.hand_cases()[name]
    got = _run(inputs, dev)
    assert got["counts"][0].tolist() == counts and got["cost"][0].tolist() == cost
    assert np.array_equal(got["errors"][0], np.asarray(errors, np.float64).astype(np.float32))


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("name", R.SYNTHETIC)
def test_synthetic_depth_maps(dev, name, norm):
    case = R.synthetic_case(name)
    _assert_equal(_run(case, dev, norm), case["ref"][norm])


def test_layers_as_the_rasteriser_returns_them(dev):
    """[L, 1, H, W] layers and a sliced (unaligned: 3015 floats per plane) view give the same table."""
    from happypose_amd import ops

    case = R.synthetic_case("odd")
    padded = torch.zeros((len(case["depth_layers"]) + 1, 1, 45, 67), device=dev)
    padded[1:, 0] = torch.as_tensor(case["depth_layers"], device=dev)
    out = ops.vsd_tables(case["est_layer"], case["gt_layer"], case["frame"], case["diameter"], torch.as_tensor(case["depth_test"], device=dev),
                         padded[1:], torch.as_tensor(case["K"]), case["delta"], case["taus"])
    _assert_equal({k: v.cpu().numpy() for k, v in out.items()}, case["ref"][True])


@pytest.mark.parametrize("name", ["odd", "vga"])
def test_determinism(dev, name):
    case = R.synthetic_case(name)
    a, b = _run(case, dev), _run(case, dev)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    rev = np.arange(len(case["est_layer"]))[::-1].copy()
    c = _run(case, dev, order=rev)
    for k in a:
        assert np.array_equal(a[k][rev], c[k]), k


def test_wrapper_rejects_ids_outside_their_tables(dev):
    from happypose_amd import ops

    case = R.synthetic_case("square")
    for column, bad in (("est_layer", 4), ("gt_layer", -1), ("frame", 1)):
        broken = dict(case)
        broken[column] = case[column].copy()
        broken[column][1] = bad
        with pytest.raises(AssertionError, match=column):
            _run(broken, dev)
    with pytest.raises(AssertionError):
        _run(dict(case, taus=tuple(range(1, 18))), dev)
    out = ops.vsd_tables(case["est_layer"][:0], case["gt_layer"][:0], case["frame"][:0], case["diameter"][:0],
                         torch.as_tensor(case["depth_test"], device=dev), torch.as_tensor(case["depth_layers"], device=dev),
                         torch.as_tensor(case["K"]), case["delta"], case["taus"])
    assert out["errors"].shape == (0, 1) and out["counts"].shape == (0, 4)


# ---- rendered ---------------------------------------------------------------------------------------------------------------------
_RENDERED = {}


def _rendered(dev, golden_dir):
    """The scene of vsd_ref.rendered_scene through ``evaluation.vsd``, the layers it rendered and the reference on those layers."""
    if not _RENDERED:
        from happypose_amd import evaluation as E
        from happypose_amd import ops

        s = R.rendered_scene()
        store = ops.MeshStore(R.rendered_dataset(golden_dir), dev)
        K = torch.as_tensor(s["K"])
        _, _, gt_dep, _ = ops.rasterize(store, store.ids_of(list(R.RENDER_LABELS)), torch.as_tensor(s["TXO_gt"]), K.expand(2, 3, 3),
                                        R.RENDER_RES, render_depth=True, render_rgb=False)
        depth = torch.as_tensor(R.rendered_test_depth(gt_dep.cpu().numpy()), device=dev)
        pred, gt = torch.as_tensor(s["TXO_pred"]), torch.as_tensor(s["TXO_gt"][s["gt_of"]])
        errors, det = E.vsd(pred, gt, s["labels"], depth, K, store, return_details=True)
        diameter = [store.mesh_db.infos[label]["diameter_m"] for label in s["labels"]]
        ref = R.vsd_rows(det["est_layer"], det["gt_layer"], det["frame"], diameter, depth.cpu().numpy(), det["depth_layers"].cpu().numpy(),
                         s["K"], E.BOP_VSD_DELTA, E.BOP_VSD_TAUS)
        _RENDERED.update(s=s, store=store, depth=depth, K=K, pred=pred, gt=gt, errors=errors.cpu().numpy(), det=det, ref=ref, gt_dep=gt_dep)
    return _RENDERED


def test_rendered(dev, golden_dir):
    from happypose_amd import evaluation as E

    r = _rendered(dev, golden_dir)
    det, ref, s = r["det"], r["ref"], r["s"]
    # 4 estimate renders and 2 ground-truth renders: the perfect estimates ARE the ground-truth layers, rendered once
    assert det["depth_layers"].shape == (6, *R.RENDER_RES)
    est_l, gt_l = det["est_layer"], det["gt_layer"]
    assert len(set(est_l.tolist())) == 6 and gt_l[[0, 1, 4]].tolist() == [est_l[4]] * 3 and gt_l[[2, 3, 5]].tolist() == [est_l[5]] * 3
    assert torch.equal(det["depth_layers"][[int(est_l[4]), int(est_l[5])]], r["gt_dep"][:, 0])
    counts, cost = det["counts"].cpu().numpy(), det["cost"].cpu().numpy()
    print("counts", counts.tolist(), "\nref   ", ref["counts"].tolist(), "\nambiguous", ref["amb_counts"][:, 0].tolist(), ref["amb_cost"].tolist())
    assert (ref["counts"][:, 0] > 300).all()
    assert (np.abs(counts - ref["counts"]) <= ref["amb_counts"]).all()
    assert (np.abs(cost - ref["cost"]) <= ref["amb_cost"]).all()
    assert _one_rounding(r["errors"], counts, cost)
    assert (r["errors"][4:] == 0).all()  # perfect estimates
    assert (r["errors"][:4] > 0).any(axis=1).all()
    # a budget of two layers at a time: several chunks (a shared ground truth is rendered once in each), the same numbers
    small = E.vsd(r["pred"], r["gt"], s["labels"], r["depth"], r["K"], r["store"], layer_budget_bytes=1)
    assert np.array_equal(small.cpu().numpy(), r["errors"])


def test_meter(dev, golden_dir):
    """``VsdMeter`` on the rendered scene against the same meter fed the reference's errors.  The two can only part where a
    reference error is within the row's ambiguous share of a correctness threshold: asserted not to happen here."""
    from happypose_amd import evaluation as E
    from happypose_amd.tensor_collection import PandasTensorCollection

    r = _rendered(dev, golden_dir)
    s, ref = r["s"], r["ref"]
    slack = (ref["amb_cost"].max(axis=1) + ref["amb_counts"][:, 0]) / ref["counts"][:, 0]
    ths = np.asarray(E.BOP_VSD_THRESHOLDS)
    assert (np.abs(ref["errors"][:, :, None] - ths[None, None, :]) > 2 * slack[:, None, None]).all()

    def collections():
        pred = pd.DataFrame({"scene_id": 3, "view_id": 11, "label": s["labels"], "score": s["scores"]})
        gt = pd.DataFrame({"scene_id": 3, "view_id": 11, "label": list(R.RENDER_LABELS)})
        return PandasTensorCollection(pred, poses=r["pred"].clone()), PandasTensorCollection(gt, poses=torch.as_tensor(s["TXO_gt"]))

    meter = E.VsdMeter(r["store"], r["store"].mesh_db, device=dev)
    meter.add(*collections(), r["depth"], r["K"])
    summary, dfs = meter.summary()

    by_pose = {r["pred"][i].numpy().tobytes(): i for i in range(len(r["pred"]))}
    stub = E.VsdMeter(None, device="cpu")
    stub.compute_errors = lambda TXO_pred, TXO_gt, labels, depth, K, frame_ids: ref["errors"][[by_pose[T.cpu().numpy().tobytes()] for T in TXO_pred]]
    stub.add(*collections(), r["depth"], r["K"])
    want, want_dfs = stub.summary()
    print(summary, "\n", dfs["recall"])
    assert summary["n_gt_valid"] == 2 and summary["n_cand"] == 6
    assert dfs["recall"]["n_matched"].tolist() == want_dfs["recall"]["n_matched"].tolist()
    assert summary["AR_VSD"] == want["AR_VSD"] and 0 < summary["AR_VSD"] <= 1
