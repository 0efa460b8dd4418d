"""The pose-error kernels (csrc/pose_errors.hip) and happypose_amd.evaluation on the device, against the float64 restatement
(tests/pose_errors_ref.py) and the reference's own run (tests/golden/g12_pose_errors.npz).  Bounds: 4 x the reference's measured
float32 error per quantity (tests/test_pose_errors_reference.py measures them; table in DESIGN.md section 2).  The clouds and poses
of every test are G12's (or cut from them), so the measured bounds apply to the shapes used here."""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pose_errors_ref as R  # noqa: E402
import test_pose_errors_host as H  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLOATS = ("norm_avg", "xyz_avg", "norm_max", "TCO_xyz", "TCO_norm")


@pytest.fixture(scope="module")
def g12(golden_dir):
    return np.load(golden_dir / "g12_pose_errors.npz")


@pytest.fixture(scope="module")
def B(g12):
    return R.bounds(g12)


def launch(modes, pred_id, gt_id, obj_id, poses_pred, poses_gt, points, symmetries, n_sym, n_pts, K=None, assign=True):
    from happypose_amd import ops

    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)  # noqa: E731
    mode_ids = np.asarray([ops.POSE_ERR_MODES[m] if isinstance(m, str) else m for m in modes], np.int32)
    # index columns go up as device tensors: the wrapper range-checks host ids itself, the kernels' guards are what is tested here
    pred_id, gt_id, obj_id, mode_ids = (t(np.asarray(a, np.int32), torch.int32) for a in (pred_id, gt_id, obj_id, mode_ids))
    out = ops.pose_errors_tables(pred_id, gt_id, obj_id, mode_ids,
                                 t(poses_pred, torch.float32), t(poses_gt, torch.float32), t(points, torch.float32),
                                 t(symmetries, torch.float32), t(n_sym, torch.int32), t(n_pts, torch.int32),
                                 K=None if K is None else t(K, torch.float32), return_assign=assign)
    return {k: v.cpu().numpy() for k, v in out.items()}


def one_object(cloud):
    return cloud[None], np.eye(4, dtype=np.float32)[None, None], np.ones(1, np.int32), np.array([len(cloud)], np.int32)


def check_row(out, r, ref, b, pixels=False):
    """A kernel row against a float64 result for the SAME neighbours / symmetry."""
    scale = b["pixel"] if pixels else None
    # rows of fewer DISTINCT terms than the measurement had (padding repeats them): the per-point bound
    m = R.mean_bounds(b, len(np.unique(ref["dists"], axis=0)))
    assert abs(out["norm_avg"][r] - ref["norm_avg"]) <= (scale or m["norm_avg"]), (r, out["norm_avg"][r], ref["norm_avg"])
    assert np.abs(out["xyz_avg"][r] - ref["xyz_avg"]).max() <= (scale or m["xyz_avg"]), (r, out["xyz_avg"][r], ref["xyz_avg"])
    assert abs(out["norm_max"][r] - ref["norm_max"]) <= (scale or b["norm_max"]), (r, out["norm_max"][r], ref["norm_max"])


def check_adds_row(out, r, T_pred, T_gt, pts, b):
    """Checks 1 and 2 of the nearest-neighbour choice; every point counts."""
    n = len(pts)
    assign = out["assign"][r][:n]
    assert assign.min() >= 0 and assign.max() < n and (out["assign"][r][n:] == -1).all()
    _, best2 = R.nearest(T_pred, T_gt, pts)
    d = R.neighbour_distance(T_pred, T_gt, pts, assign)
    assert (d <= np.sqrt(best2) + b["point"]).all(), (r, (d - np.sqrt(best2)).max())          # 1
    check_row(out, r, R.add_s(T_pred, T_gt, pts, assign=assign), b)                           # 2, own neighbours
    assert abs(out["norm_avg"][r] - R.add_s(T_pred, T_gt, pts)["norm_avg"]) <= R.mean_bounds(b, len(np.unique(pts, axis=0)))["norm_avg"] + b["point"], r  # 2, pure float64
    assert out["sym_id"][r] == -1


def test_add_and_adds_against_float64_and_golden(g12, B):
    for cloud in ("small", "large"):
        pred, gt, pts = R.golden_rows(g12, cloud)
        n = len(pred)
        ids = np.arange(n)
        out = launch(["ADD"] * n + ["ADD-S"] * n, np.r_[ids, ids], np.r_[ids, ids], np.zeros(2 * n), pred, gt, *one_object(pts))
        for r in range(n):
            check_row(out, r, R.add(pred[r], gt[r], pts), B)
            assert (out["assign"][r] == np.arange(len(pts))).all() and out["sym_id"][r] == -1
            check_adds_row(out, n + r, pred[r], gt[r], pts, B)
            for k in ("norm_avg", "xyz_avg", "norm_max"):
                assert np.abs(out[k][r] - g12[f"{cloud}/add_{k}"][r]).max() <= B[k], (cloud, k, r)
            assert abs(out["norm_avg"][n + r] - g12[f"{cloud}/adds_norm_avg"][r]) <= B["norm_avg"] + B["point"], (cloud, r)
            if cloud == "small" and (out["assign"][n + r] == g12["small/adds_assign"][r]).all():
                for k in ("norm_avg", "xyz_avg", "norm_max"):
                    assert np.abs(out[k][n + r] - g12[f"small/adds_{k}"][r]).max() <= B[k], (k, r)
        assert np.abs(out["TCO_xyz"][:n] - np.abs(pred[:, :3, 3] - gt[:, :3, 3])).max() <= 1e-7  # one float32 subtraction each
        assert np.abs(out["TCO_norm"][:n] - np.linalg.norm(pred[:, :3, 3].astype(np.float64) - gt[:, :3, 3], axis=-1)).max() <= B["norm_avg"]


def test_symmetric_modes_against_float64_and_golden(g12, B):
    obj, pred, gt = g12["sym/obj_id"], g12["sym/TXO_pred"], g12["sym/TXO_gt"]
    n = len(obj)
    ids = np.arange(n)
    K = np.tile(g12["K"], (3 * n, 1, 1))
    out = launch(["ADD-SYM"] * n + ["MSSD"] * n + ["MSPD"] * n, np.tile(ids, 3), np.tile(ids, 3), np.tile(obj, 3), pred, gt,
                 g12["sym/points"], g12["sym/symmetries"], g12["sym/n_sym"], g12["sym/n_points"], K=K)
    for r, o in enumerate(obj):
        pts, syms = g12["sym/points"][o][:g12["sym/n_points"][o]], g12["sym/symmetries"][o][:g12["sym/n_sym"][o]]
        for k, (mode, fn) in enumerate((("ADD-SYM", R.add_sym), ("MSSD", R.mssd))):
            ref = fn(pred[r], gt[r], pts, syms)
            assert out["sym_id"][k * n + r] == ref["sym_id"], (mode, r)
            check_row(out, k * n + r, ref, B)
        ref = R.mspd(pred[r], gt[r], pts, syms, g12["K"])
        assert out["sym_id"][2 * n + r] == ref["sym_id"], r
        check_row(out, 2 * n + r, ref, B, pixels=True)
        assert out["sym_id"][r] == g12["sym/sym_id"][r]
        for k in ("norm_avg", "xyz_avg", "norm_max"):
            assert np.abs(out[k][r] - g12[f"sym/{k}"][r]).max() <= B[k], (k, r)


def test_per_point_dists_from_the_device(g12, B):
    """Check 3, and the SIGN of what the public functions return: ``evaluation.dists_add_symmetric`` on the device, per point and per
    component, against the float64 differences for the kernel's own neighbours on every row and, on the rows where those neighbours
    are the reference's, against the reference's stored ``dists``."""
    from happypose_amd import evaluation as E

    pred, gt, pts = R.golden_rows(g12, "small")
    n = len(pred)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)  # noqa: E731
    dists = E.dists_add_symmetric(t(pred), t(gt), t(np.tile(pts, (n, 1, 1)))).cpu().numpy().astype(np.float64)
    ids = np.arange(n)
    assign = launch(["ADD-S"] * n, ids, ids, np.zeros(n), pred, gt, *one_object(pts))["assign"]  # the same kernel, the same bits
    same = 0
    for r in range(n):
        ref = R.add_s(pred[r], gt[r], pts, assign=assign[r])["dists"]
        assert np.linalg.norm(dists[r] - ref, axis=-1).max() <= B["point"], r
        if (assign[r] == g12["small/adds_assign"][r]).all():
            same += 1
            assert np.linalg.norm(dists[r] - g12["small/adds_dists"][r], axis=-1).max() <= B["point"], r
    print("rows whose neighbours are the reference's:", same, "of", n)
    assert same >= 1  # otherwise the comparison with the stored dists says nothing
    assert np.abs(dists[:-1]).max() > 1e3 * B["point"]  # signed values far from zero are compared: a swapped sign cannot pass


def size_table(g12):
    """Objects that are the first n points of G12's large cloud, for every n at which the kernels take another path."""
    from happypose_amd import ops

    tile, block = ops.POSE_ERR_PRED_TILE, ops.POSE_ERR_GT_BLOCK
    sizes = sorted({1, 63, 64, 65, tile - 1, tile, tile + 1, block - 1, block, block + 1})
    cloud = g12["cloud_large"][:max(sizes)]
    assert len(cloud) == max(sizes)
    points = np.stack([np.concatenate([cloud[:n], cloud[np.arange(max(sizes) - n) % n]]) for n in sizes])  # padding repeats vertices
    return sizes, points


@pytest.mark.parametrize("exact", [True, False])
def test_point_counts_around_tile_and_block(g12, B, exact):
    sizes, points = size_table(g12)
    n_obj = len(sizes)
    n_pts = np.asarray(sizes if exact else [points.shape[1]] * n_obj, np.int32)
    pred, gt = g12["large/TXO_pred"], g12["large/TXO_gt"]
    rows = np.arange(n_obj)
    pose = rows % (len(pred) - 1)
    out = launch(["ADD-S"] * n_obj + ["ADD"] * n_obj, np.r_[pose, pose], np.r_[pose, pose], np.r_[rows, rows], pred, gt, points,
                 np.eye(4, dtype=np.float32)[None, None].repeat(n_obj, 0), np.ones(n_obj, np.int32), n_pts)
    for o in range(n_obj):
        pts = points[o][:n_pts[o]]
        check_adds_row(out, o, pred[pose[o]], gt[pose[o]], pts, B)
        check_row(out, n_obj + o, R.add(pred[pose[o]], gt[pose[o]], pts), B)
        assert (out["assign"][n_obj + o][:n_pts[o]] == np.arange(n_pts[o])).all() and (out["assign"][n_obj + o][n_pts[o]:] == -1).all()


def mixed_launch(g12, rows=None):
    obj, pred, gt = g12["sym/obj_id"], g12["sym/TXO_pred"], g12["sym/TXO_gt"]
    n = 37
    modes = [R.MODES[i % 5] for i in range(n)]
    ids = np.arange(n) % len(obj)
    K = np.tile(g12["K"], (n, 1, 1))
    K[:, 0, 2] += np.arange(n)  # a K of its own for every row
    sel = np.arange(n) if rows is None else np.asarray(rows)
    out = launch([modes[i] for i in sel], ids[sel], ids[sel], obj[ids[sel]], pred, gt, g12["sym/points"], g12["sym/symmetries"],
                 g12["sym/n_sym"], g12["sym/n_points"], K=K[sel])
    return modes, out


def test_bit_identical_alone_mixed_and_again(g12):
    modes, full = mixed_launch(g12)
    _, again = mixed_launch(g12)
    for k in full:
        assert full[k].tobytes() == again[k].tobytes(), k
    for mode in R.MODES:  # one mode at a time
        rows = [i for i, m in enumerate(modes) if m == mode]
        _, part = mixed_launch(g12, rows)
        for k in full:
            assert full[k][rows].tobytes() == part[k].tobytes(), (mode, k)
    for r in (0, 1, 17, 36):  # a row alone
        _, one = mixed_launch(g12, [r])
        for k in full:
            assert full[k][r:r + 1].tobytes() == one[k].tobytes(), (r, k)


def test_large_rows_bit_identical_alone_and_together(g12):
    """ADD-S rows of more than one block: the partial sums do not depend on the rows around them."""
    pred, gt, pts = R.golden_rows(g12, "large")
    ids = np.arange(len(pred))
    full = launch(["ADD-S"] * len(pred), ids, ids, np.zeros(len(pred)), pred, gt, *one_object(pts))
    one = launch(["ADD-S"], [3], [3], [0], pred, gt, *one_object(pts))
    for k in full:
        assert full[k][3:4].tobytes() == one[k].tobytes(), k


def test_pred_equal_gt_is_exactly_zero(g12):
    for cloud in ("small", "large"):
        pred, gt, pts = R.golden_rows(g12, cloud)
        assert np.array_equal(pred[-1], gt[-1])
        out = launch(["ADD", "ADD-S"], [5, 5], [5, 5], [0, 0], pred, gt, *one_object(pts))
        for k in FLOATS:
            assert (out[k] == 0).all(), (cloud, k)
        assert (out["assign"][1] == np.arange(len(pts))).all()


def test_exact_ties_take_the_lower_index(g12, B):
    pts = g12["cloud_small"][:300]
    doubled = np.concatenate([pts, pts])[np.r_[np.arange(0, 600, 2), np.arange(1, 600, 2)]]  # every point twice, interleaved order
    first = {}
    for i, p in enumerate(map(bytes, doubled)):
        first.setdefault(p, i)
    pred, gt = g12["small/TXO_pred"], g12["small/TXO_gt"]
    out = launch(["ADD-S"] * 2, [0, 5], [0, 5], [0, 0], pred, gt, *one_object(doubled))
    lowest = np.asarray([first[bytes(p)] for p in doubled])
    for r in range(2):
        assert (lowest[out["assign"][r]] == out["assign"][r]).all()  # never the higher index of a duplicate pair
    check_adds_row(out, 0, pred[0], gt[0], doubled, B)


def test_guarded_rows_are_nan_and_neighbours_correct(g12, B):
    obj, pred, gt = g12["sym/obj_id"], g12["sym/TXO_pred"], g12["sym/TXO_gt"]
    n_sym, n_pts = g12["sym/n_sym"].copy(), g12["sym/n_points"].copy()
    n_sym[4], n_pts[5] = g12["sym/symmetries"].shape[1] + 1, g12["sym/points"].shape[1] + 1  # objects 4 and 5 are broken
    rows = [  # (mode, pred, gt, obj, guarded)
        ("ADD", 0, 0, 0, False), ("ADD", 99, 0, 0, True), ("ADD-S", 1, 1, 0, False), ("ADD-S", 0, -1, 0, True),
        ("ADD-SYM", 2, 2, 1, False), ("ADD-SYM", 2, 2, 6, True), ("MSSD", 3, 3, 1, False), (7, 3, 3, 1, True),
        ("ADD", 4, 4, 4, True), ("ADD-S", 4, 4, 5, True), ("ADD-S", 4, 4, 2, False), ("MSPD", 4, 4, 2, True)]  # MSPD without K
    modes, p, g, o, guarded = zip(*rows)
    out = launch(modes, p, g, o, pred, gt, g12["sym/points"], g12["sym/symmetries"], n_sym, n_pts)
    for r, (mode, pi, gi, oi, bad) in enumerate(rows):
        if bad:
            assert all(np.isnan(out[k][r]).all() for k in FLOATS), r
            assert out["sym_id"][r] == -1 and (out["assign"][r] == -1).all(), r
        else:
            pts = g12["sym/points"][oi][:g12["sym/n_points"][oi]]
            ref = R.row(mode, pred[pi], gt[gi], pts, g12["sym/symmetries"][oi][:g12["sym/n_sym"][oi]])
            if mode == "ADD-S":
                check_adds_row(out, r, pred[pi], gt[gi], pts, B)
            else:
                check_row(out, r, ref, B)
                assert out["sym_id"][r] == ref["sym_id"]


def test_no_rows_and_workspace_size():
    from happypose_amd import _ffi, ops

    lib = _ffi.lib()
    rc = lib.hp_pose_errors(0, None, None, None, None, -1, None, 0, None, 0, None, None, None, None, None,
                            0, 0, 0, None, None, None, None, None, None, None, None, 0, None)
    assert rc == 0  # nothing is looked at, nothing is launched
    empty = np.zeros(0, np.int32)
    out = launch([], empty, empty, empty, np.zeros((0, 4, 4)), np.zeros((0, 4, 4)), *one_object(np.zeros((4, 3), np.float32)))
    assert out["norm_avg"].shape == (0,) and out["xyz_avg"].shape == (0, 3) and out["assign"].shape == (0, 4)
    size = ops.pose_errors_workspace_bytes(64, 20000)
    blocks = -(-20000 // ops.POSE_ERR_GT_BLOCK)
    assert 0 < size < 1 << 20 and size == 64 * blocks * 32  # rows x blocks x a few dozen bytes; a P^2 one would be 100 GB
    assert ops.pose_errors_workspace_bytes(64, 40000) <= 2 * size + 64 * 32


def test_dists_functions_shape_and_memory(g12, B):
    from happypose_amd import evaluation as E

    pred, gt, pts = R.golden_rows(g12, "large")
    n = 8
    cloud = np.concatenate([pts, pts[:2000 - len(pts)] + np.float32(1e-3)])  # 2 000 distinct points
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)  # noqa: E731
    TXO_pred, TXO_gt, points = t(pred[np.arange(n) % 5]), t(gt[np.arange(n) % 5]), t(np.tile(cloud, (n, 1, 1)))
    E.dists_add_symmetric(TXO_pred[:1], TXO_gt[:1], points[:1])  # library and allocator warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dists = E.dists_add_symmetric(TXO_pred, TXO_gt, points)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert dists.shape == (n, 2000, 3) and dists.dtype == torch.float32
    assert grown < n * 2000 * 64, grown  # a [b, P, P] float temporary alone would be 128 MB
    d = dists.cpu().numpy().astype(np.float64)
    for r in range(n):
        ref = R.add_s(pred[r % 5], gt[r % 5], cloud)
        assert abs(np.linalg.norm(d[r], axis=-1).mean() - ref["norm_avg"]) <= B["norm_avg"] + B["point"], r
    add = E.dists_add(TXO_pred, TXO_gt, points).cpu().numpy()
    assert add.shape == (n, 2000, 3)
    assert np.linalg.norm(add[0] - R.add(pred[0], gt[0], cloud)["dists"], axis=-1).max() <= B["point"]


def test_evaluation_functions_on_a_mesh_db(g12, B):
    from happypose_amd import evaluation as E
    from happypose_amd.mesh_store import MeshDataBase
    from happypose_amd.synthetic import make_multiview_objects

    mesh_db = MeshDataBase.from_object_ds(make_multiview_objects()).batched(n_sym=64).to(DEV)
    assert np.array_equal(mesh_db.points.cpu().numpy(), g12["sym/points"])
    obj, pred, gt = g12["sym/obj_id"], g12["sym/TXO_pred"], g12["sym/TXO_gt"]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)  # noqa: E731
    labels = mesh_db.labels[obj]
    chamfer, none = E.chamfer_dist(t(gt), t(pred), labels, mesh_db)
    assert none is None and np.abs(chamfer.cpu().numpy() - g12["sym/chamfer"]).max() <= B["norm_avg"] + B["point"]
    n = len(obj)
    syms, pts = t(g12["sym/symmetries"])[obj.tolist()], t(g12["sym/points"])[obj.tolist()]
    dists = E.dists_add_symmetries(t(pred), t(gt)[:, None] @ syms, pts)  # all 64 table rows: the rows past n_sym are identity
    assert dists.shape == (n, pts.shape[1], 3)
    for r, o in enumerate(obj):
        got = dists[r].cpu().numpy().astype(np.float64)
        assert abs(np.linalg.norm(got, axis=-1).mean() - g12["sym/norm_avg"][r]) <= B["norm_avg"] + B["point"], r
        ref = R.add_sym(pred[r], gt[r], g12["sym/points"][o], g12["sym/symmetries"][o][:g12["sym/n_sym"][o]])
        assert np.linalg.norm(got - ref["dists"], axis=-1).max() <= B["point"], r  # per point, with sign
    K = t(np.tile(g12["K"], (n, 1, 1)))
    got_s, got_p = E.mssd(t(pred), t(gt), labels, mesh_db).cpu().numpy(), E.mspd(t(pred), t(gt), K, labels, mesh_db).cpu().numpy()
    for r, o in enumerate(obj):
        p, s = g12["sym/points"][o][:g12["sym/n_points"][o]], g12["sym/symmetries"][o][:g12["sym/n_sym"][o]]
        assert abs(got_s[r] - R.mssd(pred[r], gt[r], p, s)["norm_max"]) <= B["norm_max"], r
        assert abs(got_p[r] - R.mspd(pred[r], gt[r], p, s, g12["K"])["norm_max"]) <= B["pixel"], r


def test_meter_on_the_device_matches_the_float64_run(B):
    (host_summary, host_dfs), d2, d3 = H.run_hand_case(H.float64_device_call, device="cpu")
    (summary, dfs), _, _ = H.run_hand_case(device=DEV)
    # no decision of the case lies within the bound of its threshold: the errors THE DEVICE computes for every pair of one label
    # (the candidates before the sphere check) against match_threshold x d and 0.1 d
    from happypose_amd import evaluation as E

    db, _, _, gt, pred = H.hand_case()
    pairs = [(p, g) for p in range(len(pred[0])) for g in range(len(gt[0])) if pred[0]["label"][p] == gt[0]["label"][g]]
    assert len(pairs) == 7
    t = lambda a: torch.as_tensor(a, dtype=torch.float32).to(DEV)  # noqa: E731
    labels = np.asarray([pred[0]["label"][p] for p, _ in pairs])
    device_errors = E.PoseErrorMeter(db, error_type="ADD", device=DEV).compute_errors(
        t(pred[1][[p for p, _ in pairs]]), t(gt[1][[g for _, g in pairs]]), labels)["norm_avg"].cpu().numpy()
    for e, label in zip(device_errors, labels):
        d = d2 if label == "mv_2" else d3
        assert min(abs(e - 0.5 * d), abs(e - 0.1 * d)) > 100 * B["norm_avg"], (e, label)
    assert np.sort(dfs["matches"]["norm"].to_numpy()).tolist() == np.sort(device_errors)[[0, 2]].tolist()  # p0-A and p2-B
    H.check_hand_case(summary, dfs, d2, d3, tol=1e-7 + B["norm_avg"])
    for k in ("gt", "matches", "preds"):
        a, b = dfs[k], host_dfs[k]
        assert list(a.columns) == list(b.columns) and len(a) == len(b)
        for col in ("scene_id", "view_id", "label", "pred_inst_id", "gt_inst_id", "cand_id", "valid", "0.1d"):
            if col in a:
                assert a[col].equals(b[col]), (k, col)
    for k, v in host_summary.items():
        assert np.allclose(summary[k], v, rtol=0, atol=10 * B["norm_avg"], equal_nan=True), k


def test_meter_mspd_on_the_device_matches_the_float64_run(B):
    kw = dict(error_type="MSPD", match_threshold=50.0)
    (host_summary, host_dfs), _, _ = H.run_hand_case(H.float64_device_call, device="cpu", **kw)
    (summary, dfs), _, _ = H.run_hand_case(device=DEV, **kw)
    norms = dfs["matches"]["norm"].to_numpy()
    assert len(norms) == 2 and (np.abs(norms - 50.0) > 100 * B["pixel"]).all()  # no device error near the threshold
    assert np.abs(norms - host_dfs["matches"]["norm"].to_numpy()).max() <= B["pixel"]
    for col in ("label", "pred_inst_id", "gt_inst_id", "cand_id", "0.1d"):
        assert dfs["matches"][col].equals(host_dfs["matches"][col]), col
    for k, v in host_summary.items():
        assert np.allclose(summary[k], v, rtol=0, atol=10 * B["pixel"], equal_nan=True), k


def test_meter_add_or_adds_and_sampled_points_on_the_device(g12, B):
    """``ADD(-S)`` picks the mode per row from ``is_symmetric`` in one launch; ``sample_n_points`` scores the reference's
    deterministic subset of the padded table."""
    from happypose_amd import evaluation as E
    from happypose_amd.mesh_store import MeshDataBase, sample_point_ids
    from happypose_amd.synthetic import make_multiview_objects

    db = MeshDataBase.from_object_ds(make_multiview_objects())
    obj, pred, gt = g12["sym/obj_id"], g12["sym/TXO_pred"], g12["sym/TXO_gt"]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)  # noqa: E731
    meter = E.PoseErrorMeter(db, error_type="ADD(-S)", device=DEV)
    labels = meter.mesh_db.labels[obj]
    out = {k: v.cpu().numpy() for k, v in meter.compute_errors(t(pred), t(gt), labels).items()}
    for r, o in enumerate(obj):
        pts = g12["sym/points"][o][:g12["sym/n_points"][o]]
        if o in (0, 1):  # mv_0 and mv_1 carry symmetries: ADD-S
            ref = R.add_s(pred[r], gt[r], pts)
            assert abs(out["norm_avg"][r] - ref["norm_avg"]) <= B["norm_avg"] + B["point"], r
        else:
            check_row(out, r, R.add(pred[r], gt[r], pts), B)
    sym_rows = np.isin(obj, (0, 1)) & (np.arange(len(obj)) < len(obj) - 1)
    plain = E.PoseErrorMeter(db, error_type="ADD", device=DEV).compute_errors(t(pred), t(gt), labels)["norm_avg"].cpu().numpy()
    assert (out["norm_avg"][sym_rows] < plain[sym_rows]).all() and (out["norm_avg"][~np.isin(obj, (0, 1))] == plain[~np.isin(obj, (0, 1))]).all()

    n_sample = 80
    meter = E.PoseErrorMeter(db, error_type="ADD", exact_meshes=False, sample_n_points=n_sample, device=DEV)
    out = {k: v.cpu().numpy() for k, v in meter.compute_errors(t(pred), t(gt), labels).items()}
    pick = sample_point_ids(g12["sym/points"].shape[1], n_sample)
    for r, o in enumerate(obj):
        check_row(out, r, R.add(pred[r], gt[r], g12["sym/points"][o][pick]), B)


def test_calls_without_adds_rows_skip_its_launches(g12):
    """A mode column on the host tells the wrapper that no row is ADD-S (``n_add_s = 0``: no ADD-S launches, no workspace); the
    rows come out bit-identical to the call that does not know.  An ADD-S row in a call declared to hold none is answered NaN."""
    from happypose_amd import _ffi, ops

    obj, pred, gt = g12["sym/obj_id"], g12["sym/TXO_pred"], g12["sym/TXO_gt"]
    n = len(obj)
    modes = ["ADD", "ADD-SYM", "MSSD"] * n
    ids = np.tile(np.arange(n), 3)
    tables = (g12["sym/points"], g12["sym/symmetries"], g12["sym/n_sym"], g12["sym/n_points"])
    unknown = launch(modes, ids, ids, np.tile(obj, 3), pred, gt, *tables)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)  # noqa: E731
    known = ops.pose_errors_tables(ids.astype(np.int32), ids.astype(np.int32), np.tile(obj, 3).astype(np.int32),
                                   np.asarray([ops.POSE_ERR_MODES[m] for m in modes], np.int32), t(pred, torch.float32), t(gt, torch.float32),
                                   t(tables[0], torch.float32), t(tables[1], torch.float32), t(tables[2], torch.int32),
                                   t(tables[3], torch.int32), return_assign=True)
    for k, v in known.items():
        assert v.cpu().numpy().tobytes() == unknown[k].tobytes(), k
    # the C entry point with n_add_s = 0, no workspace, and one ADD-S row among ADD rows
    col = lambda a: t(np.asarray(a, np.int32), torch.int32)  # noqa: E731
    i3, mode = col([0, 1, 2]), col([0, 1, 0])
    dev = [t(pred, torch.float32), t(gt, torch.float32)] + [t(a, dt) for a, dt in zip(tables, (torch.float32, torch.float32, torch.int32, torch.int32))]
    outs = [torch.zeros(3, device=DEV), torch.zeros(3, 3, device=DEV), torch.zeros(3, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV),
            torch.zeros(3, 3, device=DEV), torch.zeros(3, device=DEV)]
    p = _ffi.ptr
    rc = _ffi.lib().hp_pose_errors(3, p(i3), p(i3), p(col(obj[:3])), p(mode), 0, p(dev[0]), len(pred), p(dev[1]), len(gt), None, p(dev[2]),
                                   p(dev[3]), p(dev[4]), p(dev[5]), tables[0].shape[0], tables[0].shape[1], tables[1].shape[1],
                                   *[p(o) for o in outs], None, None, 0, _ffi.stream_ptr(DEV))
    assert rc == 0
    norm_avg = outs[0].cpu().numpy()
    assert np.isnan(norm_avg[1]) and outs[3].cpu().numpy()[1] == -1
    same = [next(i for i in range(3 * n) if modes[i] == "ADD" and ids[i] == k) for k in (0, 2)]  # ADD of poses 0 and 2 in `unknown`
    assert norm_avg[[0, 2]].tobytes() == unknown["norm_avg"][same].tobytes()
