"""Host entry points of the multi-view matching (hp_ransac_make_infos, hp_ransac_find_inliers), the mesh tables and the Python
layer that needs no GPU, against the reference's own run (tests/golden/g11_multiview.npz).  CPU only."""

import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import multiview_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def g11(golden_dir):
    return np.load(golden_dir / "g11_multiview.npz")


@pytest.mark.parametrize("scene", R.SCENES)
def test_make_infos_exact(g11, scene):
    """Seeds and tentative matches in the reference's order, including the permutations (scene B: fewer iterations than pairs)."""
    from happypose_amd import ops

    sc = R.load_scene(g11, scene)
    n_iter = 1 if scene == "D" else int(sc["n_ransac_iter"])  # known camera poses: one hypothesis per view pair (ransac.py:167)
    seeds, tm = ops.ransac_make_infos(sc["view_id"], sc["label_id"], n_iter, 0)
    for k in R.SEED_COLUMNS:
        assert np.array_equal(seeds[k], sc["seeds"][k]), k
    assert np.array_equal(np.stack([tm[k] for k in ("hypothesis_id", "cand1", "cand2")]), sc["tmatches"])
    if scene == "B":
        assert len(seeds["view1"]) == 12 * 12 < 12 * 30


@pytest.mark.parametrize("scene", R.SCENES)
def test_find_inliers_exact(g11, scene):
    from happypose_amd import ops

    sc = R.load_scene(g11, scene)
    h, c1, c2 = sc["tmatches"]
    out = ops.ransac_find_inliers(sc["seeds"]["view1"], sc["seeds"]["view2"], h, c1, c2, sc["dists"], R.DIST_THRESHOLD, R.N_MIN_INLIERS)
    assert np.array_equal(out["inlier_matches_cand1"], sc["inlier_cand1"])
    assert np.array_equal(out["inlier_matches_cand2"], sc["inlier_cand2"])
    assert np.array_equal(out["best_hypotheses"], sc["best_hypotheses"])


def test_hypothesis_zero_is_never_kept(g11):
    """The reference's `> 0`: scene D has 12 view pairs, one hypothesis each, all good -- 11 are kept, hypothesis 0 is not."""
    sc = R.load_scene(g11, "D")
    assert len(sc["seeds"]["view1"]) == 12 and sorted(sc["best_hypotheses"].tolist()) == list(range(1, 12))


def test_host_argument_errors():
    from happypose_amd import _ffi

    lib = _ffi.lib()
    assert lib.hp_ransac_make_infos(-1, None, None, 1, 0, None, None, None, 0, None, 0) == -1
    assert lib.hp_mv_score_matches(1, None, None, None, None, 1, None, None, 1, None, 1, None, 7, None, None, None, 1, 8, 1, None,
                                   None, None) == -1
    assert b"unknown mode" in lib.hp_last_error()
    assert lib.hp_mv_estimate_camera_poses(1, None, None, None, None, None, None, 1, None, None, None, 0, 8, 1, None, None) == -1


@pytest.mark.parametrize("scene", R.SCENES)
def test_scene_level_matching_and_view_groups(g11, scene):
    import torch

    from happypose_amd import multiview as mv
    from happypose_amd.tensor_collection import PandasTensorCollection

    sc = R.load_scene(g11, scene)
    infos = pd.DataFrame({"view_id": sc["view_id"], "label": [f"mv_{i}" for i in sc["label_id"]], "score": sc["score"],
                          "cand_id": np.arange(len(sc["view_id"]))})
    cand = PandasTensorCollection(infos=infos, poses=torch.as_tensor(sc["poses"]))
    inl = {"inlier_matches_cand1": sc["inlier_cand1"], "inlier_matches_cand2": sc["inlier_cand2"], "best_hypotheses": sc["best_hypotheses"]}
    matched = mv.scene_level_matching(cand, inl)
    assert np.array_equal(matched.infos["cand_id"].values, sc["matched_cand_id"])
    assert R.partition(matched.infos["obj_id"].values, matched.infos["cand_id"].values) == \
        R.partition(sc["matched_obj_id"], sc["matched_cand_id"])
    assert sorted(set(matched.infos["obj_id"])) == list(range(matched.infos["obj_id"].nunique()))
    assert torch.equal(matched.poses, torch.as_tensor(sc["poses"][sc["matched_cand_id"]]))
    obj = mv.make_obj_infos(matched)
    assert obj["n_cand"].sum() == len(matched) and (obj["n_cand"] >= 2).all()
    pairs = mv.get_best_viewpair_pose_est(torch.as_tensor(sc["TC1C2"]), sc["seeds"], inl)
    assert np.array_equal(pairs.infos["view1"].values, sc["pairs_view1"]) and np.array_equal(pairs.infos["view2"].values, sc["pairs_view2"])
    assert np.array_equal(pairs.TC1C2.numpy(), sc["pairs_TC1C2"])
    groups = mv.make_view_groups(pairs)
    assert np.array_equal(groups["view_id"].values, sc["group_view_id"])
    assert R.partition(groups["view_group"].values, groups["view_id"].values) == R.partition(sc["group_view_group"], sc["group_view_id"])


def test_components_numbered_by_smallest_member():
    from happypose_amd.multiview import strongly_connected_components as scc

    assert scc(6, [5, 4, 1, 2, 3], [4, 5, 2, 1, 3]).tolist() == [0, 1, 1, 2, 3, 3]
    assert scc(3, [0, 1], [1, 2]).tolist() == [0, 1, 2]  # a chain is not strongly connected
    assert scc(0, [], []).tolist() == []


def test_mesh_tables(g11):
    from happypose_amd.mesh_store import MeshDataBase, pad_stack_points
    from happypose_amd.synthetic import make_multiview_objects

    db = MeshDataBase.from_object_ds(make_multiview_objects())
    plain = db.batched()
    # the no-argument call: today's points, bit for bit
    pts = pad_stack_points([np.asarray(m.vertices, np.float64) * db.obj_dict[l].scale for l, m in db.meshes.items()]).astype(np.float32)
    assert plain.points.dtype == np.float32 and np.array_equal(plain.points, pts)
    b = db.batched(aabb=True, n_sym=64)
    assert b.points.shape == (6, 8, 3) and b.symmetries.shape == (6, 64, 4, 4) and b.symmetries.dtype == np.float32
    assert b.n_sym.tolist() == [2, 64, 1, 1, 1, 1] and b.n_sym_mapping["mv_1"] == 64
    for o in range(6):
        v = np.asarray(db.meshes[f"mv_{o}"].vertices)
        assert np.allclose(b.points[o].min(0), v.min(0)) and np.allclose(b.points[o].max(0), v.max(0))
        assert np.array_equal(b.symmetries[o, b.n_sym[o]:], np.tile(np.eye(4, dtype=np.float32), (64 - b.n_sym[o], 1, 1)))
        assert np.array_equal(b.symmetries[o, 0], np.eye(4, dtype=np.float32))
    R_ = b.symmetries[..., :3, :3].astype(np.float64)
    assert np.abs(R_ @ R_.swapaxes(-1, -2) - np.eye(3)).max() < 1e-6 and np.allclose(np.linalg.det(R_), 1.0, atol=1e-6)
    assert np.allclose(b.symmetries[0, 1], np.diag([-1.0, -1.0, 1.0, 1.0]))
    a = 2 * np.pi * 5 / 64  # continuous axis z, 64 steps
    assert np.allclose(b.symmetries[1, 5, :2, :2], [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], atol=1e-7)
    assert db.batched(n_sym=8).symmetries.shape[1] == 8 and db.batched(n_sym=8).n_sym.tolist() == [2, 8, 1, 1, 1, 1]
    assert np.array_equal(b.points, g11["points"]) and np.array_equal(b.symmetries, g11["symmetries"])
    sel = b.select(["mv_1", "mv_0"])
    assert sel.symmetries.shape == (2, 64, 4, 4) and sel.points.shape == (2, 8, 3)
    with pytest.raises(NotImplementedError):
        db.batched(resample_n_points=100)


def test_discrete_then_continuous_order():
    """sym_c * sym_d, continuous index fastest; discrete translations are scaled by the mesh unit."""
    from happypose_amd.mesh_store import make_bop_symmetries

    d = np.eye(4)
    d[:3, :3] = np.diag([1.0, -1.0, -1.0])
    d[:3, 3] = [10.0, 0.0, 0.0]
    S = make_bop_symmetries([d.reshape(-1).tolist()], [{"axis": [0, 0, 1], "offset": [0, 0, 0]}], 4, scale=0.001)
    assert S.shape == (8, 4, 4)
    Rz = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    d[:3, 3] *= 0.001
    assert np.allclose(S[1], Rz) and np.allclose(S[4], d) and np.allclose(S[5], Rz @ d)


def _ba_problem(sc, device="cpu"):
    """The product's MultiviewRefinement on G11's matched candidates (torch CPU tensors: no kernel is called by the constructor
    or by sample_initial_TWO_TWC)."""
    import torch

    from happypose_amd import multiview as mv
    from happypose_amd.mesh_store import MeshDataBase
    from happypose_amd.synthetic import make_multiview_objects
    from happypose_amd.tensor_collection import PandasTensorCollection

    mesh_db = MeshDataBase.from_object_ds(make_multiview_objects()).batched(aabb=True, n_sym=64).to(device)
    cid = sc["matched_cand_id"]
    infos = pd.DataFrame({"view_id": sc["view_id"][cid], "label": [f"mv_{i}" for i in sc["label_id"][cid]], "score": sc["score"][cid],
                          "cand_id": cid, "obj_id": sc["matched_obj_id"]})
    cand = PandasTensorCollection(infos=infos, poses=torch.as_tensor(sc["poses"][cid], device=device))
    cams = PandasTensorCollection(infos=pd.DataFrame({"view_id": np.arange(4)}), K=torch.as_tensor(sc["cameras_K"]))
    pairs = PandasTensorCollection(infos=pd.DataFrame({"view1": sc["pairs_view1"], "view2": sc["pairs_view2"]}),
                                   TC1C2=torch.as_tensor(sc["pairs_TC1C2"]))
    return mv.MultiviewRefinement(cand, cams, pairs, mesh_db)


@pytest.mark.parametrize("scene", R.SCENES)
def test_sample_initial_TWO_TWC(g11, scene):
    """The seeded initialisation (np.random.RandomState(0)) against the reference's: same spanning order, float32 products."""
    sc = R.load_scene(g11, scene)
    pb = _ba_problem(sc)
    assert pb.obj_infos["obj_id"].tolist() == sc["ba_obj_id"].tolist() and pb.cam_infos["view_id"].tolist() == sc["ba_view_id"].tolist()
    TWO, TWC = pb.sample_initial_TWO_TWC(0)
    # the same float32 matrix products in the same order: a few ulp of entries <= 1.5 (BLAS kernels may differ in FMA use)
    assert np.abs(TWO.numpy() - sc["ba_init_TWO"]).max() < 1e-6 and np.abs(TWC.numpy() - sc["ba_init_TWC"]).max() < 1e-6
    assert not np.array_equal(pb.sample_initial_TWO_TWC(1)[1].numpy(), TWC.numpy())


def test_unsupported_continuous_symmetry_does_not_break_batching():
    """A continuous axis the reference's formula does not cover: the single-view tables are built as before, the multi-view path
    refuses with the reason."""
    from happypose_amd import ops
    from happypose_amd.mesh_store import MeshDataBase, RigidObject
    from happypose_amd.synthetic import make_mesh

    obj = RigidObject("odd", make_mesh(3, n_lat=4, n_lon=6, tex_size=16), symmetries_continuous=[{"axis": [0, 0, -1], "offset": [0, 0, 0]}])
    b = MeshDataBase([obj]).batched()
    assert b.points.shape[0] == 1 and b.unsupported_symmetries == ["odd"]
    with pytest.raises(ValueError, match="not supported"):
        ops._mv_tables(b.to("cpu"))


def test_device_tables_follow_the_tensors():
    from happypose_amd.mesh_store import MeshDataBase
    from happypose_amd.synthetic import make_multiview_objects

    b = MeshDataBase.from_object_ds(make_multiview_objects()).batched(aabb=True)
    assert b.device_tables is None
    b = b.to("cpu")
    b.points = b.points * 2
    assert np.array_equal(b.device_tables["points"].numpy(), b.points.numpy()) and b.device_tables["n_sym"].tolist() == [2, 64, 1, 1, 1, 1]


@pytest.mark.parametrize("scene", R.SCENES)
def test_seed_row_tables_reproduce_the_rows(g11, scene):
    """The compact row form the device reads (per-seed offsets + each view pair's match list once) expands to exactly the
    (hypothesis_id, cand1, cand2) rows of make_ransac_infos."""
    from happypose_amd import ops

    sc = R.load_scene(g11, scene)
    tm = dict(zip(("hypothesis_id", "cand1", "cand2"), sc["tmatches"]))
    row_off, pair_off, pc1, pc2 = ops.seed_row_tables(sc["seeds"], tm)
    rows = np.arange(len(tm["cand1"]))
    seed = np.searchsorted(row_off, rows, side="right") - 1
    assert row_off[0] == 0 and row_off[-1] == len(rows) and np.array_equal(seed, tm["hypothesis_id"])
    assert np.array_equal(pc1[pair_off[seed] + rows - row_off[seed]], tm["cand1"])
    assert np.array_equal(pc2[pair_off[seed] + rows - row_off[seed]], tm["cand2"])
    assert len(pc1) <= len(rows) and len(pair_off) == len(sc["seeds"]["view1"])
