"""The multi-view matching kernels (csrc/multiview.hip) and ``happypose_amd.multiview`` on the GPU, against the float64
restatement (tests/multiview_ref.py) and the reference's own run (tests/golden/g11_multiview.npz).

Tolerances are not chosen here: for each quantity the reference's OWN float32 deviation from float64 is measured on the CPU
(tests/test_multiview_reference.py, constants in multiview_ref.py) and the kernels -- float32 with FMA and another summation
order -- are allowed GPU_FACTOR = 4 times that."""

import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import multiview_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# measured reference error (multiview_ref.py) -> bound = 4 x
TOL_DISTS = R.GPU_FACTOR * R.REF_F32_ERR_DISTS  # 4 x 3.4573e-07 = 1.383e-06 m
TOL_TC1C2_T = R.GPU_FACTOR * R.REF_F32_ERR_TC1C2_T  # 4 x 2.2740e-07 = 9.096e-07 m
TOL_TC1C2_R = R.GPU_FACTOR * R.REF_F32_ERR_TC1C2_R  # 4 x 1.1408e-07 = 4.563e-07
# Reprojected distance (no reference run recorded: it belongs to the bundle adjustment).  Bound from the number format: pixel
# coordinates here lie in [0, 1024), float32 ulp there is 6.1e-5 px; a projected coordinate goes through ~8 rounded operations
# (matrix products, divide) and a distance takes the difference of two: 16 ulp = 1e-3 px.
TOL_REPROJ_PX = 16 * 2.0 ** -14


@pytest.fixture(scope="module")
def g11(golden_dir):
    return np.load(golden_dir / "g11_multiview.npz")


@pytest.fixture(scope="module")
def mesh_db():
    from happypose_amd.mesh_store import MeshDataBase
    from happypose_amd.synthetic import make_multiview_objects

    return MeshDataBase.from_object_ds(make_multiview_objects()).batched(aabb=True, n_sym=64).to("cuda")


def _kernels(sc, mesh_db):
    from happypose_amd import ops

    poses = torch.as_tensor(sc["poses"], device="cuda")
    if "cameras_TWC" in sc:
        TWC = sc["cameras_TWC"].astype(np.float32)
        TC1C2 = torch.as_tensor(R.invert(TWC[sc["seeds"]["view1"]]) @ TWC[sc["seeds"]["view2"]], device="cuda")
    else:
        TC1C2 = ops.mv_estimate_camera_poses(poses, sc["label_id"], sc["seeds"], mesh_db)
    h, c1, c2 = sc["tmatches"]
    dists = ops.mv_score_matches(h, c1, c2, TC1C2, poses, sc["label_id"], poses, mesh_db)
    return TC1C2.cpu().numpy(), dists.cpu().numpy()


def _deviation(sc, T, d):
    T64, d64 = R.restate(sc)
    return (np.abs(d - d64).max(), np.abs(T[:, :3, 3] - T64[:, :3, 3]).max(), np.abs(T[:, :3, :3] - T64[:, :3, :3]).max())


@pytest.mark.parametrize("scene", R.SCENES)
def test_kernels_against_float64(g11, mesh_db, scene):
    sc = R.load_scene(g11, scene)
    T, d = _kernels(sc, mesh_db)
    e_d, e_t, e_r = _deviation(sc, T, d)
    print(f"scene {scene}: |dists| {e_d:.4e} (bound {TOL_DISTS:.3e})  |TC1C2 t| {e_t:.4e} ({TOL_TC1C2_T:.3e})  "
          f"|TC1C2 R| {e_r:.4e} ({TOL_TC1C2_R:.3e})")
    assert np.array_equal(T[:, 3], np.tile([0, 0, 0, 1], (len(T), 1)))
    assert e_d <= TOL_DISTS and e_t <= TOL_TC1C2_T and e_r <= TOL_TC1C2_R


@pytest.mark.parametrize("scene", R.SCENES)
def test_decisions_equal_the_reference(g11, mesh_db, scene):
    """Inliers and best hypotheses from the PRODUCT's distances.  No row lies in the margin band on any scene (asserted on the CPU:
    test_margin_band_and_ties), so nothing is excluded."""
    from happypose_amd import ops

    sc = R.load_scene(g11, scene)
    _, d = _kernels(sc, mesh_db)
    h, c1, c2 = sc["tmatches"]
    out = ops.ransac_find_inliers(sc["seeds"]["view1"], sc["seeds"]["view2"], h, c1, c2, d, R.DIST_THRESHOLD, R.N_MIN_INLIERS)
    assert np.array_equal(out["inlier_matches_cand1"], sc["inlier_cand1"])
    assert np.array_equal(out["inlier_matches_cand2"], sc["inlier_cand2"])
    assert np.array_equal(out["best_hypotheses"], sc["best_hypotheses"])


def test_mutated_symmetry_table_fails_the_check(g11, mesh_db):
    """One symmetry of the 2-fold object turned by 1 degree: the scene-C distances leave the bound (by orders of magnitude)."""
    import copy

    sc = R.load_scene(g11, "C")
    bad = copy.copy(mesh_db)  # shares everything but the symmetry table, which is replaced by a turned copy
    sym = mesh_db.symmetries.clone()
    a = np.deg2rad(1.0)
    turn = torch.eye(4, device="cuda")
    turn[:2, :2] = torch.tensor([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    sym[0, 1] = turn @ sym[0, 1]
    bad.symmetries = sym
    e_d, _, _ = _deviation(sc, *_kernels(sc, bad))
    print(f"mutated table: |dists| {e_d:.4e} (bound {TOL_DISTS:.3e})")
    assert e_d > 100 * TOL_DISTS
    assert _deviation(sc, *_kernels(sc, mesh_db))[0] <= TOL_DISTS


def test_reprojected_mode(g11, mesh_db):
    """HP_MV_DIST_REPROJECTED on scene C's matched pairs: T1 = a candidate's pose, T2 = TC1C2 @ the other view's candidate."""
    from happypose_amd import ops

    sc = R.load_scene(g11, "C")
    h, c1, c2 = (a[::7] for a in sc["tmatches"])
    K = np.tile(np.array([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]]), (len(sc["TC1C2"]), 1, 1))
    T64 = sc["TC1C2"].astype(np.float64)
    p64 = sc["poses"].astype(np.float64)
    want, want_ids = R.reprojected_distance(p64[c1], T64[h] @ p64[c2], K[h], sc["label_id"][c1], sc["points"].astype(np.float64),
                                            sc["symmetries"].astype(np.float64), sc["n_sym"])
    got, ids = ops.mv_score_matches(h, c1, c2, torch.as_tensor(sc["TC1C2"]), torch.as_tensor(sc["poses"]), sc["label_id"],
                                    torch.as_tensor(sc["poses"]), mesh_db, K=torch.as_tensor(K), return_sym_ids=True)
    got, ids = got.cpu().numpy(), ids.cpu().numpy()
    ok = np.isfinite(want) & (want < 20.0)  # true matches: both projections inside the 640 x 480 image the bound is derived for
    assert ok.sum() > 50
    print(f"reprojected: max deviation {np.abs(got - want)[ok].max():.3e} px (bound {TOL_REPROJ_PX:.3e}), {ok.sum()} rows")
    assert np.abs(got - want)[ok].max() <= TOL_REPROJ_PX
    clear = ok & (sc["n_sym"][sc["label_id"][c1]] <= 2)  # the continuous axis has neighbours 5.6 deg apart: may be close calls
    assert clear.any() and np.array_equal(ids[clear], want_ids[clear])


def test_out_of_range_index_answers_nan(g11, mesh_db):
    """Index columns already on the device are not read by the host; the kernel answers NaN."""
    from happypose_amd import ops

    sc = R.load_scene(g11, "A")
    poses = torch.as_tensor(sc["poses"], device="cuda")
    h, c1, c2 = (torch.as_tensor(a[:8].copy(), device="cuda") for a in sc["tmatches"])
    c2[3] = 10 ** 6
    h[5] = -1
    d = ops.mv_score_matches(h, c1, c2, torch.as_tensor(sc["TC1C2"]), poses, sc["label_id"], poses, mesh_db).cpu().numpy()
    assert np.isnan(d[[3, 5]]).all() and np.isfinite(np.delete(d, [3, 5])).all()
    seeds = {k: torch.as_tensor(v[:4].copy(), device="cuda") for k, v in sc["seeds"].items()}
    seeds["match2_cand1"][2] = len(poses)
    T = ops.mv_estimate_camera_poses(poses, sc["label_id"], seeds, mesh_db).cpu().numpy()
    assert np.isnan(T[2]).all() and np.isfinite(T[[0, 1, 3]]).all()


def _candidates(sc):
    from happypose_amd.tensor_collection import PandasTensorCollection

    infos = pd.DataFrame({"view_id": sc["view_id"], "label": [f"mv_{i}" for i in sc["label_id"]], "score": sc["score"]})
    return PandasTensorCollection(infos=infos, poses=torch.as_tensor(sc["poses"], device="cuda"))


def _match(sc, mesh_db, scene):
    from happypose_amd import multiview as mv
    from happypose_amd.tensor_collection import PandasTensorCollection

    cameras = None
    if scene == "D":
        cameras = PandasTensorCollection(infos=pd.DataFrame({"view_id": np.arange(4)}), TWC=torch.as_tensor(sc["cameras_TWC"]))
    return mv.multiview_candidate_matching(_candidates(sc), mesh_db, dist_threshold=R.DIST_THRESHOLD, cameras=cameras,
                                           n_ransac_iter=int(sc["n_ransac_iter"]), n_min_inliers=R.N_MIN_INLIERS)


@pytest.mark.parametrize("scene", R.SCENES)
def test_candidate_matching_end_to_end(g11, mesh_db, scene):
    from happypose_amd import multiview as mv

    sc = R.load_scene(g11, scene)
    out = _match(sc, mesh_db, scene)
    fc, pairs = out["filtered_candidates"], out["pairs_TC1C2"]
    assert set(out) == {"filtered_candidates", "scene_infos", "pairs_TC1C2", "time_models", "time_score", "time_misc"}
    assert np.array_equal(fc.infos["cand_id"].values, sc["matched_cand_id"])
    assert R.partition(fc.infos["obj_id"].values, fc.infos["cand_id"].values) == R.partition(sc["matched_obj_id"], sc["matched_cand_id"])
    assert np.array_equal(pairs.infos["view1"].values, sc["pairs_view1"]) and np.array_equal(pairs.infos["view2"].values, sc["pairs_view2"])
    e = np.abs(pairs.TC1C2.cpu().numpy() - sc["pairs_TC1C2"])
    # both sides are float32 runs: the reference's own error plus the kernel's allowance
    assert e[:, :3, 3].max() <= TOL_TC1C2_T + R.REF_F32_ERR_TC1C2_T and e[:, :3, :3].max() <= TOL_TC1C2_R + R.REF_F32_ERR_TC1C2_R
    groups = mv.make_view_groups(pairs)
    assert R.partition(groups["view_group"].values, groups["view_id"].values) == R.partition(sc["group_view_group"], sc["group_view_id"])
    assert len(out["scene_infos"]) == fc.infos["obj_id"].nunique()
    again = _match(sc, mesh_db, scene)  # reproducibility: bit-identical
    assert torch.equal(again["pairs_TC1C2"].TC1C2, pairs.TC1C2) and again["filtered_candidates"].infos.equals(fc.infos)


def test_kernels_bit_identical_across_runs(g11, mesh_db):
    sc = R.load_scene(g11, "C")
    T1, d1 = _kernels(sc, mesh_db)
    T2, d2 = _kernels(sc, mesh_db)
    assert T1.tobytes() == T2.tobytes() and d1.tobytes() == d2.tobytes()


def test_robustness(g11, mesh_db):
    from happypose_amd import multiview as mv

    sc = R.load_scene(g11, "A")
    cand = _candidates(sc)
    with pytest.raises(ValueError, match="nothing to match"):  # no candidate at all (e.g. none above score_th)
        mv.multiview_candidate_matching(cand[np.zeros(0, dtype=int)], mesh_db)
    with pytest.raises(ValueError, match="nothing to match"):  # a single view
        mv.multiview_candidate_matching(cand[np.where(sc["view_id"] == 0)[0]], mesh_db)
    # no view pair reaches n_min_inliers: the reference's answer is an empty scene
    out = mv.multiview_candidate_matching(cand, mesh_db, n_ransac_iter=30, n_min_inliers=7)
    assert len(out["filtered_candidates"]) == 0 and len(out["pairs_TC1C2"]) == 0 and len(out["scene_infos"]) == 0


# ---- bundle adjustment and the scene predictor -----------------------------------------------------------------------------------
# bounds = 4 x the reference arithmetic's own float32 error (multiview_ref.py; measured by tests/test_multiview_reference.py)
TOL_BA_ERRORS_PX = R.GPU_FACTOR * R.REF_F32_ERR_BA_ERRORS_PX  # 4 x 1.293e-04 = 5.17e-04 px
TOL_JTJ_REL = R.GPU_FACTOR * R.REF_F32_ERR_JTJ_REL  # 4 x 2.894e-07 = 1.16e-06 of the largest entry
TOL_JTE_REL = R.GPU_FACTOR * R.REF_F32_ERR_JTE_REL  # 4 x 1.428e-04 = 5.71e-04 of the largest entry
TOL_BA_SYMDIST = R.GPU_FACTOR * R.REF_F32_ERR_BA_SYMDIST  # 4 x 2.5163e-05 = 1.007e-04 m
TOL_BA_GEODESIC = R.GPU_FACTOR * R.REF_F32_ERR_BA_GEODESIC  # 4 x 5.2736e-04 = 2.109e-03 rad


@pytest.mark.parametrize("scene", R.SCENES)
def test_ba_linearize_against_float64_autograd(g11, scene):
    """hp_mv_ba_linearize at G11's initialisation: residuals in (candidate, point, xy) order, loss, and the per-candidate 18 x 18
    blocks added in candidate order, against the autograd Jacobian of the float64 restatement."""
    from test_multiview_host import _ba_problem

    sc = R.load_scene(g11, scene)
    ref = R.BAProblem(sc)
    e64, loss64, J = ref.forward_jacobian(ref.TWO_9d0, ref.TCW_9d0)
    pb = _ba_problem(sc, "cuda")
    TWO_9d, TCW_9d = ref.TWO_9d0.float().cuda(), ref.TCW_9d0.float().cuda()
    errors, loss, JtJ, Jte = pb.forward_jacobian(TWO_9d, TCW_9d, 25.0)
    assert errors.shape == (len(ref.cand_obj), 8, 2) and JtJ.shape == (J.shape[1], J.shape[1])
    A, b = (J.T @ J).numpy(), (J.T @ e64.reshape(-1)).numpy()
    d_e = (errors.cpu().double() - e64).abs().max().item()
    d_A, d_b = np.abs(JtJ - A).max() / np.abs(A).max(), np.abs(Jte - b).max() / np.abs(b).max()
    print(f"scene {scene}: |errors| {d_e:.3e} px ({TOL_BA_ERRORS_PX:.3e})  JtJ {d_A:.3e} ({TOL_JTJ_REL:.3e})  Jte {d_b:.3e} ({TOL_JTE_REL:.3e})")
    assert d_e <= TOL_BA_ERRORS_PX and d_A <= TOL_JTJ_REL and d_b <= TOL_JTE_REL
    assert abs(float(loss) - float(loss64)) <= 1e-4 * float(loss64)
    assert np.array_equal(JtJ, JtJ.T)  # structure: symmetric, and zero where no candidate links the two parameter blocks
    vis = np.zeros((ref.n_obj, ref.n_views), bool)
    vis[ref.cand_obj, ref.cand_view] = True
    o, v = np.argwhere(~vis)[0] if (~vis).any() else (None, None)
    if o is not None:
        assert not JtJ[9 * o:9 * o + 9, 9 * (ref.n_obj + v):9 * (ref.n_obj + v) + 9].any()
    again = pb.forward_jacobian(TWO_9d, TCW_9d, 25.0)
    assert torch.equal(again[0], errors) and np.array_equal(again[2], JtJ) and np.array_equal(again[3], Jte)


def _scene_inputs(name):
    from happypose_amd.synthetic import make_multiview_scene
    from happypose_amd.tensor_collection import PandasTensorCollection

    sc = make_multiview_scene(name)
    n = len(sc["view_id"])
    infos = pd.DataFrame({"scene_id": np.zeros(n, int), "group_id": np.zeros(n, int), "view_id": sc["view_id"],
                          "label": [f"mv_{i}" for i in sc["label_id"]], "score": sc["score"], "batch_im_id": sc["view_id"]})
    cand = PandasTensorCollection(infos=infos, poses=torch.as_tensor(sc["poses"], device="cuda"))
    cams = PandasTensorCollection(infos=pd.DataFrame({"scene_id": np.zeros(4, int), "view_id": np.arange(4), "batch_im_id": np.arange(4)}),
                                  K=torch.as_tensor(sc["K"], dtype=torch.float32), TWC=torch.as_tensor(sc["TWC"], dtype=torch.float32))
    return cand, cams


@pytest.fixture(scope="module")
def predictor():
    from happypose_amd.mesh_store import MeshDataBase
    from happypose_amd.multiview import MultiviewScenePredictor
    from happypose_amd.synthetic import make_multiview_objects

    return MultiviewScenePredictor(MeshDataBase.from_object_ds(make_multiview_objects()))


@pytest.mark.parametrize("scene", R.SCENES)
def test_predict_scene_state(g11, predictor, scene):
    """End to end on every scene: partition and view groups as G11; the gauge-invariant poses inv(TWC[v]) TWO[o] of ba_output
    against G11's by symmetric distance and rotation geodesic.  When the accept / reject sequence of the LM run differs from the
    reference's (float32 noise in `rho` at convergence: it differs between float64 and the reference on every scene, see
    test_ba_restatement_against_the_reference) the final loss is compared instead: within 1 % of G11's, or lower.  The
    residuals and normal-equation blocks are float64 here, so the run follows the float64 restatement's path (scene D, known
    cameras, is the sensitive one: 100 iterations, lambda up to 1e6, reference 0.185782, float64 0.185640)."""
    from happypose_amd.synthetic import MULTIVIEW_SCENES

    sc = R.load_scene(g11, scene)
    n_iter, known = MULTIVIEW_SCENES[scene]
    cand, cams = _scene_inputs(scene)
    captured = []
    from happypose_amd import multiview as mv

    solve = mv.MultiviewRefinement.solve
    mv.MultiviewRefinement.solve = lambda self, *a, **k: captured.append(solve(self, *a, **k)) or captured[-1]
    try:
        pred = predictor.predict_scene_state(cand, cams, use_known_camera_poses=known, ransac_n_iter=n_iter)
        again = predictor.predict_scene_state(cand, cams, use_known_camera_poses=known, ransac_n_iter=n_iter)
    finally:
        mv.MultiviewRefinement.solve = solve
    assert set(pred) == {"cand_inputs", "cand_matched", "scene/objects", "scene/cameras", "ba_input", "ba_output", "ba_output+all_cand"}
    assert torch.equal(pred["ba_output"].poses, again["ba_output"].poses)  # bit-identical runs
    m = pred["cand_matched"].infos
    assert R.partition(m["obj_id"].values, m["cand_id"].values) == R.partition(sc["matched_obj_id"], sc["matched_cand_id"])
    assert sorted(pred["scene/cameras"].infos["view_id"]) == sorted(sc["ba_view_id"].tolist())
    assert len(pred["ba_output+all_cand"]) == len(pred["ba_output"]) + len(cand)
    hist = captured[0]["history"]
    loss = [float(x) for x in hist["loss"]]
    assert loss[-1] <= loss[0]
    # ba_output in G11's object order: objects are matched through their member candidates
    out = pred["ba_output"]
    first_cand = {o: c for c, o in reversed(list(zip(sc["matched_cand_id"].tolist(), sc["matched_obj_id"].tolist())))}
    mine_obj = dict(zip(m["cand_id"].tolist(), m["obj_id"].tolist()))
    poses = np.zeros((len(sc["ba_obj_id"]), len(sc["ba_view_id"]), 4, 4))
    for row, (o, v) in enumerate(zip(out.infos["obj_id"].tolist(), out.infos["view_id"].tolist())):
        for gi, go in enumerate(sc["ba_obj_id"].tolist()):
            if mine_obj[first_cand[go]] == o:
                poses[gi, sc["ba_view_id"].tolist().index(v)] = out.poses[row].cpu().numpy()
    d, geo = R.pose_deviation(poses, R.golden_relative_poses(sc), sc["ba_obj_label_id"], sc["points"], sc["symmetries"])
    same_branches = len(hist["lambda"]) == len(sc["ba_lambda"]) and np.allclose(hist["lambda"], sc["ba_lambda"])
    print(f"scene {scene}: {len(loss)} iterations (reference {len(sc['ba_loss'])}), loss {loss[0]:.6f} -> {loss[-1]:.6f} (reference "
          f"{sc['ba_loss'][-1]:.6f}), symmetric distance {d:.3e} m ({TOL_BA_SYMDIST:.3e}), geodesic {geo:.3e} rad ({TOL_BA_GEODESIC:.3e}), "
          f"same accept/reject sequence: {same_branches}")
    if same_branches:
        assert d <= TOL_BA_SYMDIST and geo <= TOL_BA_GEODESIC
    else:
        assert loss[-1] <= 1.01 * float(sc["ba_loss"][-1])
        # the run ends in the same minimum all the same (A - C: a converged LM run; D keeps moving slowly): the pose bounds hold
        # for the converged scenes whichever branch sequence led there, so they are asserted, not only printed
        if scene != "D":
            assert d <= TOL_BA_SYMDIST and geo <= TOL_BA_GEODESIC


def test_predictor_robustness(predictor):
    cand, cams = _scene_inputs("A")
    with pytest.raises(ValueError, match="no candidate"):
        predictor.predict_scene_state(cand, cams, score_th=2.0)
    with pytest.raises(ValueError, match="nothing to match"):
        predictor.predict_scene_state(cand[np.where(cand.infos["view_id"] == 0)[0]], cams)
    with pytest.raises(ValueError, match="enough inlier"):  # threshold so tight that no view pair reaches three inliers
        predictor.predict_scene_state(cand, cams, ransac_n_iter=30, ransac_dist_threshold=1e-7)


@pytest.mark.parametrize("scene", R.SCENES)
def test_seed_indexed_rows_equal_explicit_rows(g11, mesh_db, scene):
    """hp_mv_score_seed_matches (no per-row index columns) gives bit for bit the distances of hp_mv_score_matches on the rows."""
    from happypose_amd import ops

    sc = R.load_scene(g11, scene)
    T, d = _kernels(sc, mesh_db)
    tm = dict(zip(("hypothesis_id", "cand1", "cand2"), sc["tmatches"]))
    d2 = ops.mv_score_seed_matches(sc["seeds"], tm, torch.as_tensor(T, device="cuda"), torch.as_tensor(sc["poses"], device="cuda"),
                                   sc["label_id"], mesh_db).cpu().numpy()
    assert d.tobytes() == d2.tobytes()


def test_scale_memory_is_bounded_by_the_rows(mesh_db):
    """6 views x 24 candidates per view at n_ransac_iter = 2000 (the reference's default): the matching completes, and the device
    memory it takes on top of what was there is at most rows x 8 B plus the tables -- no [rows, symmetries] temporary, no per-row
    index columns.  Tables: per seed 4 index columns + TC1C2 + 2 offsets = 16 + 64 + 8 B, per candidate pose + object id = 68 B,
    each view pair's match list twice 4 B; the caching allocator rounds every block up to 512 B, 64 KiB covers that for the
    handful of blocks involved."""
    from happypose_amd import multiview as mv, ops
    from happypose_amd.synthetic import make_multiview_scene
    from happypose_amd.tensor_collection import PandasTensorCollection

    sc = make_multiview_scene("scale", n_views=6, n_objects=24)
    assert len(sc["view_id"]) == 6 * 24
    infos = pd.DataFrame({"view_id": sc["view_id"], "label": [f"mv_{i}" for i in sc["label_id"]], "score": sc["score"]})
    cand = PandasTensorCollection(infos=infos, poses=torch.as_tensor(sc["poses"], device="cuda"))
    seeds, tm = ops.ransac_make_infos(sc["view_id"], sc["label_id"], 2000, 0)
    n_rows, n_seeds, n_cand = len(tm["cand1"]), len(seeds["view1"]), len(cand)
    n_pair_matches = len(ops.seed_row_tables(seeds, tm)[2])
    assert n_seeds == 30 * 2000 and n_rows > 5_000_000
    del seeds, tm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = mv.multiview_candidate_matching(cand, mesh_db, n_ransac_iter=2000)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    bound = n_rows * 8 + n_seeds * (16 + 64 + 8) + n_cand * 68 + n_pair_matches * 8 + 64 * 1024
    print(f"scale: {n_rows} rows, {n_seeds} seeds, peak {peak / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB "
          f"(rows x 8 B = {n_rows * 8 / 2**20:.1f} MiB; a [rows, 64, 4, 4] float temporary would be {n_rows * 4096 / 2**30:.1f} GiB)")
    assert peak <= bound
    assert len(out["pairs_TC1C2"]) == 30 and out["filtered_candidates"].infos["obj_id"].nunique() == 24
    gt = sc["gt_obj"][out["filtered_candidates"].infos["cand_id"].values]
    assert R.partition(out["filtered_candidates"].infos["obj_id"].values) == R.partition(gt)
