"""The float64 restatement of the multi-view candidate matching (tests/multiview_ref.py) against the reference's own run
(tests/golden/g11_multiview.npz, tools/gen_golden_multiview.py).  CPU only.  It also measures the reference's float32 error --
the yardstick of the GPU tolerances -- and asserts the conditions under which decisions can be compared exactly."""

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import multiview_ref as R  # noqa: E402

# a distance closer to the threshold than this could fall on either side in a float32 implementation
DIST_TOL = R.GPU_FACTOR * R.REF_F32_ERR_DISTS


@pytest.fixture(scope="module")
def g11(golden_dir):
    return np.load(golden_dir / "g11_multiview.npz")


@pytest.fixture(scope="module")
def restated(g11):
    return {s: R.restate(R.load_scene(g11, s)) for s in R.SCENES}


def _errors(g11, restated, s):
    sc = R.load_scene(g11, s)
    T, d = restated[s]
    return (np.abs(d - sc["dists"]).max(), np.abs(T[:, :3, 3] - sc["TC1C2"][:, :3, 3]).max(),
            np.abs(T[:, :3, :3] - sc["TC1C2"][:, :3, :3]).max())


@pytest.mark.parametrize("scene", R.SCENES)
def test_real_outputs_within_float32_roundoff(g11, restated, scene):
    """TC1C2 and dists of the reference's float32 run agree with float64 to a few float32 ulps of their magnitude (poses ~1 m,
    distances up to ~1.5 m: ulp 1.2e-7)."""
    e_d, e_t, e_r = _errors(g11, restated, scene)
    print(f"scene {scene}: |dists| {e_d:.4e}  |TC1C2 t| {e_t:.4e}  |TC1C2 R| {e_r:.4e}")
    assert e_d < 1e-6 and e_t < 1e-6 and e_r < 5e-7


def test_reference_float32_error_is_the_recorded_one(g11, restated):
    """The constants the GPU tolerances are derived from are what is measured here."""
    e = np.array([_errors(g11, restated, s) for s in R.SCENES]).max(0)
    print("measured max over scenes:", e)
    np.testing.assert_allclose(e, [R.REF_F32_ERR_DISTS, R.REF_F32_ERR_TC1C2_T, R.REF_F32_ERR_TC1C2_R], rtol=5e-3)


@pytest.mark.parametrize("scene", R.SCENES)
def test_decisions_exact(g11, restated, scene):
    """Inliers and best hypotheses from the float64 distances (rounded to float32) equal the reference's; the restated inlier
    search run on the reference's own distances does too."""
    sc = R.load_scene(g11, scene)
    for dists in (sc["dists"], restated[scene][1]):
        i1, i2, best = R.find_inliers(sc["seeds"]["view1"], sc["seeds"]["view2"], sc["tmatches"], dists)
        assert np.array_equal(i1, sc["inlier_cand1"]) and np.array_equal(i2, sc["inlier_cand2"])
        assert np.array_equal(best, sc["best_hypotheses"])
    assert len(sc["best_hypotheses"]) > 0


@pytest.mark.parametrize("scene", R.SCENES)
def test_margin_band_and_ties(g11, restated, scene):
    """Conditions for exact decision tests of a float32 implementation: (1) at most 0.5 % of the rows lie within DIST_TOL of the
    threshold, none on A, B, D; (2) no two DISTINCT hypotheses of a view pair with equal inlier counts have distance sums closer
    than the error a sum of that many distances can carry.  Seeds that share match 1 and its symmetry are one and the same model
    -- TC1C2 = TC1Oa S* inv(TC2Ob) is a function of (a, b, S*) alone, here, in the reference and in the kernel, so their rows are
    bitwise equal and the first one in seed order wins everywhere (strict `<`); they are not ties of rounding; (3) no seed's symmetry choice is a near tie."""
    sc = R.load_scene(g11, scene)
    T, d = restated[scene]
    share = float((np.abs(d - R.DIST_THRESHOLD) <= DIST_TOL).mean())
    print(f"scene {scene}: share of rows in the margin band {share:.4%} (closest {np.abs(d - R.DIST_THRESHOLD).min():.3e})")
    assert share <= 0.005
    if scene in "ABD":
        assert share == 0.0
    v1, v2 = sc["seeds"]["view1"], sc["seeds"]["view2"]
    *_, stats = R.find_inliers(v1, v2, sc["tmatches"], d, details=True)
    closest = np.inf
    for pair in set(zip(v1.tolist(), v2.tolist())):
        hyps = [h for h in range(len(v1)) if (v1[h], v2[h]) == pair and stats[h][0] >= R.N_MIN_INLIERS]
        for i, a in enumerate(hyps):
            for b in hyps[i + 1:]:
                if stats[a][0] == stats[b][0] and T[a].tobytes() != T[b].tobytes():
                    gap = abs(stats[a][1] - stats[b][1]) / stats[a][0]  # per summed distance
                    closest = min(closest, gap)
    print(f"scene {scene}: closest pair of hypotheses, |sum difference| / n_inliers = {closest:.3e}")
    assert closest > 2 * DIST_TOL  # each sum carries at most n_inliers * DIST_TOL


@pytest.mark.parametrize("scene", ("A", "B", "C"))
def test_symmetry_choice_of_the_seeds_is_not_a_tie(g11, scene):
    """The arg-min symmetry of estimate_camera_poses is separated from the runner-up by more than the tolerance on every seed
    whose object a has symmetries (else TC1C2 could not be compared)."""
    sc = R.load_scene(g11, scene)
    poses, pts, sym = (sc[k].astype(np.float64) for k in ("poses", "points", "symmetries"))
    TObC2, obj, n_sym = R.invert(poses), sc["label_id"], sc["n_sym"]
    a, b, g, d = (sc["seeds"][k] for k in R.SEED_COLUMNS[2:])
    closest = np.inf
    for n in np.where(n_sym[obj[a]] > 1)[0]:
        S = sym[obj[a[n]], :n_sym[obj[a[n]]]]
        T2 = ((poses[a[n]] @ S) @ TObC2[b[n]]) @ poses[d[n]]
        dist, _ = R.symmetric_distance(np.repeat(poses[g[n]][None], len(S), 0), T2, np.repeat(obj[g[n]], len(S)), pts, sym)
        two = np.sort(dist)[:2]
        closest = min(closest, two[1] - two[0])
    print(f"scene {scene}: smallest gap between the best two symmetries of a seed {closest:.3e}")
    assert closest > 2 * DIST_TOL


@pytest.mark.parametrize("scene", R.SCENES)
def test_partitions(g11, scene):
    """Matched candidates and view groups of the product's component routine equal the reference's as partitions; scene C drops
    the view that shares two objects only and keeps two instances of one label apart."""
    from happypose_amd.multiview import strongly_connected_components

    sc = R.load_scene(g11, scene)
    n = len(sc["view_id"])
    ids = strongly_connected_components(n, sc["inlier_cand1"], sc["inlier_cand2"])
    keep = np.bincount(ids)[ids] >= 2
    assert np.array_equal(np.where(keep)[0], sc["matched_cand_id"])
    assert R.partition(ids[keep], np.where(keep)[0]) == R.partition(sc["matched_obj_id"], sc["matched_cand_id"])
    if scene == "C":
        assert set(sc["group_view_id"].tolist()) == {0, 1, 2}
        lab = sc["label_id"][sc["matched_cand_id"]]
        assert len({o for o, l in zip(sc["matched_obj_id"], lab) if l == 2}) == 2


# ---- bundle adjustment --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ba_runs(g11):
    import torch

    out = {}
    for s in R.SCENES:
        sc = R.load_scene(g11, s)
        pb = R.BAProblem(sc)
        TWO, TCW, hist = pb.optimize_lm(optimize_cameras=(s != "D"))
        e, _, J = pb.forward_jacobian(pb.TWO_9d0, pb.TCW_9d0)
        pb32 = R.BAProblem(sc, torch.float32)
        e32, _, J32 = pb32.forward_jacobian(pb32.TWO_9d0, pb32.TCW_9d0)
        A, A32 = (J.T @ J).numpy(), (J32.T @ J32).double().numpy()
        b, b32 = (J.T @ e.reshape(-1)).numpy(), (J32.T @ e32.reshape(-1)).double().numpy()
        out[s] = dict(sc=sc, pb=pb, TWO=TWO, TCW=TCW, hist=hist,
                      dev=R.pose_deviation(pb.relative_poses(TWO, TCW), R.golden_relative_poses(sc), pb.obj_mesh, sc["points"], sc["symmetries"]),
                      jtj=np.abs(A - A32).max() / np.abs(A).max(), jte=np.abs(b - b32).max() / np.abs(b).max(),
                      err=float((e - e32.double()).abs().max()))
    return out


@pytest.mark.parametrize("scene", R.SCENES)
def test_ba_restatement_against_the_reference(ba_runs, scene):
    """The float64 LM run from G11's initialisation ends where the reference's float32 run ends: same loss to 0.1 %, poses within
    a few 1e-5 m.  The accept / reject sequence is NOT the same on any scene -- float32 noise in `rho` near convergence ends the
    reference's run a step or two later -- which is why the GPU test falls back to the final loss when its sequence differs."""
    r = ba_runs[scene]
    sc, hist = r["sc"], r["hist"]
    print(f"scene {scene}: {len(hist['loss'])} iterations (reference {len(sc['ba_loss'])}), loss {hist['loss'][0]:.6f} -> "
          f"{hist['loss'][-1]:.6f} (reference {sc['ba_loss'][0]:.6f} -> {sc['ba_loss'][-1]:.6f}), symmetric distance {r['dev'][0]:.4e} m, "
          f"geodesic {r['dev'][1]:.4e} rad")
    assert abs(hist["loss"][0] - sc["ba_loss"][0]) < 1e-3 * sc["ba_loss"][0]
    assert abs(hist["loss"][-1] - sc["ba_loss"][-1]) < 1e-3 * sc["ba_loss"][-1]
    assert hist["loss"][-1] <= hist["loss"][0]
    assert r["dev"][0] < 1e-4 and r["dev"][1] < 2e-3


def test_ba_reference_float32_error_is_the_recorded_one(ba_runs):
    dev = np.array([ba_runs[s]["dev"] for s in R.SCENES]).max(0)
    jtj, jte, err = (max(ba_runs[s][k] for s in R.SCENES) for k in ("jtj", "jte", "err"))
    print("measured:", dev, jtj, jte, err)
    np.testing.assert_allclose([dev[0], dev[1], jtj, jte, err], [R.REF_F32_ERR_BA_SYMDIST, R.REF_F32_ERR_BA_GEODESIC,
                               R.REF_F32_ERR_JTJ_REL, R.REF_F32_ERR_JTE_REL, R.REF_F32_ERR_BA_ERRORS_PX], rtol=2e-2)


@pytest.mark.parametrize("scene", R.SCENES)
def test_reprojected_distance_at_the_initialisation(ba_runs, scene):
    """symmetric_distance_reprojected as the reference computed it (G11 ba_init_reproj_dists, continuous axis included)."""
    r = ba_runs[scene]
    d, _ = r["pb"].align(r["pb"].TWO_9d0, r["pb"].TCW_9d0)
    assert np.abs(d - r["sc"]["ba_init_reproj_dists"]).max() < 16 * 2.0 ** -14
