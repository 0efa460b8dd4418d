"""The TEASER++ depth refiner without a GPU: the CPU restatement of its definition (tests/teaserpp_ref.py) does what a
robust registration must, and the refiner is wired into the package (module, constructor, model loading)."""
import inspect
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import teaserpp_ref as TR  # noqa: E402


def _angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1.0) / 2.0, -1.0, 1.0)))


@pytest.fixture(scope="module")
def occluded_case():
    """40 inliers at <= 1 mm noise, 88 outliers displaced by 5 - 30 cm towards the camera."""
    a, b, R, t, inl = TR.make_registration_case(128, 40, seed=3, one_sided=True)
    return dict(a=a, b=b, R=R, t=t, inl=inl)


def test_register_recovers_pose_and_clique_is_the_inlier_set(occluded_case):
    c = occluded_case
    r = TR.register(c["a"], c["b"], min_num_inliers=30)
    assert r["status"] == 0 and r["clique"] == sorted(np.nonzero(c["inl"])[0]) and r["clique_size"] == 40
    assert r["num_inliers"] >= 40
    # 1 mm noise over a 0.2 m point set: translation below the noise, angle below 2 noise / extent
    assert np.linalg.norm(r["T"][:3, 3] - c["t"]) < 1e-3
    assert _angle(r["T"][:3, :3], c["R"]) < 0.01
    # the float32 run of the same formulae takes the same decisions
    r32 = TR.register(c["a"], c["b"], min_num_inliers=30, dtype=np.float32)
    assert r32["status"] == 0 and r32["clique"] == r["clique"] and np.abs(r32["T"] - r["T"]).max() < 1e-5


def test_plain_least_squares_fails_on_the_same_data(occluded_case):
    """The case is a real one: the closed-form fit over ALL correspondences is off by centimetres."""
    c = occluded_case
    a, b = c["a"].astype(np.float64), c["b"].astype(np.float64)
    ca, cb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((a - ca).T @ (b - cb))
    V = Vt.T
    R = V @ np.diag([1.0, 1.0, np.linalg.det(V @ U.T)]) @ U.T
    t = cb - R @ ca
    err = np.linalg.norm((a @ R.T + t) - (a @ c["R"].T + c["t"]), axis=1)
    assert err.max() > 0.02 and np.linalg.norm(t - c["t"]) > 0.02


def test_all_outliers_are_rejected():
    a, b, _, _, _ = TR.make_registration_case(128, 0, seed=4)
    r = TR.register(a, b)
    assert r["status"] in (-2, -3) and np.array_equal(r["T"], np.eye(4))


def test_too_few_masked_pixels_keep_the_pose():
    K = np.array([[100.0, 0, 16], [0, 100.0, 12], [0, 0, 1]])
    rendered = np.zeros((24, 32))
    rendered[4:12, 4:12] = 0.8  # 64 pixels
    measured = np.full((24, 32), 0.81)
    TCO = np.eye(4)
    TCO[:3, 3] = [0.01, 0.02, 0.8]
    T, status, inliers, clique = TR.refine(rendered, measured, K, TCO, n_min_points=100)
    assert status == -1 and np.array_equal(T, TCO) and inliers == 0 and clique == 0
    # enough pixels: the 1 cm shift along z is found (the measured patch is also 1.25 % larger, which a rigid fit cannot follow:
    # hence millimetres, not round-off)
    T, status, inliers, clique = TR.refine(rendered, measured, K, TCO, n_min_points=50, n_points=64, min_num_inliers=50)
    assert status == 0 and clique == 64 and inliers == 64
    assert _angle(T[:3, :3], np.eye(3)) < 0.02 and np.allclose(T[:3, 3] - TCO[:3, 3], [0, 0, 0.01], atol=2e-3)
    # the threshold mask removes everything when the maps are far apart
    assert TR.refine(rendered, measured + 1.0, K, TCO, mask_type="threshold", n_min_points=50)[1] == -1
    with pytest.raises(ValueError):
        TR.refine(rendered, measured, K, TCO, mask_type="nope")


def test_fps_takes_the_corners_of_a_cube_first():
    rs = np.random.RandomState(0)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float)
    pts = np.concatenate([rs.uniform(-0.3, 0.3, (1, 3)), corners, rs.uniform(-0.3, 0.3, (50, 3))])
    idx = TR.fps(pts, 9)
    assert idx[0] == 0 and sorted(idx[1:]) == list(range(1, 9))
    # ties go to the lowest index, and fewer points than samples gives them all
    line = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0.5, 0, 0]], float)
    assert list(TR.fps(line, 8)) == [0, 1, 2, 3]
    assert list(TR.fps(line[:1], 8)) == [0]


def test_refiner_module_and_constructor_signature():
    from happypose_amd.icp_refiner import DepthRefiner
    from happypose_amd.teaserpp_refiner import TeaserppRefiner

    assert issubclass(TeaserppRefiner, DepthRefiner)
    params = inspect.signature(TeaserppRefiner.__init__).parameters
    assert list(params) == ["self", "mesh_db", "renderer", "mask_type", "depth_delta_thresh", "n_min_points", "n_points",
                            "noise_bound", "min_num_inliers", "use_farthest_point_sampling"]
    defaults = {k: p.default for k, p in params.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(mask_type="simple", depth_delta_thresh=0.1, n_min_points=100, n_points=1000, noise_bound=0.01,
                            min_num_inliers=50, use_farthest_point_sampling=True)
    assert list(inspect.signature(TeaserppRefiner.refine_poses).parameters) == ["self", "predictions", "masks", "depth", "K"]
    renderer = SimpleNamespace(device="cpu")
    r = TeaserppRefiner("mesh_db", renderer)
    assert r.mesh_db == "mesh_db" and r.renderer is renderer and r.n_points == 1000
    with pytest.raises(ValueError):
        TeaserppRefiner("mesh_db", renderer, n_points=1025)
    with pytest.raises(ValueError):
        TeaserppRefiner("mesh_db", renderer, mask_type="nope")


def test_load_model_builds_the_named_depth_refiner(monkeypatch):
    from happypose_amd import load_model
    from happypose_amd.icp_refiner import ICPRefiner
    from happypose_amd.teaserpp_refiner import TeaserppRefiner

    renderer = SimpleNamespace(device="cpu")
    for name in ("teaserpp", "TEASERPP", "TeaserPP"):
        r = load_model.make_depth_refiner(name, "mesh_db", renderer)
        assert isinstance(r, TeaserppRefiner) and r.renderer is renderer
    assert isinstance(load_model.make_depth_refiner("ICP", "mesh_db", renderer), ICPRefiner)
    assert load_model.make_depth_refiner(None, "mesh_db", renderer) is None
    with pytest.raises(ValueError):
        load_model.make_depth_refiner("ransac", "mesh_db", renderer)

    # load_named_model: the entry's refiner by default, the keyword overrides it
    monkeypatch.setattr(load_model, "load_pose_models",
                        lambda **kw: (SimpleNamespace(), SimpleNamespace(renderer=renderer), "mesh_db"))
    monkeypatch.setattr(load_model, "PoseEstimator", lambda **kw: SimpleNamespace(**kw))
    monkeypatch.setitem(load_model.NAMED_MODELS, "test-teaserpp",
                        dict(load_model.NAMED_MODELS["megapose-1.0-RGB-multi-hypothesis-icp"], depth_refiner="teaserpp"))
    icp_name = "megapose-1.0-RGB-multi-hypothesis-icp"
    assert isinstance(load_model.load_named_model(icp_name, None).depth_refiner, ICPRefiner)
    assert load_model.load_named_model("megapose-1.0-RGB", None).depth_refiner is None
    assert isinstance(load_model.load_named_model("test-teaserpp", None).depth_refiner, TeaserppRefiner)
    assert isinstance(load_model.load_named_model(icp_name, None, depth_refiner="teaserpp").depth_refiner, TeaserppRefiner)
    assert isinstance(load_model.load_named_model("megapose-1.0-RGB", None, depth_refiner="icp").depth_refiner, ICPRefiner)
    assert load_model.load_named_model(icp_name, None, depth_refiner=None).depth_refiner is None
