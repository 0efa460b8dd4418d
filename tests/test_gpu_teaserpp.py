"""GPU tests of the TEASER++ depth refiner (csrc/teaser.hip, ``TeaserppRefiner``) against the NumPy restatement of its
definition (tests/teaserpp_ref.py).  Parity with the teaserpp_python library of the reference is unpinned (absent here): what is
compared is this project's definition, stage by stage -- sampling, clique, registration -- and the quality of the refined poses
on a rendered scene."""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import teaserpp_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

NOISE_BOUND = 0.01
MARGIN = 1e-4  # no pair of the generated correspondences is this close to the graph's threshold


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


# ---- the C entry points on NumPy inputs ------------------------------------------------------------------------------

def _fps(dev, clouds, k):
    """``hp_teaser_fps`` on a list of [N_i, 3] float32 clouds (one batch): list of the selected indices."""
    from happypose_amd._ffi import check, lib, ptr, stream_ptr

    n, n_max = len(clouds), max(len(c) for c in clouds)
    pts = np.zeros((n, n_max, 3), np.float32)
    for i, c in enumerate(clouds):
        pts[i, :len(c)] = c
    d_pts = torch.as_tensor(pts, device=dev)
    d_cnt = torch.as_tensor(np.array([len(c) for c in clouds], np.int32), device=dev)
    scratch = torch.empty((n, n_max), dtype=torch.float32, device=dev)
    idx = torch.full((n, k), -7, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_teaser_fps(n, n_max, ptr(d_pts), ptr(d_cnt), k, ptr(scratch), ptr(idx), stream_ptr(dev)), "hp_teaser_fps")
    idx = idx.cpu().numpy()
    out = []
    for i, c in enumerate(clouds):
        m = min(k, len(c))
        assert (idx[i, m:] == -1).all(), idx[i, m:]
        out.append(idx[i, :m].astype(np.int64))
    return out


def _register(dev, pairs, min_num_inliers=50, m_max=None):
    """``hp_teaser_register`` on a list of ``(a [M_i,3], b [M_i,3])`` float32 (one batch)."""
    from happypose_amd._ffi import check, lib, ptr, stream_ptr

    n = len(pairs)
    m_max = m_max or max(1, max(len(a) for a, _ in pairs))
    A = np.zeros((n, m_max, 3), np.float32)
    B = np.zeros((n, m_max, 3), np.float32)
    for i, (a, b) in enumerate(pairs):
        A[i, :len(a)], B[i, :len(b)] = a, b
    d_a, d_b = torch.as_tensor(A, device=dev), torch.as_tensor(B, device=dev)
    d_m = torch.as_tensor(np.array([len(a) for a, _ in pairs], np.int32), device=dev)
    T = torch.empty((n, 4, 4), dtype=torch.float32, device=dev)
    status, inliers, clique = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    mask = torch.empty((n, 32), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_teaser_register(n, m_max, ptr(d_a), ptr(d_b), ptr(d_m), NOISE_BOUND, min_num_inliers, ptr(T), ptr(status),
                                       ptr(inliers), ptr(clique), ptr(mask), stream_ptr(dev)), "hp_teaser_register")
    return dict(T=T.cpu().numpy(), status=status.cpu().numpy(), num_inliers=inliers.cpu().numpy(),
                clique_size=clique.cpu().numpy(), clique_mask=mask.cpu().numpy().view(np.uint32))


def _angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra.astype(np.float64) @ Rb.T.astype(np.float64)) - 1.0) / 2.0, -1.0, 1.0)))


# ---- sampling ------------------------------------------------------------------------------------------------------

def _lattice(n, seed):
    """Points on a 1/1024 m lattice inside a 0.5 m cube: squared distances are exact in float32 and ties are real."""
    return (np.random.RandomState(seed).randint(0, 512, (n, 3)) / 1024.0).astype(np.float32)


@pytest.mark.parametrize("n_points", [3001, 50, 1])
def test_fps_exact_on_a_lattice(dev, n_points):
    cloud = _lattice(n_points, seed=n_points)
    got = _fps(dev, [cloud], 64)[0]
    assert np.array_equal(got, TR.fps(cloud, 64, dtype=np.float32))
    assert np.array_equal(got, TR.fps(cloud, 64))  # exact arithmetic: float64 agrees too


def test_fps_batch_of_different_sizes(dev):
    clouds = [_lattice(3001, 1), _lattice(50, 2), _lattice(1, 3)]
    got = _fps(dev, clouds, 64)
    for g, c in zip(got, clouds):
        assert np.array_equal(g, TR.fps(c, 64))


def test_fps_float_points_take_a_farthest_point_at_every_step(dev):
    """20 000 random float32 points, k = 1000: the device's own sequence is checked step by step in float64 -- the chosen
    point's distance to the set chosen before it is within 1e-6 (relative) of the largest.  Robust to near-ties, unlike a
    comparison of indices."""
    cloud = np.random.RandomState(7).uniform(-0.25, 0.25, (20000, 3)).astype(np.float32)
    idx = _fps(dev, [cloud], 1000)[0]
    assert idx[0] == 0 and len(idx) == 1000 and len(set(idx.tolist())) == 1000
    P = cloud.astype(np.float64)
    mind = np.full(len(P), np.inf)
    worst = 0.0
    for s in range(1, 1000):
        mind = np.minimum(mind, ((P - P[idx[s - 1]]) ** 2).sum(1))
        worst = max(worst, 1.0 - mind[idx[s]] / mind.max())
    print("largest relative shortfall of a chosen squared distance:", worst)
    assert worst <= 1e-6


# ---- graph, clique and registration ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases():
    """30 % inliers at <= 1 mm noise, the rest displaced by 5 - 30 cm, no pair within MARGIN of the graph's threshold; with the
    float64 and float32 runs of the restatement."""
    out = {}
    for M in (65, 130, 1000):
        a, b, R, t, inl = TR.make_registration_case(M, int(round(0.3 * M)), seed=M, margin=MARGIN)
        min_inl = int(inl.sum()) // 2
        out[M] = dict(a=a, b=b, R=R, t=t, inl=inl, min_inl=min_inl, ref=TR.register(a, b, NOISE_BOUND, min_num_inliers=min_inl),
                      ref32=TR.register(a, b, NOISE_BOUND, min_num_inliers=min_inl, dtype=np.float32))
    return out


@pytest.fixture(scope="module")
def registered(dev, cases):
    return {M: _register(dev, [(c["a"], c["b"])], c["min_inl"]) for M, c in cases.items()}


@pytest.mark.parametrize("M", [65, 130, 1000])
def test_clique_equals_the_restatement(cases, registered, M):
    c, got = cases[M], registered[M]
    # what makes an exact comparison legitimate: both precisions decide every edge alike
    gaps = TR.pair_gaps(c["a"], c["b"])
    off = ~np.eye(M, dtype=bool)
    assert (np.abs(gaps[off] - 2 * NOISE_BOUND) >= MARGIN).all()
    assert np.array_equal(TR.consistency_graph(c["a"], c["b"], NOISE_BOUND, dtype=np.float32), TR.consistency_graph(c["a"], c["b"], NOISE_BOUND))
    want = TR.clique_mask_words(c["ref"]["clique"])
    print("clique size", int(got["clique_size"][0]), "restatement", c["ref"]["clique_size"], "inliers", int(c["inl"].sum()))
    assert np.array_equal(got["clique_mask"][0], want)
    assert got["clique_size"][0] == c["ref"]["clique_size"]
    # padding bits
    bits = np.unpackbits(got["clique_mask"][0].view(np.uint8), bitorder="little")
    assert not bits[M:].any()


@pytest.mark.parametrize("M", [65, 130, 1000])
def test_registration_matches_the_restatement(cases, registered, M):
    c, got = cases[M], registered[M]
    ref, ref32 = c["ref"], c["ref32"]
    assert ref["status"] == 0
    # the scale of legitimate round-off: the float32 against the float64 run of the restatement, never the device's output
    tol = max(4.0 * float(np.abs(ref32["T"].astype(np.float64) - ref["T"]).max()), 1e-6)
    diff = float(np.abs(got["T"][0].astype(np.float64) - ref["T"]).max())
    print("M", M, "tolerance", tol, "largest difference", diff)
    assert got["status"][0] == ref["status"] and got["num_inliers"][0] == ref["num_inliers"]
    assert diff <= tol
    assert np.array_equal(got["T"][0][3], [0, 0, 0, 1])


@pytest.mark.parametrize("M", [65, 130, 1000])
def test_registration_recovers_the_truth(cases, registered, M):
    c, got = cases[M], registered[M]
    T = got["T"][0]
    t_err, ang = float(np.linalg.norm(T[:3, 3] - c["t"])), _angle(T[:3, :3], c["R"])
    print("M", M, "translation error", t_err, "angle", ang)
    assert t_err < 1e-3      # the noise amplitude
    assert ang < 0.01        # 2 noise / extent at the 0.2 m extent of the point set


def test_registration_rejections(dev, cases):
    eye = np.eye(4, dtype=np.float32)
    a, b, _, _, _ = TR.make_registration_case(128, 0, seed=4, margin=MARGIN)  # every edge decided alike in both precisions
    ref = TR.register(a, b, NOISE_BOUND)
    got = _register(dev, [(a, b)])
    assert ref["status"] in (-2, -3) and got["status"][0] == ref["status"] and np.array_equal(got["T"][0], eye)
    assert got["clique_size"][0] == ref["clique_size"]
    # two correspondences: no clique of three
    got = _register(dev, [(a[:2], a[:2])], min_num_inliers=1)
    assert got["status"][0] == -2 and np.array_equal(got["T"][0], eye) and got["clique_size"][0] == 2
    # a batch whose middle prediction is rejected
    c = cases[130]
    got = _register(dev, [(c["a"], c["b"]), (a, b), (c["a"][:65], c["b"][:65])], min_num_inliers=10, m_max=130)
    assert got["status"].tolist() == [0, ref["status"], 0]
    assert np.array_equal(got["T"][1], eye)
    for i in (0, 2):
        assert np.linalg.norm(got["T"][i][:3, 3] - c["t"]) < 2e-3 and _angle(got["T"][i][:3, :3], c["R"]) < 0.02


# ---- the refiner on a rendered scene -----------------------------------------------------------------------------------

def _make_scene(dev):
    """Measured depth = rendered depth of 3 objects at their true poses over a far wall, with an occluder (a block of depth
    10 cm nearer) over about a third of the object with the largest visible area; predictions = the true poses perturbed by millimetres / degrees."""
    from happypose_amd.renderer import BatchRenderer
    from happypose_amd.synthetic import euler_to_R, make_object_dataset, make_scene

    ds = make_object_dataset(3, seed=1, tex_size=64)
    renderer = BatchRenderer(ds, device=dev)
    sc = make_scene(n_detections=3, n_hypotheses=1, n_objects=3, seed=5)
    H, W = 480, 640
    K = torch.as_tensor(sc["K"], device=dev)
    T_gt = torch.as_tensor(sc["TCO_det"], device=dev)
    labels = [renderer.store.labels[i] for i in sc["det_obj_ids"]]
    d = renderer.render(labels, T_gt, K.expand(3, 3, 3).contiguous(), [[]] * 3, (H, W), render_depth=True).depths[:, 0]
    measured = torch.full((H, W), 1.5, device=dev)
    for i in range(3):  # nearest surface wins
        measured = torch.where((d[i] > 0) & (d[i] < measured), d[i], measured)
    # the occluder: the left third of the columns that object is visible in
    visible = [(d[i] > 0) & (d[i] == measured) for i in range(3)]
    occ = int(np.argmax([int(v.sum()) for v in visible]))
    cols = torch.nonzero(visible[occ].any(0))[:, 0]
    u0, u1 = int(cols.min()), int(cols.min()) + (int(cols.max()) - int(cols.min()) + 1) // 3
    block = torch.zeros((H, W), dtype=torch.bool, device=dev)
    block[:, u0:u1] = True
    block &= visible[occ]
    measured = torch.where(block, measured - 0.10, measured)
    rs = np.random.RandomState(0)
    T_pred = sc["TCO_det"].copy().astype(np.float64)
    T_pred[:, :3, :3] = T_pred[:, :3, :3] @ euler_to_R(rs.normal(0, 1.5, (3, 3)) * np.pi / 180)
    T_pred[:, :3, 3] += rs.normal(0, 1.0, (3, 3)) * np.array([0.004, 0.004, 0.008])
    return dict(renderer=renderer, labels=labels, K=K, T_gt=sc["TCO_det"], T_pred=T_pred.astype(np.float32),
                measured=measured[None].contiguous(), store=renderer.store, occ=occ,
                visible=[int(v.sum()) for v in visible],
                occluded=float(block.sum()) / float(visible[occ].sum()))


@pytest.fixture(scope="module")
def scene(dev):
    return _make_scene(dev)


def _predictions(scene, dev):
    import pandas as pd

    from happypose_amd.tensor_collection import PandasTensorCollection

    infos = pd.DataFrame(dict(label=scene["labels"], batch_im_id=[0, 0, 0], instance_id=[0, 1, 2]))
    return PandasTensorCollection(infos=infos, poses=torch.as_tensor(scene["T_pred"], device=dev))


def _terr(A, B):
    return np.linalg.norm(A[:, :3, 3] - B[:, :3, 3], axis=1)


def _refine(scene, dev, **kw):
    from happypose_amd.teaserpp_refiner import TeaserppRefiner

    refiner = TeaserppRefiner(scene["store"].mesh_db, scene["renderer"], **kw)
    preds = _predictions(scene, dev)
    out, extra = refiner.refine_poses(preds, depth=scene["measured"], K=scene["K"])
    rv = extra["retval"].cpu().numpy()
    e1 = _terr(out.poses.cpu().numpy(), scene["T_gt"])
    print(kw, "retval", rv.tolist(), "inliers", extra["num_inliers"].tolist(), "clique", extra["clique_size"].tolist(),
          "error after", e1.tolist())
    return refiner, preds, out, extra, rv, e1


def test_refiner_on_a_scene_with_an_occluder(dev, scene):
    """Accepted poses are closer to the truth than the input, for every prediction, with ``mask_type="threshold"``.

    Why not the "simple" mask for that statement: in this scene (the fixture of tests/test_gpu_icp.py) the third object lies
    entirely BEHIND the second -- none of its pixels is visible in the measured depth.  With the simple mask every one of its
    correspondences pairs its rendered surface with the surface in front of it, 10 - 20 cm nearer: a large, rigidly consistent
    set of wrong correspondences.  The definition itself then moves the pose onto the occluding object (the float64
    restatement, tests/teaserpp_ref.py, on the same depth maps: clique 625, 574 inliers, translation error 6.3 mm -> 119 mm;
    the device returns the same numbers), as the reference's solver would on such input; no registration of depth can improve
    a pose that has no visible pixel.  The threshold mask (|measured - rendered| <= 0.1, the reference's other mask type) is what
    removes such correspondences: that prediction is then rejected as "too few masked pixels" and keeps its pose.
    The robustness to an occluder is checked with the simple mask on the object that carries it: 28 % of its visible pixels
    are covered by a block 10 cm nearer, and further pixels fall on the wall."""
    e0 = _terr(scene["T_pred"], scene["T_gt"])
    occ, visible = scene["occ"], np.array(scene["visible"])
    print("occluded object", occ, "share", scene["occluded"], "visible pixels", visible.tolist(), "error before", e0.tolist())
    assert 0.15 < scene["occluded"] < 0.5

    refiner, preds, out, extra, rv, e1 = _refine(scene, dev, mask_type="threshold")
    got = out.poses.cpu().numpy()
    assert torch.equal(out.poses_input, preds.poses)
    assert set(extra) == {"retval", "num_inliers", "clique_size", "depth_rendered"}
    assert (rv[visible > 0] == 0).all()  # every object that can be seen is registered
    assert (e1[rv == 0] < e0[rv == 0]).all()
    assert np.array_equal(got[rv != 0], scene["T_pred"][rv != 0])
    acc = rv == 0
    assert (extra["num_inliers"].cpu().numpy()[acc] >= refiner.min_num_inliers).all()
    assert (extra["clique_size"].cpu().numpy()[acc] >= 3).all()
    # bit-identical from run to run
    out2, extra2 = refiner.refine_poses(preds, depth=scene["measured"], K=scene["K"])
    assert torch.equal(out2.poses, out.poses) and torch.equal(extra2["num_inliers"], extra["num_inliers"])

    # evenly spaced correspondences instead of farthest-point sampling
    _, _, _, _, rv3, e3 = _refine(scene, dev, mask_type="threshold", use_farthest_point_sampling=False)
    assert (rv3[visible > 0] == 0).all() and (e3[rv3 == 0] < e0[rv3 == 0]).all()

    # the simple mask keeps the occluder's and the wall's pixels as wrong correspondences of the occluded object: it is still
    # registered, and better than before
    _, _, out4, _, rv4, e4 = _refine(scene, dev)
    assert rv4[occ] == 0 and e4[occ] < e0[occ]
    assert torch.equal(out4.poses_input, preds.poses)


def test_refiner_rejections(dev, scene):
    from happypose_amd.teaserpp_refiner import TeaserppRefiner

    preds = _predictions(scene, dev)
    # no overlap between rendered and measured depth within the threshold (measured is 1 m farther): every pose is kept
    refiner = TeaserppRefiner(scene["store"].mesh_db, scene["renderer"], mask_type="threshold")
    out, extra = refiner.refine_poses(preds, depth=scene["measured"] + 1.0, K=scene["K"])
    assert (extra["retval"].cpu().numpy() == -1).all() and torch.equal(out.poses, preds.poses)
    assert torch.equal(out.poses_input, preds.poses)
    # empty input
    out, extra = refiner.refine_poses(preds[[]], depth=scene["measured"], K=scene["K"])
    assert len(out) == 0 and extra == {}
