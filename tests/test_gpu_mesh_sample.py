"""Mesh surface resampling on the device (csrc/mesh_sample.hip), ``MeshDataBase.batched(resample_n_points=...)`` and
``ModelNetErrorMeter`` against the NumPy restatement (tests/mesh_sample_ref.py).

Shapes: the smallest at which each mechanism can break -- a tetrahedron, a cube with two zero-area faces (one last), a single
triangle (the clamp), strips of 1023 / 1024 / 1025 / 2049 faces (the scan works in chunks of 1024 faces: one short of a chunk, a
full one, one into the second, one into the third), the golden mesh (15728 faces, 16 chunks), 1 .. 4096 samples (one thread, one
short of a wavefront, a wavefront, one over, several workgroups) and three ragged objects in one call.

Bounds: face ids are EQUAL wherever the pick is at least 1e-9 (relative) away from a CDF boundary -- the device's fp64 prefix sum
differs from the sequential one by about F 2^-53; the area within F 2^-50 relative (a reordered fp64 sum); the points within 4 x
the restatement's own float32-vs-float64 difference on that case (``mesh_sample_ref.POINT_F32_ERROR``, measured and asserted by
tests/test_mesh_sample_reference.py), floor one float32 ulp of the largest coordinate."""

import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mesh_sample_ref as R  # noqa: E402
import pose_errors_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_MAX = max(R.N_SAMPLES)
EMPTY = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))


@pytest.fixture(scope="module")
def cases(golden_dir):
    return R.cases(golden_dir)


@pytest.fixture(scope="module")
def ref(cases):
    """The restatement of (case, object index) at the largest sample count, computed once and never written to."""
    cache = {}

    def get(name, obj=0):
        if (name, obj) not in cache:
            cache[name, obj] = R.sample(*cases[name], N_MAX, R.SEED, obj)
        return cache[name, obj]

    return get


def draw(meshes, n, seed=R.SEED):
    from happypose_amd import ops

    pts, fid, area = ops.mesh_sample_surface([m[0] for m in meshes], [m[1] for m in meshes], n, seed=seed, return_face_ids=True,
                                             return_areas=True, device=DEV)
    assert pts.is_cuda and pts.dtype == torch.float32 and fid.dtype == torch.int32 and area.dtype == torch.float64
    assert pts.shape == (len(meshes), n, 3) and fid.shape == (len(meshes), n) and area.shape == (len(meshes),)
    return pts.cpu().numpy(), fid.cpu().numpy(), area.cpu().numpy()


def check_object(name, mesh, s, pts, fid, area, n):
    """Checks 1 - 3 of one object of a call: ``s`` is the restatement at the same object index."""
    v, f = mesh
    F = len(f)
    keep = s["margin"][:n] >= R.MARGIN_MIN
    share = float((~keep).mean())
    rel_area = abs(area - s["total"]) / s["total"]
    assert (fid >= 0).all() and (fid < F).all()
    p_ref = R.points_from(v, f, fid, s["ia"][:n], s["ib"][:n], np.float64)  # the device's own face, the same (ia, ib)
    err = float(np.linalg.norm(pts.astype(np.float64) - p_ref, axis=1).max())
    print(f"{name} n={n}: left out {int((~keep).sum())}, face mismatches {int((fid[keep] != s['face_id'][:n][keep]).sum())}, "
          f"area rel {rel_area:.3e} (bound {F * 2.0 ** -50:.3e}), points {err:.3e} (bound {R.point_bound(name, v):.3e})")
    assert share <= R.EXCLUDED_SHARE_CAP, (name, n, share)
    assert np.array_equal(fid[keep], s["face_id"][:n][keep]), name                                 # 1
    assert rel_area <= F * 2.0 ** -50, (name, rel_area)                                            # 2
    assert err <= R.point_bound(name, v), (name, err)                                              # 3


@pytest.mark.parametrize("name", ["tetrahedron", "cube", "triangle"] + [f"grid{n}" for n in R.GRID_FACES] + ["golden"])
def test_every_case_against_the_restatement(cases, ref, name):
    pts, fid, area = draw([cases[name]], N_MAX)
    check_object(name, cases[name], ref(name), pts[0], fid[0], area[0], N_MAX)
    if name == "cube":  # the zero-area faces (5 and the last one) are never picked
        assert not np.isin(fid[0], [5, len(cases[name][1]) - 1]).any()


@pytest.mark.parametrize("n", R.N_SAMPLES[:-1])
def test_sample_counts(cases, ref, n):
    """1, 63, 64, 65 and 1000 samples of the cube and the tetrahedron: the same samples as the first ``n`` of 4096."""
    meshes = [cases["cube"], EMPTY, cases["tetrahedron"]]
    pts, fid, area = draw(meshes, n)
    check_object("cube", cases["cube"], ref("cube", 0), pts[0], fid[0], area[0], n)
    check_object("tetrahedron", cases["tetrahedron"], ref("tetrahedron", 2), pts[2], fid[2], area[2], n)
    big_pts, big_fid, _ = draw(meshes, N_MAX)
    assert np.array_equal(pts[[0, 2]].view(np.uint32), big_pts[[0, 2], :n].view(np.uint32)) and np.array_equal(fid[[0, 2]], big_fid[[0, 2], :n])
    assert np.isnan(pts[1]).all() and (fid[1] == -1).all() and area[1] == 0  # no faces


def test_ragged_call_independence_and_seed(cases, ref):
    meshes = [cases[name] for name in R.RAGGED]
    pts, fid, area = draw(meshes, 1000)
    for o, name in enumerate(R.RAGGED):
        check_object(name, cases[name], ref(name, o), pts[o], fid[o], area[o], 1000)
    # two calls give identical bytes
    pts2, fid2, area2 = draw(meshes, 1000)
    assert pts.tobytes() == pts2.tobytes() and fid.tobytes() == fid2.tobytes() and area.tobytes() == area2.tobytes()
    # an object alone (at the same object index, behind face-less placeholders) is what it is inside the ragged call
    for o, name in enumerate(R.RAGGED):
        p1, f1, a1 = draw([EMPTY] * o + [cases[name]], 1000)
        assert p1[o].tobytes() == pts[o].tobytes() and f1[o].tobytes() == fid[o].tobytes() and a1[o] == area[o], name
        assert np.isnan(p1[:o]).all() and (f1[:o] == -1).all()
    # ... and depends on its index and on both halves of the seed
    p0, _, _ = draw([cases[R.RAGGED[1]]], 1000)
    assert not np.array_equal(p0[0], pts[1])
    for seed in (R.SEED ^ 1, R.SEED ^ (1 << 40)):
        ps, fs, a_s = draw(meshes, 1000, seed=seed)
        assert not np.array_equal(ps, pts) and a_s.tobytes() == area.tobytes()
        check_object(R.RAGGED[2], cases[R.RAGGED[2]], R.sample(*cases[R.RAGGED[2]], 1000, seed, 2), ps[2], fs[2], a_s[2], 1000)


def test_guarded_objects_and_their_neighbours(cases, ref):
    from happypose_amd import ops

    v_t, f_t = cases["tetrahedron"]
    flat = (np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]], np.float32), np.array([[0, 1, 2], [1, 2, 3], [0, 0, 3]], np.int32))
    pts, fid, area = draw([cases["cube"], flat, cases["tetrahedron"]], 300)  # (a mesh without faces: test_sample_counts)
    assert np.isnan(pts[1]).all() and (fid[1] == -1).all() and area[1] == 0  # every face has zero area
    check_object("cube", cases["cube"], ref("cube", 0), pts[0], fid[0], area[0], 300)
    check_object("tetrahedron", cases["tetrahedron"], ref("tetrahedron", 2), pts[2], fid[2], area[2], 300)

    # an index outside the object's own vertices: refused on the host ...
    bad_hi, bad_lo = f_t.copy(), f_t.copy()
    bad_hi[2, 1], bad_lo[1, 0] = len(v_t), -1  # = V: it would read the NEXT object's first vertex
    for bad in (bad_hi, bad_lo):
        with pytest.raises(AssertionError):
            ops.mesh_sample_surface([v_t, v_t], [bad, f_t], 10, device=DEV)
    # ... and through the tables, which check nothing, a guard row of the kernels: NaN / -1, it reads no vertex, neighbours as before
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)  # noqa: E731
    v_c, f_c = cases["cube"]
    for bad in (bad_hi, bad_lo):
        verts = np.concatenate([v_c, v_t, v_t])
        faces = np.concatenate([f_c, bad, f_t])
        voff = np.cumsum([0, len(v_c), len(v_t), len(v_t)])
        foff = np.cumsum([0, len(f_c), len(bad), len(f_t)])
        out = ops.mesh_sample_surface_tables(t(verts, torch.float32), t(faces, torch.int32), t(voff, torch.int32), t(foff, torch.int32),
                                             300, seed=R.SEED)
        p, fi, a = (out[k].cpu().numpy() for k in ("points", "face_id", "area"))
        assert np.isnan(p[1]).all() and (fi[1] == -1).all() and np.isnan(a[1])
        check_object("cube", cases["cube"], ref("cube", 0), p[0], fi[0], a[0], 300)
        check_object("tetrahedron", cases["tetrahedron"], ref("tetrahedron", 2), p[2], fi[2], a[2], 300)
    # offsets that pass the face table the workspace was sized for: the object is guarded, nothing past the table is touched
    out = ops.mesh_sample_surface_tables(t(v_t, torch.float32), t(f_t, torch.int32), t([0, 4, 4], torch.int32), t([0, 4, 9], torch.int32), 64,
                                         seed=R.SEED)
    assert np.isnan(out["points"][1].cpu().numpy()).all() and (out["face_id"][1] == -1).all() and not torch.isnan(out["points"][0]).any()


def test_nothing_to_do_launches_nothing():
    """``n_samples == 0`` / ``n_obj == 0``: HP_OK before any pointer is looked at."""
    from happypose_amd import _ffi, ops

    lib = _ffi.lib()
    assert lib.hp_mesh_sample_surface(3, None, None, None, None, 0, 5, None, None, None, None, 0, None) == 0
    assert lib.hp_mesh_sample_surface(0, None, None, None, None, 100, 5, None, None, None, None, 0, None) == 0
    pts, fid = ops.mesh_sample_surface([R.tetrahedron()[0]], [R.tetrahedron()[1]], 0, return_face_ids=True, device=DEV)
    assert pts.shape == (1, 0, 3) and fid.shape == (1, 0)


# ---- MeshDataBase.batched(resample_n_points=...) ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mesh_db(cases):
    """The golden mesh (millimetres), a point cloud of 600 vertices and a scaled tetrahedron: surfaces at positions 0 and 2."""
    from happypose_amd.mesh_io import MeshData
    from happypose_amd.mesh_store import MeshDataBase, RigidObject

    v_g, f_g = cases["golden"]
    v_t, f_t = cases["tetrahedron"]
    cloud = np.random.RandomState(11).uniform(-30, 30, (600, 3))
    objs = [RigidObject("obj_000001", MeshData(vertices=v_g.astype(np.float64), faces=f_g), mesh_units="mm"),
            RigidObject("cloud", MeshData(vertices=cloud, faces=np.zeros((0, 3), np.int32)), mesh_units="mm"),
            RigidObject("tetra", MeshData(vertices=v_t.astype(np.float64), faces=f_t), mesh_units="m", scaling_factor=0.05)]
    return MeshDataBase(objs)


def test_batched_resample(cases, mesh_db):
    from happypose_amd import ops
    from happypose_amd.mesh_store import sample_point_ids

    n = 500
    b = mesh_db.batched(resample_n_points=n, resample_seed=9)
    assert b.points.shape == (3, n, 3) and b.points.dtype == np.float32 and b.symmetries.shape == (3, 1, 4, 4)
    assert [b.infos[label]["n_points"] for label in b.labels] == [n, n, n] and b.labels.tolist() == ["obj_000001", "cloud", "tetra"]
    cloud = np.asarray(mesh_db.meshes["cloud"].vertices)
    assert np.array_equal(b.points[1], (cloud[sample_point_ids(len(cloud), n)] * 0.001).astype(np.float32))  # the host branch, beside surfaces
    meshes = [cases["golden"], EMPTY, cases["tetrahedron"]]
    pts, fid, _ = (a.cpu().numpy() for a in ops.mesh_sample_surface([m[0] for m in meshes], [m[1] for m in meshes], n, seed=9,
                                                                    return_face_ids=True, return_areas=True, device=DEV))
    for o, (name, scale) in {0: ("golden", 0.001), 2: ("tetrahedron", 0.05)}.items():
        assert np.array_equal(b.points[o], (pts[o].astype(np.float64) * scale).astype(np.float32)), name  # scale applied, object = position
        v, f = cases[name]
        a, bb, dist = R.barycentric(v, f, fid[o], pts[o])
        bound = R.point_bound(name, v)
        corners = v[f[fid[o]]].astype(np.float64)
        slack = bound / min(np.linalg.norm(corners[:, k] - corners[:, 0], axis=1).min() for k in (1, 2))  # the bound in edge lengths
        print(f"{name}: residual to the face plane {dist.max():.3e} (bound {bound:.3e}), barycentric min {min(a.min(), bb.min()):.3e} max sum {(a + bb).max():.9f}")
        assert dist.max() <= bound, (name, dist.max())
        assert a.min() >= -8 * slack and bb.min() >= -8 * slack and (a + bb).max() <= 1 + 8 * slack, name
    # the default seed is 0 and a second call repeats it
    assert np.array_equal(mesh_db.batched(resample_n_points=50).points, mesh_db.batched(resample_n_points=50, resample_seed=0).points)
    assert not np.array_equal(mesh_db.batched(resample_n_points=50).points[0], b.points[0, :50])
    # the no-argument call still is the padded vertex table
    assert mesh_db.batched().points.shape == (3, len(cases["golden"][0]), 3)


def test_batched_resample_fps(cases, mesh_db):
    from happypose_amd import ops

    n, over = 100, 8
    b = mesh_db.batched(resample_n_points=n, resample_method="fps", resample_oversample=over, resample_seed=4)
    meshes = [cases["golden"], EMPTY, cases["tetrahedron"]]
    drawn = ops.mesh_sample_surface([m[0] for m in meshes], [m[1] for m in meshes], n * over, seed=4, device=DEV)
    ids = ops.farthest_point_ids(drawn, torch.tensor([n * over, 0, n * over], dtype=torch.int32), n).cpu().numpy()
    drawn = drawn.cpu().numpy()
    assert (ids[1] == -1).all()
    for o, scale in {0: 0.001, 2: 0.05}.items():
        assert ids[o, 0] == 0 and len(np.unique(ids[o])) == n and ids[o].min() >= 0 and ids[o].max() < n * over  # a subset, the first sample starts it
        assert np.array_equal(b.points[o], (drawn[o, ids[o]].astype(np.float64) * scale).astype(np.float32))
        # farthest-point order: the second pick is the sample farthest from the first
        d = np.linalg.norm(drawn[o].astype(np.float64) - drawn[o, 0], axis=1)
        assert d[ids[o, 1]] >= d.max() * (1 - 1e-6)
    assert b.infos["obj_000001"]["n_points"] == n and b.points.shape == (3, n, 3)


def test_multiview_predictor_constructs_with_resampled_points(mesh_db):
    from happypose_amd.multiview import MultiviewScenePredictor

    pred = MultiviewScenePredictor(mesh_db, ba_aabb=False, ba_n_points=64, device=DEV)
    assert tuple(pred.mesh_db_ba.points.shape) == (3, 64, 3) and pred.mesh_db_ba.points.is_cuda
    assert torch.isfinite(pred.mesh_db_ba.points).all() and tuple(pred.mesh_db_ransac.points.shape) == (3, 8, 3)


# ---- ModelNetErrorMeter -------------------------------------------------------------------------------------------------------------
def _frames(g12):
    """Twelve frames with one object each: G12's poses (the pose-error bounds were measured on them)."""
    pred = np.concatenate([g12["small/TXO_pred"], g12["large/TXO_pred"]])
    gt = np.concatenate([g12["small/TXO_gt"], g12["large/TXO_gt"]])
    return pred, gt


def _collections(pred, gt, K, frame_of_pred):
    """Prediction ``k`` belongs to frame (view) ``frame_of_pred[k]``; ground truth ``j`` is frame ``j``."""
    from happypose_amd.tensor_collection import PandasTensorCollection

    n = len(gt)
    p_infos = pd.DataFrame({"scene_id": 3, "view_id": np.asarray(frame_of_pred), "label": "obj_000001", "score": 1.0})
    g_infos = pd.DataFrame({"scene_id": 3, "view_id": np.arange(n), "label": "obj_000001"})
    return (PandasTensorCollection(p_infos, poses=torch.as_tensor(pred[np.asarray(frame_of_pred)])),
            PandasTensorCollection(g_infos, poses=torch.as_tensor(gt), K=torch.as_tensor(np.tile(K, (n, 1, 1)))))


def test_modelnet_meter(golden_dir, mesh_db):
    from happypose_amd.evaluation import ModelNetErrorMeter

    g12 = np.load(golden_dir / "g12_pose_errors.npz")
    B = PR.bounds(g12)
    n_points = 1000
    assert n_points >= B["min_points"]  # the mean's bound was measured on rows of at least that many points
    from happypose_amd.mesh_store import MeshDataBase

    surfaces = MeshDataBase([mesh_db.obj_dict["obj_000001"], mesh_db.obj_dict["tetra"]])  # the cloud has fewer vertices than n_points
    meter = ModelNetErrorMeter(surfaces, sample_n_points=n_points, device=DEV)
    pred, gt = _frames(g12)
    order = np.random.RandomState(1).permutation(8)  # predictions arrive in another order than the ground truth
    meter.add(*_collections(pred[:8], gt[:8], g12["K"], order))
    meter.add(*_collections(pred[8:], gt[8:], g12["K"], np.arange(4)))
    summary, df = meter.summary()
    assert len(df) == 12 and set(summary) == {"add0.1d", "5deg_5cm", "proj2d_5px"}
    assert df["pred_id"].tolist() == list(range(8)) + list(range(4)) and df["gt_id"].tolist() == order.tolist() + list(range(4))
    pts = meter.mesh_db.points[0, :n_points].cpu().numpy()  # the object's own points, as the device holds them
    rows = []
    for k, (_, m) in enumerate(df.iterrows()):
        i = int(m["gt_id"]) + (0 if k < 8 else 8)  # the frame of the match
        r = R.modelnet_errors(pred[i], gt[i], g12["K"], pts)
        rows.append(r)
        # the trace form and the quaternion form agree on a rotation; G12's matrices are float32, 18 entries each within 6e-8 of one:
        # |q.q| may differ by 1.1e-6, the angle by 2 * 1.1e-6 / sin(angle / 2) (at the least the clamp's angle)
        ang_tol = np.rad2deg(2 * 1.1e-6 / max(np.sin(np.deg2rad(r["angular_dist"]) / 2), np.sin(np.arccos(1 - 1e-7))))
        print(f"frame {i}: add {m['add']:.6e} ({r['add']:.6e}), proj {m['proj_error']:.5f} ({r['proj_error']:.5f}), trans {m['trans_dist']:.6e} "
              f"({r['trans_dist']:.6e}), angle {m['angular_dist']:.6f} ({r['angular_dist']:.6f} +- {ang_tol:.1e}), diameter {m['diameter']:.7f} ({r['diameter']:.7f})")
        assert abs(m["add"] - r["add"]) <= B["norm_avg"], i
        assert abs(m["proj_error"] - r["proj_error"]) <= B["pixel"], i
        assert abs(m["trans_dist"] - r["trans_dist"]) <= B["norm_avg"], i
        # float32 extent and norm against float64: a few roundings of the format
        assert abs(m["diameter"] - r["diameter"]) <= 4 * np.spacing(np.float32(r["diameter"])), i
        assert abs(m["angular_dist"] - r["angular_dist"]) <= ang_tol, i
    assert summary == R.modelnet_summary(rows), (summary, R.modelnet_summary(rows))

    # two predictions for one ground truth raise; so does a ground truth without one
    two = _collections(pred[:3], gt[:3], g12["K"], [0, 1, 2, 0])
    with pytest.raises(AssertionError):
        ModelNetErrorMeter(meter.mesh_db, device=DEV).add(*two)
    with pytest.raises(AssertionError):
        ModelNetErrorMeter(meter.mesh_db, device=DEV).add(*_collections(pred[:3], gt[:3], g12["K"], [0, 1]))
