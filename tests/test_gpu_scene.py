"""GPU tests of the scene kernels (csrc/scene.hip) and of happypose_amd.scene.

The layers come from ``ops.rasterize``; the new kernels are compared with tests/scene_ref.py applied to those SAME layers by
exact equality -- compose copies values, visibility counts integers, contour and overlay are byte functions: no tolerance.
``render_scene`` end to end is compared with ``oracle.native.rasterize`` layers composed by scene_ref.py under the bounds of the
single-object comparisons of tests/test_gpu_kernels.py (``_close_to_oracle`` below).
"""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import scene_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

RESOLUTIONS = [(48, 64), (37, 50)]  # 37 x 50 = 1850 pixels: not a multiple of 4, every plane after the first starts unaligned


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dataset():
    from happypose_amd.synthetic import make_object_dataset

    return make_object_dataset(3, seed=1, tex_size=256)


@pytest.fixture(scope="module")
def store(dev, dataset):
    from happypose_amd.ops import MeshStore

    return MeshStore(dataset, dev)


def _pose(seed, t):
    from happypose_amd.synthetic import random_rotations

    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = random_rotations(np.random.RandomState(seed), 1)[0]
    T[:3, 3] = t
    return T


def _K(res, f):
    return np.array([[f, 0, res[1] / 2], [0, f, res[0] / 2], [0, 0, 1]], np.float32)


_CACHE = {}


def _scene_a(store, res, normals):
    """Three cameras with {0, 1, 5} layers.  Camera 1: one object so close that it touches all four borders.  Camera 2: an
    object, an identical copy (tie), the same object pushed back along its viewing ray (entirely hidden), a non-finite pose
    (a zero image) and another object in front of part of the first."""
    key = ("a", res, normals)
    if key not in _CACHE:
        from happypose_amd import ops

        P = _pose(3, (0.004, -0.003, 0.5))
        back = P.copy()
        back[:3, 3] *= 1.6
        nan = P.copy()
        nan[0, 3] = np.nan
        front = _pose(4, (0.03, 0.01, 0.38))
        T = np.stack([_pose(5, (0, 0, 0.3)), P, P, back, nan, front])
        obj = np.array([2, 0, 0, 0, 0, 1], np.int32)
        K = np.stack([_K(res, 400.0)] + [_K(res, 150.0)] * 5)
        rgb, nrm, dep, _ = ops.rasterize(store, torch.as_tensor(obj), torch.as_tensor(T), torch.as_tensor(K), res, render_normals=normals,
                                         render_depth=True, msaa=True, aniso=True)
        _CACHE[key] = (np.array([0, 0, 1, 6], np.int32), rgb, nrm, dep)
    return _CACHE[key]


def _scene_b(store, res=(48, 64)):
    """One camera, 33 layers (past any unroll or register-array bound), random poses that overlap in the middle of the frame."""
    key = ("b", res)
    if key not in _CACHE:
        from happypose_amd import ops

        rs = np.random.RandomState(7)
        T = np.stack([_pose(100 + i, (rs.uniform(-0.06, 0.06), rs.uniform(-0.05, 0.05), rs.uniform(0.4, 0.9))) for i in range(33)])
        obj = (np.arange(33) % 3).astype(np.int32)
        K = np.stack([_K(res, 150.0)] * 33)
        rgb, nrm, dep, _ = ops.rasterize(store, torch.as_tensor(obj), torch.as_tensor(T), torch.as_tensor(K), res, render_normals=True,
                                         render_depth=True, msaa=True, aniso=True)
        _CACHE[key] = (np.array([0, 33], np.int32), rgb, nrm, dep)
    return _CACHE[key]


def _np(t):
    return None if t is None else t.cpu().numpy()


def _assert_compose_equal(got, ref):
    for k in ("rgb", "normals", "depth", "ids", "mask"):
        if ref[k] is None:
            assert got[k] is None
            continue
        g = _np(got[k])
        assert g.dtype == ref[k].dtype and g.shape == ref[k].shape, k
        assert np.array_equal(g, ref[k]), (k, int((g != ref[k]).sum()))


# --------------------------------------------------------------------------------------------------------------------- compose
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_compose_three_cameras(store, res, normals):
    from happypose_amd import ops

    off, rgb, nrm, dep = _scene_a(store, res, normals)
    got = ops.scene_compose(off, rgb, nrm, dep)
    ref = R.compose(off, _np(rgb), _np(nrm), _np(dep))
    _assert_compose_equal(got, ref)
    # the scenario is what it claims to be (judged on the reference's answer)
    d = _np(dep)[:, 0]
    assert not ref["mask"][0].any() and (ref["ids"][0] == -1).all() and not ref["rgb"][0].any()      # a camera without layers
    assert np.array_equal(d[1], d[2]) and (d[1] > 0).sum() > 100 and not (ref["ids"][2] == 1).any()  # the tie goes to the lower layer
    assert (d[3] > 0).sum() > 50 and not (ref["ids"][2] == 2).any()                                  # entirely behind
    assert not d[4].any() and not (ref["ids"][2] == 3).any()                                         # the non-finite pose never wins
    both = (d[1] > 0) & (d[5] > 0)
    assert both.sum() > 50 and (ref["ids"][2][both] == 4).all() and (ref["ids"][2] == 0).sum() > 50   # real occlusion, both visible
    assert set(np.unique(ref["ids"][2])) == {-1, 0, 4}


def test_compose_33_layers(store):
    from happypose_amd import ops

    off, rgb, nrm, dep = _scene_b(store)
    got = ops.scene_compose(off, rgb, nrm, dep)
    ref = R.compose(off, _np(rgb), _np(nrm), _np(dep))
    _assert_compose_equal(got, ref)
    assert len(np.unique(ref["ids"])) > 8 and ref["ids"].max() == 32  # many winners, the last layer among them
    # a slice that starts on an odd layer: base pointers that are 16-byte aligned or not, same answer
    got1 = ops.scene_compose([0, 32], rgb[1:], nrm[1:], dep[1:])
    _assert_compose_equal(got1, R.compose([0, 32], _np(rgb)[1:], _np(nrm)[1:], _np(dep)[1:]))


# ------------------------------------------------------------------------------------------------------------------ visibility
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_visibility(store, res):
    from happypose_amd import ops

    for off, rgb, nrm, dep in (_scene_a(store, res, False), _scene_b(store) if res == (48, 64) else _scene_a(store, res, True)):
        h, w = dep.shape[2:]
        ids = ops.scene_compose(off, rgb, None, dep)["ids"]
        t1 = ops.scene_visibility(off, dep, ids)
        t2 = ops.scene_visibility(off, dep, ids)
        ref = R.visibility(off, _np(dep), _np(ids))
        assert t1.dtype == torch.int32 and tuple(t1.shape) == ref.shape
        assert np.array_equal(_np(t1), ref), (_np(t1).tolist(), ref.tolist())
        assert torch.equal(t1, t2)                                  # integer atomics: the same bits on every run
        if len(off) == 4:
            assert ref[0, 2:6].tolist() == [0, 0, w - 1, h - 1]     # touches all four borders
            assert ref[3, 0] > 50 and ref[3, 1] == 0 and ref[3, 6:].tolist() == [-1] * 4 and ref[3, 2] >= 0   # hidden: no visible box
            assert ref[4].tolist() == [0, 0] + [-1] * 8             # the zero image: both boxes empty
            assert 0 < ref[1, 1] < ref[1, 0]                        # partly occluded


# --------------------------------------------------------------------------------------------------------------------- contour
def _contour_cases(store, dev):
    """(name, ids [n, h, w] int32 numpy): composed scenes at both resolutions (camera 1's object touches the border), an empty
    map, a single pixel and a block in the corner, the last three on a 37 x 50 frame that no tile divides."""
    from happypose_amd import ops

    cases = []
    for res in RESOLUTIONS:
        off, rgb, nrm, dep = _scene_a(store, res, False)
        cases.append((f"scene{res}", _np(ops.scene_compose(off, rgb, None, dep)["ids"])))
    cases.append(("scene_b", _np(ops.scene_compose(*[_scene_b(store)[i] for i in (0, 1, 2, 3)])["ids"])))
    hand = -np.ones((3, 37, 50), np.int32)
    hand[1, 20, 49] = 0     # one pixel, on the right border
    hand[2, :9, :7] = 2     # a block in the corner, beside ...
    hand[2, 30:, 3:] = 5    # ... a block that touches three borders and crosses tile seams
    cases.append(("hand", hand))
    return cases


@pytest.mark.parametrize("dilate", [0, 1, 3])
def test_contour(store, dev, dilate):
    from happypose_amd import ops

    rs = np.random.RandomState(11)
    for name, ids in _contour_cases(store, dev):
        n, h, w = ids.shape
        frame = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
        t_frame, t_ids = torch.as_tensor(frame, device=dev), torch.as_tensor(ids, device=dev)
        mask = (ids >= 0).astype(np.uint8)
        runs = {"mask": ops.scene_contour(t_frame, mask=torch.as_tensor(mask, device=dev)[:, None], color=(0, 255, 0), dilate_iterations=dilate),
                "ids": ops.scene_contour(t_frame, ids=t_ids, color=(7, 8, 9), dilate_iterations=dilate),
                "per_object": ops.scene_contour(t_frame, ids=t_ids, per_object=True, color=(255, 0, 255), dilate_iterations=dilate)}
        labels = {"mask": np.where(ids >= 0, 0, -1), "ids": np.where(ids >= 0, 0, -1), "per_object": ids}
        colors = {"mask": (0, 255, 0), "ids": (7, 8, 9), "per_object": (255, 0, 255)}
        for mode, (out, edge) in runs.items():
            for i in range(n):
                want_out, want_edge = R.contour(frame[i], labels[mode][i], colors[mode], dilate)
                assert np.array_equal(_np(edge[i]), want_edge), (name, mode, i, dilate)
                assert np.array_equal(_np(out[i]), want_out), (name, mode, i, dilate)
        assert torch.equal(t_frame, torch.as_tensor(frame, device=dev))   # the input frame is not written
        if name == "hand":
            e = _np(runs["mask"][1])
            assert not e[0].any() and np.array_equal(_np(runs["mask"][0][0]), frame[0])      # empty mask: a plain copy
            assert (e[1] > 0).sum() == (dilate + 1) * (2 * dilate + 1)                        # one pixel on the border, dilated and clipped
        if name == "scene_b" and dilate == 0:
            assert (_np(runs["per_object"][1]) > 0).sum() > (_np(runs["ids"][1]) > 0).sum()   # seams between objects are outlined too
    out_only, none = ops.scene_contour(t_frame, ids=t_ids, dilate_iterations=dilate, return_edge=False)
    assert none is None and out_only.shape == t_frame.shape
    with pytest.raises(AssertionError, match="dilate_iterations"):
        ops.scene_contour(t_frame, ids=t_ids, dilate_iterations=4)


# --------------------------------------------------------------------------------------------------------------------- overlay
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_overlay(store, dev, res):
    from happypose_amd import ops
    from happypose_amd import scene as S

    off, rgb, nrm, dep = _scene_a(store, res, False)
    comp = ops.scene_compose(off, rgb, None, dep)
    render = S._to_u8_hwc(comp["rgb"])
    mask = _np(comp["mask"])[:, 0].astype(bool)
    render_np = _np(render).copy()
    rs = np.random.RandomState(5)
    holes = mask & (rs.rand(*mask.shape) < 0.2)
    render_np[holes] = 0                      # black texels inside the object: the two mask sources differ there
    assert holes.sum() > 20
    frame = rs.randint(0, 256, render_np.shape).astype(np.uint8)
    lut_r, lut_i = (torch.as_tensor(t) for t in S.overlay_tables())
    t_in, t_r = torch.as_tensor(frame, device=dev), torch.as_tensor(render_np, device=dev)
    got_rgb = _np(ops.scene_overlay(t_in, t_r, lut_r, lut_i))
    got_msk = _np(ops.scene_overlay(t_in, t_r, lut_r, lut_i, mask=comp["mask"]))
    for i in range(len(frame)):
        assert np.array_equal(got_rgb[i], R.overlay(frame[i], render_np[i]))
        assert np.array_equal(got_msk[i], R.overlay(frame[i], render_np[i], mask=mask[i]))
    assert (got_rgb != got_msk).any()
    # the numpy front-end
    assert np.array_equal(S.make_overlay(frame[2], render_np[2], device=dev), got_rgb[2])
    assert np.array_equal(S.make_overlay(frame[2], render_np[2], mask=mask[2], device=dev), got_msk[2])


# ------------------------------------------------------------------------------------------------------------- render_scene
E2E_RES = (120, 160)


def _e2e_scene():
    """Three objects that overlap in both views, more than 5 cm apart in depth.  Chosen on the CPU with the oracle alone: its
    id maps show every object as a winner in both cameras, the composed depth differs from every object's own layer (each
    object hides or is hidden somewhere), and at most a handful of pixels have two objects within 1 mm of each other."""
    from happypose_amd import scene as S

    objects = [S.Panda3dObjectData("obj_000001", TWO=_pose(21, (0.0, 0.0, 0.55))),
               S.Panda3dObjectData("obj_000002", TWO=_pose(22, (0.05, 0.02, 0.70)), color=(1, 1, 1, 1)),
               {"name": "obj_000003", "TWO": _pose(23, (-0.05, -0.03, 0.85))}]
    TWC1 = np.eye(4)
    a = np.deg2rad(12.0)
    TWC1[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    TWC1[:3, 3] = (-0.14, 0.01, 0.0)
    cameras = [S.Panda3dCameraData(K=_K(E2E_RES, 260.0), resolution=E2E_RES), S.Panda3dCameraData(K=_K(E2E_RES, 240.0), resolution=E2E_RES, TWC=TWC1)]
    return objects, cameras


def _oracle_scene(packed, objects, cameras, lights, msaa, aniso):
    """The same scene from ``oracle.native.rasterize`` layers composed by scene_ref.py."""
    from happypose_amd import scene as S
    from oracle import native

    objs = [S._object_data(o) for o in objects]
    (g,) = S.plan_layers(objs, cameras)
    oid = np.array([packed.label_to_id[o.label] for o in objs], np.int32)
    center, radius = S.scene_bounds(packed.bounds_center[oid], packed.bounds_radius[oid], [o.TWO for o in objs])
    amb, pos_w, col = S.scene_lights(lights, center, radius)
    pos = S.light_positions_in_object_frames(pos_w, [o.TWO for o in objs])[g.layer_object]
    L = len(g.layer_object)
    ref = native.rasterize(packed, oid[g.layer_object], g.TCO, g.K, g.resolution, True, True, False, ambient=np.tile(amb[None], (L, 1)),
                           light_pos=pos, light_col=np.tile(col[None], (L, 1, 1)), msaa=msaa, aniso=aniso)
    return g, ref, R.compose(g.layer_off, ref["rgbs"], ref["normals"], ref["depths"])


def _close_to_oracle(got, ref, msaa):
    """The bounds of the single-object comparisons in tests/test_gpu_kernels.py, on a composed scene.  Geometry as in
    ``_compare_renders``: ids (there: coverage) may differ on at most 5e-4 of the pixels; where they agree, depth differs by more
    than 1e-6 on fewer than 1e-3 of them and never by 5e-3.  Colours and normals where the ids agree: single-sampled as in
    ``_compare_renders`` (within 1.01 / 255 everywhere, different at all on fewer than 2e-3), multisampled + anisotropic as in
    the oracle tests of that state (more than 1.5 / 255 apart on fewer than 2e-3, never more than one sample pair's share, 0.5)."""
    ids, rid = _np(got["ids"]), ref["ids"]
    mism = ids != rid
    print(f"ids mismatch {mism.mean():.2e}")
    assert mism.mean() <= 5e-4, f"ids mismatch {mism.mean():.2e}"
    ok = ~mism
    assert np.array_equal(_np(got["mask"])[:, 0][ok], ref["mask"][:, 0][ok])
    dd = np.abs(_np(got["depth"]) - ref["depth"])[:, 0][ok]
    print(f"depth: max {dd.max():.2e}, fraction > 1e-6 {(dd > 1e-6).mean():.2e}")
    assert (dd > 1e-6).mean() < 1e-3 and dd.max() < 5e-3
    for k in ("rgb", "normals"):
        d = np.abs(_np(got[k]) - ref[k]).max(1)[ok]
        print(f"{k}: max {d.max():.3f}, fraction > 1e-6 {(d > 1e-6).mean():.2e}, fraction > 1.5/255 {(d > 1.5 / 255).mean():.2e}")
        if msaa:
            assert (d > 1.5 / 255).mean() < 2e-3 and d.max() <= 0.5 + 1e-6, k
        else:
            assert d.max() <= 1.01 / 255 and (d > 1e-6).mean() < 2e-3, k


@pytest.mark.parametrize("msaa", [False, True])
def test_render_scene_vs_oracle(store, msaa):
    from happypose_amd import scene as S
    from happypose_amd.renderer import make_scene_lights

    objects, cameras = _e2e_scene()
    lights = make_scene_lights()
    key = ("oracle", msaa)
    if key not in _CACHE:
        _CACHE[key] = _oracle_scene(store.packed, objects, cameras, lights, msaa, msaa)
    g, layers, ref = _CACHE[key]
    # the scene does what the docstring of _e2e_scene says (on the oracle's answer alone)
    d = layers["depths"][:, 0]
    for c in range(2):
        assert set(np.unique(ref["ids"][c])) == {-1, 0, 1, 2}
        for j in range(3):
            assert (ref["depth"][c, 0] != d[3 * c + j]).any() and (ref["ids"][c] == j).sum() > 100
        for a in range(3):
            for b in range(a + 1, 3):
                both = (d[3 * c + a] > 0) & (d[3 * c + b] > 0)
                assert (np.abs(d[3 * c + a] - d[3 * c + b])[both] < 1e-3).sum() <= 5
    renderer = S.SceneRenderer(store=store, msaa=msaa, aniso=msaa)
    (got,) = renderer.render_scene_tensors(objects, cameras, lights, render_normals=True, render_depth=True)
    assert got["cameras"] == [0, 1] and got["layer_camera"].tolist() == [0, 0, 0, 1, 1, 1] and got["layer_object"].tolist() == [0, 1, 2] * 2
    _close_to_oracle(got, ref, msaa)


def test_render_scene_types_chunks_and_visibility(store, dataset):
    from happypose_amd import scene as S
    from happypose_amd.renderer import BatchRenderer, make_scene_lights

    objects, cameras = _e2e_scene()
    lights = make_scene_lights()
    h, w = E2E_RES
    renderer = S.SceneRenderer(renderer=BatchRenderer(dataset, store=store))
    assert renderer.store is store and renderer.msaa and renderer.aniso
    (full,) = renderer.render_scene_tensors(objects, cameras, lights, render_normals=True, render_depth=True)
    # CameraRenderingData as the reference returns it
    out = renderer.render_scene(objects, cameras, lights, render_normals=True, render_depth=True, render_binary_mask=True)
    assert len(out) == 2 and all(isinstance(o, S.CameraRenderingData) for o in out)
    for i, o in enumerate(out):
        assert o.rgb.shape == (h, w, 3) and o.rgb.dtype == np.uint8 and o.normals.shape == (h, w, 3) and o.normals.dtype == np.uint8
        assert o.depth.shape == (h, w, 1) and o.depth.dtype == np.float32 and o.binary_mask.shape == (h, w, 1) and o.binary_mask.dtype == np.bool_
        assert np.array_equal(o.binary_mask, o.depth > 0) and o.binary_mask.any()
        assert np.array_equal(o.rgb, np.round(_np(full["rgb"][i]).transpose(1, 2, 0) * 255).astype(np.uint8))
        assert np.array_equal(o.depth[..., 0], _np(full["depth"][i, 0]))
    plain = renderer.render_scene(objects, cameras[:1], lights)[0]
    assert plain.normals is None and plain.depth is None and plain.binary_mask is None and np.array_equal(plain.rgb, out[0].rgb)
    # chunked rendering: a camera's three layers one at a time (3 chunks per camera), then whole cameras one at a time
    layer_bytes = h * w * 4 * 7
    for budget in (layer_bytes, 3 * layer_bytes):
        small = S.SceneRenderer(store=store, layer_budget_bytes=budget)
        (part,) = small.render_scene_tensors(objects, cameras, lights, render_normals=True, render_depth=True)
        for k in ("rgb", "normals", "depth", "ids", "mask"):
            assert torch.equal(part[k], full[k]), (budget, k)
    # gt-info of the scene
    df = renderer.scene_visibility(objects, cameras)
    assert list(df.columns) == ["cam_id", "obj_id", "label", "px_count_all", "px_count_visib", "visib_fract", "bbox_obj", "bbox_visib"]
    assert df[["cam_id", "obj_id"]].values.tolist() == [[c, j] for c in range(2) for j in range(3)]
    ids = _np(full["ids"])
    for _, row in df.iterrows():
        m = ids[row.cam_id] == row.obj_id
        ys, xs = np.nonzero(m)
        assert row.px_count_visib == m.sum() and 0 < row.px_count_visib <= row.px_count_all
        assert row.bbox_visib == (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1)
        assert row.visib_fract == row.px_count_visib / row.px_count_all
    assert (df.visib_fract < 1).any()
    # an empty scene is a black frame
    (empty,) = renderer.render_scene([], cameras[:1], lights, render_depth=True, render_binary_mask=True)
    assert not empty.rgb.any() and not empty.depth.any() and not empty.binary_mask.any()


def test_make_poses_visualization_writes_the_three_images(store, dataset, tmp_path):
    from PIL import Image

    from happypose_amd import scene as S

    objects, cameras = _e2e_scene()
    h, w = E2E_RES
    rgb = np.random.RandomState(3).randint(0, 256, (h, w, 3)).astype(np.uint8)
    renderer = S.SceneRenderer(store=store)
    paths = S.make_poses_visualization(rgb, dataset, objects, cameras[0], tmp_path / "visualizations", renderer=renderer)
    assert sorted(p.name for p in paths.values()) == ["all_results.png", "contour_overlay.png", "mesh_overlay.png"]
    mesh, contour, both = (np.array(Image.open(tmp_path / "visualizations" / n)) for n in ("mesh_overlay.png", "contour_overlay.png", "all_results.png"))
    assert mesh.shape == contour.shape == (h, w, 3) and both.shape == (h, 3 * w, 3)
    assert np.array_equal(both, np.concatenate([rgb, contour, mesh], 1))
    render = renderer.render_scene(objects, cameras[:1], S._ambient_white())[0].rgb
    assert np.array_equal(mesh, R.overlay(rgb, render))
    want = R.contour(rgb, np.where((render > 0).any(-1), 0, -1), (0, 255, 0), 1)
    res = S.make_contour_overlay(rgb, render, dilate_iterations=1)
    assert np.array_equal(contour, want[0]) and np.array_equal(res["img"], want[0]) and np.array_equal(res["canny"], want[1])
    assert res["mask"].dtype == np.bool_ and np.array_equal(res["mask"], (render > 0).any(-1)) and (want[1] > 0).sum() > 50
    # the single-view helper: poses in the camera frame, the reference's dict camera
    import pandas as pd

    from happypose_amd.tensor_collection import PandasTensorCollection

    objs = [S._object_data(o) for o in objects]
    pred = PandasTensorCollection(infos=pd.DataFrame(dict(label=[o.label for o in objs])), poses=torch.as_tensor(np.stack([o.TWO for o in objs])).float())
    again = S.render_prediction_wrt_camera(renderer, pred, camera=dict(K=cameras[0].K, TWC=np.full((4, 4), 7.0)), resolution=(w, h))
    assert np.array_equal(again, render)
