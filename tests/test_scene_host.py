"""Host-side checks of the scene renderer (happypose_amd/scene.py, csrc/scene.hip): layer bookkeeping, guards, overlay tables,
light transforms and the argument errors of the four hp_scene_* entry points.  No GPU."""

import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import scene_ref as R  # noqa: E402

from happypose_amd import scene as S  # noqa: E402
from happypose_amd.renderer import Panda3dLightData, make_scene_lights  # noqa: E402


def _pose(seed, t):
    from happypose_amd.synthetic import random_rotations

    T = np.eye(4)
    T[:3, :3] = random_rotations(np.random.RandomState(seed), 1)[0]
    T[:3, 3] = t
    return T


K0 = np.array([[600.0, 0, 32], [0, 600.0, 24], [0, 0, 1]])


@pytest.mark.parametrize("n_obj", [0, 1, 4])
def test_layer_plan_order_offsets_and_TCO(n_obj):
    objects = [S.Panda3dObjectData(label=f"o{j}", TWO=_pose(j, (0.01 * j, 0, 0.5))) for j in range(n_obj)]
    cameras = [S.Panda3dCameraData(K=K0 * (1 + i), resolution=(48, 64), TWC=_pose(10 + i, (0.1 * i, 0.02, -0.1))) for i in range(3)]
    (g,) = S.plan_layers(objects, cameras)
    assert g.resolution == (48, 64) and g.cameras == [0, 1, 2]
    assert g.layer_off.tolist() == [0, n_obj, 2 * n_obj, 3 * n_obj] and g.layer_off.dtype == np.int32
    assert g.layer_camera.tolist() == [i for i in range(3) for _ in range(n_obj)]
    assert g.layer_object.tolist() == [j for _ in range(3) for j in range(n_obj)]
    assert g.TCO.shape == (3 * n_obj, 4, 4) and g.TCO.dtype == np.float32 and g.K.shape == (3 * n_obj, 3, 3)
    for i in range(3):
        for j in range(n_obj):
            want = np.linalg.inv(cameras[i].TWC) @ objects[j].TWO
            np.testing.assert_allclose(g.TCO[i * n_obj + j], want, atol=1e-6)
            np.testing.assert_array_equal(g.K[i * n_obj + j], (K0 * (1 + i)).astype(np.float32))


def test_layer_plan_groups_cameras_by_resolution():
    objects = [{"name": "a", "TWO": np.eye(4), "color": (1, 1, 1, 1)}, {"name": "b", "TWO": _pose(1, (0, 0, 1))}]
    res = [(48, 64), (37, 50), (48, 64), (37, 50), (48, 64)]
    cameras = [dict(K=K0, resolution=r, TWC=_pose(20 + i, (0, 0, 0))) for i, r in enumerate(res)]
    groups = S.plan_layers(objects, cameras)
    assert [(g.resolution, g.cameras) for g in groups] == [((48, 64), [0, 2, 4]), ((37, 50), [1, 3])]
    assert groups[0].layer_off.tolist() == [0, 2, 4, 6] and groups[1].layer_off.tolist() == [0, 2, 4]
    assert groups[1].layer_camera.tolist() == [1, 1, 3, 3] and groups[1].layer_object.tolist() == [0, 1, 0, 1]
    np.testing.assert_allclose(groups[1].TCO[3], np.linalg.inv(_pose(23, (0, 0, 0))) @ _pose(1, (0, 0, 1)), atol=1e-6)


def test_pose_inputs_accepted():
    quat = S.Panda3dObjectData("a", TWO=((0.0, 0.0, 0.0, 1.0), (0.1, 0.2, 0.3)))
    want = np.eye(4)
    want[:3, 3] = (0.1, 0.2, 0.3)
    np.testing.assert_array_equal(quat.TWO, want)
    T = _pose(3, (0, 0, 1))
    assert np.array_equal(S.Panda3dObjectData("a", TWO=SimpleNamespace(toHomogeneousMatrix=lambda: T)).TWO, T)
    assert np.array_equal(S.Panda3dObjectData("a", TWO=torch.as_tensor(T)).TWO, T)
    d = S.Panda3dObjectData("a")
    assert np.array_equal(d.TWO, np.eye(4)) and d.color is None and d.scale == 1 and d.material is None and not d.remove_mesh_material
    c = S.Panda3dCameraData(K=K0, resolution=(4, 5))
    assert np.array_equal(c.TWC, np.eye(4)) and c.z_near == 0.1 and c.z_far == 10 and c.node_name == "camera" and c.positioning_function is None


@pytest.mark.parametrize("obj_kw,cam_kw", [
    (dict(scale=2.0), {}), (dict(material=object()), {}), (dict(color=(1, 0, 0, 1)), {}), (dict(color=(1, 1, 1, 0.5)), {}),
    (dict(positioning_function=lambda r, n: None), {}), ({}, dict(z_near=0.01)), ({}, dict(z_far=100.0)),
    ({}, dict(positioning_function=lambda r, n: None))])
def test_unsupported_scene_features_raise(obj_kw, cam_kw):
    objects = [S.Panda3dObjectData("a", **obj_kw)]
    cameras = [S.Panda3dCameraData(K=K0, resolution=(48, 64), **cam_kw)]
    with pytest.raises(NotImplementedError):
        S._check_supported(objects, cameras)
    # and through the public call, before anything touches a device
    r = S.SceneRenderer.__new__(S.SceneRenderer)
    with pytest.raises(NotImplementedError):
        r.render_scene_tensors(objects, cameras, [])


def test_supported_scene_passes_the_guards_and_mask_needs_depth():
    S._check_supported([S.Panda3dObjectData("a", color=(1, 1, 1, 1)), S.Panda3dObjectData("b")], [S.Panda3dCameraData(K=K0, resolution=(4, 4))])
    r = S.SceneRenderer.__new__(S.SceneRenderer)
    with pytest.raises(AssertionError, match="Binary mask"):
        r.render_scene([S.Panda3dObjectData("a")], [S.Panda3dCameraData(K=K0, resolution=(4, 4))], [], render_binary_mask=True)
    with pytest.raises(AssertionError, match="Binary mask"):
        r.render_scene_tensors([], [], [], render_binary_mask=True)


def test_overlay_tables_are_the_reference_expression():
    lut_render, lut_input = S.overlay_tables()
    assert lut_render.dtype == np.uint8 and lut_input.dtype == np.uint8 and lut_render.shape == lut_input.shape == (256,)
    v = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, -1)
    # the reference's code on an image holding every byte value: all rendered (render branch), none rendered (input branch)
    got_render = R.overlay(np.zeros_like(v), v, mask=np.ones((16, 16), bool))
    got_input = R.overlay(v, np.zeros_like(v), mask=np.zeros((16, 16), bool))
    assert np.array_equal(lut_render, got_render[..., 0].reshape(-1)) and np.array_equal(lut_input, got_input[..., 0].reshape(-1))
    assert lut_render[0] == 51 and lut_render[255] == 255 and lut_input[0] == 102 and lut_input[255] == 255


def test_scene_from_predictions():
    from happypose_amd.tensor_collection import PandasTensorCollection

    TWO = torch.stack([torch.as_tensor(_pose(i, (0.1 * i, 0, 0))) for i in range(3)]).float()
    TWC = torch.stack([torch.as_tensor(_pose(5 + i, (0, 0.1 * i, -1))) for i in range(2)]).float()
    K = torch.as_tensor(np.stack([K0, 2 * K0])).float()
    preds = {"scene/objects": PandasTensorCollection(infos=pd.DataFrame(dict(label=["a", "b", "a"], view_group=[0, 0, 1])), TWO=TWO),
             "scene/cameras": PandasTensorCollection(infos=pd.DataFrame(dict(view_id=[3, 7], view_group=[0, 0])), TWC=TWC, K=K)}
    with pytest.raises(AssertionError, match="view_group"):
        S.scene_from_predictions(preds, (48, 64))
    objs, cams = S.scene_from_predictions(preds, (48, 64), view_group=0)
    assert [o.label for o in objs] == ["a", "b"] and all(isinstance(o, S.Panda3dObjectData) for o in objs)
    np.testing.assert_array_equal(objs[1].TWO, TWO[1].numpy().astype(np.float64))
    assert len(cams) == 2 and all(c.resolution == (48, 64) for c in cams)
    np.testing.assert_array_equal(cams[1].TWC, TWC[1].numpy().astype(np.float64))
    np.testing.assert_array_equal(cams[1].K, 2 * K0)
    _, cams = S.scene_from_predictions(preds, [(48, 64), (37, 50)], view_group=0)
    assert [c.resolution for c in cams] == [(48, 64), (37, 50)]
    (g0, g1) = S.plan_layers(objs, cams)
    assert g0.cameras == [0] and g1.cameras == [1]


def test_point_light_moves_into_each_object_frame():
    p_w = np.array([[0.3, -0.2, 1.5]])
    Ta = np.eye(4)
    Ta[:3, 3] = (0.1, 0.0, 0.5)                    # a pure translation: the light moves by -t
    Tb = np.eye(4)
    Tb[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]  # 90 degrees about z, then a translation
    Tb[:3, 3] = (0.0, 0.2, 1.0)
    pos = S.light_positions_in_object_frames(p_w, [Ta, Tb])
    assert pos.shape == (2, 1, 3) and pos.dtype == np.float32
    np.testing.assert_allclose(pos[0, 0], [0.2, -0.2, 1.0], atol=1e-6)
    np.testing.assert_allclose(pos[1, 0], [-0.4, -0.3, 0.5], atol=1e-6)   # R^T (p - t)
    for T, q in ((Ta, pos[0, 0]), (Tb, pos[1, 0])):                       # and back: TWO @ q is the world position
        np.testing.assert_allclose(T[:3, :3] @ q + T[:3, 3], p_w[0], atol=1e-6)


def test_scene_lights_use_the_union_of_the_object_spheres():
    Ta, Tb = np.eye(4), np.eye(4)
    Tb[:3, 3] = (1.0, 0, 0)
    c, r = S.scene_bounds(np.zeros((2, 3)), np.array([0.1, 0.3]), [Ta, Tb])
    np.testing.assert_allclose(c, [0.6, 0, 0], atol=1e-12)               # spans x in [-0.1, 1.3]
    assert abs(r - 0.7) < 1e-12
    c1, r1 = S.scene_bounds(np.array([[0.0, 0, 0], [0.01, 0, 0]]), np.array([0.5, 0.1]), [Ta, Ta])
    assert np.allclose(c1, 0) and r1 == 0.5                                # a sphere inside the other changes nothing
    assert S.scene_bounds(np.zeros((0, 3)), np.zeros(0), [])[1] == 0.0
    amb, pos, col = S.scene_lights(make_scene_lights(), c, r)
    np.testing.assert_allclose(amb, [0.1, 0.1, 0.1])
    assert pos.shape == (6, 3) and col.shape == (6, 3)
    np.testing.assert_allclose(pos[0], [7.0, 0, 0])                        # the reference's pos_fn: direction * radius * 10
    np.testing.assert_allclose(pos[5], [0, 0, -7.0])
    with pytest.raises(NotImplementedError):
        S.scene_lights([Panda3dLightData("directional")], c, r)
    with pytest.raises(AssertionError):
        S.scene_lights([Panda3dLightData("point")], c, r)


def test_scene_argument_errors_reported_without_gpu():
    from happypose_amd import _ffi

    lib = _ffi.lib()
    p = 4096  # never dereferenced: every call below is refused before a launch
    # a NULL buffer
    assert lib.hp_scene_compose(1, p, 1, 4, 4, p, None, p, None, None, p, p, p, None) == -1 and b"hp_scene_compose" in lib.hp_last_error()
    assert lib.hp_scene_compose(1, p, 1, 4, 4, None, None, p, p, None, p, p, p, None) == -1
    assert lib.hp_scene_compose(1, p, 1, 4, 4, p, None, p, p, p, p, p, p, None) == -1      # normals out without layer normals
    assert lib.hp_scene_visibility(1, p, 1, 4, 4, p, p, None, None) == -1 and b"hp_scene_visibility" in lib.hp_last_error()
    assert lib.hp_scene_contour(1, 4, 4, None, p, None, 0, 0, 255, 0, 1, p, None, None) == -1 and b"hp_scene_contour" in lib.hp_last_error()
    assert lib.hp_scene_contour(1, 4, 4, p, None, None, 0, 0, 255, 0, 1, p + 64, None, None) == -1   # neither mask nor ids
    assert lib.hp_scene_contour(1, 4, 4, p, p, p, 0, 0, 255, 0, 1, p + 64, None, None) == -1         # both
    assert lib.hp_scene_contour(1, 4, 4, p, p, None, 1, 0, 255, 0, 1, p + 64, None, None) == -1      # per_object without ids
    assert lib.hp_scene_contour(1, 4, 4, p, p, None, 0, 0, 255, 0, 1, p, None, None) == -1           # in place
    assert lib.hp_scene_contour(1, 4, 4, p, p, None, 0, 0, 256, 0, 1, p + 64, None, None) == -1      # colour outside a byte
    assert lib.hp_scene_overlay(1, 4, 4, p, p, None, None, p, p, None) == -1 and b"hp_scene_overlay" in lib.hp_last_error()
    # dilate_iterations outside 0..3
    for d in (4, -1):
        assert lib.hp_scene_contour(1, 4, 4, p, p, None, 0, 0, 255, 0, d, p + 64, None, None) == -1
        assert b"dilate_iterations" in lib.hp_last_error()
    # a negative n_cam, non-positive frame sizes
    assert lib.hp_scene_compose(-1, p, 0, 4, 4, p, None, p, p, None, p, p, p, None) == -1 and b"n_cam" in lib.hp_last_error()
    assert lib.hp_scene_visibility(-1, p, 1, 4, 4, p, p, p, None) == -1 and b"n_cam" in lib.hp_last_error()
    assert lib.hp_scene_contour(-1, 4, 4, p, p, None, 0, 0, 255, 0, 1, p + 64, None, None) == -1 and b"n_cam" in lib.hp_last_error()
    assert lib.hp_scene_overlay(-1, 4, 4, p, p, None, p, p, p, None) == -1 and b"n_cam" in lib.hp_last_error()
    assert lib.hp_scene_compose(1, p, -1, 4, 4, p, None, p, p, None, p, p, p, None) == -1
    assert lib.hp_scene_compose(1, p, 1, 0, 4, p, None, p, p, None, p, p, p, None) == -1
    assert lib.hp_scene_overlay(1, 4, 0, p, p, None, p, p, p, None) == -1
    with pytest.raises(AssertionError):
        _ffi.check(-1, "hp_scene_overlay")
    # nothing to do is not an error and launches nothing
    assert lib.hp_scene_compose(0, None, 0, 4, 4, None, None, None, None, None, None, None, None, None) == 0
    assert lib.hp_scene_visibility(0, None, 0, 4, 4, None, None, None, None) == 0
    assert lib.hp_scene_contour(0, 4, 4, p, p, None, 0, 0, 255, 0, 1, p + 64, None, None) == 0
    assert lib.hp_scene_overlay(0, 4, 4, p, p, None, p, p, p, None) == 0


def test_reference_contour_definition_on_a_hand_made_mask():
    """tests/scene_ref.py is the specification of the contour: pin it on a case small enough to check by eye."""
    lab = -np.ones((5, 6), np.int32)
    lab[1:4, 1:5] = 0                      # a 3 x 4 block: its ring is the edge, the two centre pixels are not
    frame = np.zeros((5, 6, 3), np.uint8)
    out, e = R.contour(frame, lab, (0, 255, 0), 0)
    want = np.zeros((5, 6), bool)
    want[1:4, 1:5] = True
    want[2, 2:4] = False
    assert np.array_equal(e > 0, want) and np.array_equal(out[..., 1] == 255, want) and set(np.unique(e)) == {0, 255}
    _, e1 = R.contour(frame, lab, (0, 255, 0), 1)
    assert e1.all()                        # every pixel of the 5 x 6 frame is within distance 1 of the ring
    full = np.zeros((4, 4), np.int32)      # the region fills the image: the border is not an edge
    assert not R.contour(np.zeros((4, 4, 3), np.uint8), full, (1, 2, 3), 3)[1].any()
    two = np.zeros((2, 4), np.int32)
    two[:, 2:] = 1                         # per-object labels: both sides of the seam are edges
    assert (R.contour(np.zeros((2, 4, 3), np.uint8), two, (1, 2, 3), 0)[1] > 0).tolist() == [[False, True, True, False]] * 2
