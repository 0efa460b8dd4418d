"""CPU tests of the host-side mirror of the reference interfaces (no GPU, no HIP calls)."""

import io
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

from happypose_amd import mesh_io, mesh_store
from happypose_amd.pose_estimator import (InferenceConfig, ObservationTensor, add_instance_id,
                                          assert_detections_valid, filter_detections, load_SO3_grid,
                                          make_detections_from_object_data)
from happypose_amd.tensor_collection import PandasTensorCollection, TensorCollection, concatenate


def test_tensor_collection_semantics():
    tc = TensorCollection(a=torch.arange(6).view(3, 2), b=torch.ones(3))
    assert tc.a.shape == (3, 2) and set(tc.tensors) == {"a", "b"}
    sub = tc[[0, 2]]
    assert sub.a.tolist() == [[0, 1], [4, 5]]
    tc.a = tc.a + 1  # assigning a registered name replaces the tensor
    assert tc.tensors["a"][0, 0] == 1
    with pytest.raises(AttributeError):
        tc.missing
    df = pd.DataFrame({"label": ["x", "y", "z"], "batch_im_id": [0, 0, 1]}, index=[5, 6, 7])
    p = PandasTensorCollection(df, poses=torch.eye(4).repeat(3, 1, 1))
    assert len(p) == 3 and p.infos.index.tolist() == [0, 1, 2]  # index is reset like the reference
    q = p[[2, 0]]
    assert q.infos.label.tolist() == ["z", "x"] and q.poses.shape == (2, 4, 4)
    c = concatenate([p, q, p[[]]])
    assert len(c) == 5 and c.infos.index.tolist() == list(range(5))
    assert len(concatenate([])) == 0
    import pickle

    r = pickle.loads(pickle.dumps(p))
    assert r.infos.equals(p.infos) and torch.equal(r.poses, p.poses)
    cl = p.clone()
    cl.poses[0, 0, 0] = 5
    assert p.poses[0, 0, 0] == 1


def test_detection_helpers():
    det = make_detections_from_object_data(["a", "b", "a"], np.array([[0, 0, 10, 10], [5, 5, 20, 20], [1, 1, 2, 2.0]]))
    assert_detections_valid(det)
    assert det.bboxes.dtype == torch.float32
    df = pd.DataFrame({"label": ["a", "b", "a", "a"], "batch_im_id": [0, 0, 0, 1]})
    d2 = add_instance_id(PandasTensorCollection(df, bboxes=torch.zeros(4, 4)))
    assert d2.infos.instance_id.tolist() == [0, 0, 1, 0]
    f = filter_detections(det, labels=["a"])
    assert f.infos.label.tolist() == ["a", "a"] and f.bboxes.shape == (2, 4)
    det.infos["score"] = [0.2, 0.9, 0.8]
    g = filter_detections(det, one_instance_per_class=True)
    assert sorted(g.infos.score.tolist()) == [0.8, 0.9]
    with pytest.raises(AssertionError):
        assert_detections_valid(PandasTensorCollection(pd.DataFrame({"label": ["a"]}), bboxes=torch.zeros(1, 4)))


def test_observation_tensor():
    rgb = (np.random.RandomState(0).rand(48, 64, 3) * 255).astype(np.uint8)
    depth = np.random.RandomState(1).rand(48, 64).astype(np.float32)
    K = np.array([[60.0, 0, 32], [0, 60, 24], [0, 0, 1]])
    o = ObservationTensor.from_numpy(rgb, depth, K)
    assert o.images.shape == (1, 4, 48, 64) and o.K.shape == (1, 3, 3) and o.is_valid()
    assert o.channel_dim == 4 and o.batch_size == 1 and o.depth.shape == (1, 48, 64)
    assert torch.allclose(o.images[0, :3], torch.as_tensor(rgb).permute(2, 0, 1).float() / 255)
    assert not ObservationTensor(o.images * 255, o.K).is_valid()  # rgb must be in [0,1]
    ob = ObservationTensor.from_torch_batched(torch.as_tensor(rgb).permute(2, 0, 1)[None], None, torch.as_tensor(K)[None])
    assert ob.images.shape == (1, 3, 48, 64)
    cfg = InferenceConfig()
    assert (cfg.n_refiner_iterations, cfg.n_pose_hypotheses, cfg.bsz_objects, cfg.bsz_images, cfg.SO3_grid_size) == (5, 5, 16, 576, 576)


def test_so3_grid_matches_oracle():
    from oracle import geometry as G

    for n in (72, 576):
        R = load_SO3_grid(n)
        assert R.shape == (n, 3, 3) and R.dtype == torch.float32
        np.testing.assert_allclose(R.numpy(), G.load_SO3_grid(n), atol=1e-6)


PLY_ASCII = """ply
format ascii 1.0
comment TextureFile tex.png
element vertex 4
property float x
property float y
property float z
property float nx
property float ny
property float nz
property float texture_u
property float texture_v
element face 2
property list uchar int vertex_indices
end_header
0 0 0 0 0 1 0 0
1 0 0 0 0 1 1 0
1 1 0 0 0 1 1 1
0 1 0 0 0 1 0 1
3 0 1 2
4 0 1 2 3
"""


def test_ply_and_obj_readers(tmp_path):
    (tmp_path / "m.ply").write_text(PLY_ASCII)
    m = mesh_io.load_mesh(tmp_path / "m.ply")
    assert m.vertices.shape == (4, 3) and m.faces.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3]]
    assert m.uvs.shape == (4, 2) and m.normals.shape == (4, 3) and m.texture is None
    # binary little-endian with vertex colours
    import struct

    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\n"
           "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
           "element face 1\nproperty list uchar int vertex_indices\nend_header\n").encode()
    body = b"".join(struct.pack("<fffBBB", *v) for v in [(0, 0, 0, 255, 0, 0), (1, 0, 0, 0, 255, 0), (0, 1, 0, 0, 0, 255)])
    body += struct.pack("<Biii", 3, 0, 1, 2)
    (tmp_path / "b.ply").write_bytes(hdr + body)
    b = mesh_io.load_mesh(tmp_path / "b.ply")
    assert b.colors.tolist() == [[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255]]
    np.testing.assert_allclose(b.normals, [[0, 0, 1]] * 3)  # computed from the face
    (tmp_path / "o.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nvn 0 0 1\nf 1/1/1 2/2/1 3/3/1\n")
    o = mesh_io.load_mesh(tmp_path / "o.obj")
    assert o.vertices.shape == (3, 3) and o.uvs.shape == (3, 2) and o.faces.tolist() == [[0, 1, 2]]
    with pytest.raises(ValueError):
        mesh_io.load_mesh(tmp_path / "x.stl")


def test_reference_test_asset_and_mesh_database(golden_dir):
    obj = mesh_store.RigidObject("can", golden_dir / "obj_000001.npz", mesh_units="mm")
    small = mesh_store.RigidObject("tri", mesh_io.MeshData(vertices=np.random.RandomState(0).rand(50, 3),
                                                           faces=np.array([[0, 1, 2]], np.int32),
                                                           normals=np.zeros((50, 3), np.float32)), mesh_units="m",
                                   scaling_factor=0.1)
    ds = mesh_store.RigidObjectDataset([obj, small])
    assert obj.scale == 0.001 and abs(small.scale - 0.1) < 1e-12 and len(ds) == 2
    assert ds.get_object_by_label("can") is obj
    with pytest.raises(RuntimeError):
        mesh_store.RigidObjectDataset([obj, obj])
    db = mesh_store.MeshDataBase.from_object_ds(ds)
    assert 0.1 < obj.diameter_meters < 0.25  # YCB-V master chef can, metres
    bm = db.batched()
    assert bm.points.shape == (2, 9951, 3) and bm.points.dtype == np.float32
    # the padded tail of the small object re-samples its own vertices
    own = {tuple(np.round(p, 6)) for p in bm.points[1, :50]}
    assert all(tuple(np.round(p, 6)) in own for p in bm.points[1, 50:200])
    sel = bm.select(["tri", "can"])
    assert sel.points.shape == (2, 9951, 3)
    s1 = sel.sample_points(2000, deterministic=True)
    s2 = sel.sample_points(2000, deterministic=True)
    assert s1.shape == (2, 2000, 3) and np.array_equal(s1, s2)
    pk = mesh_store.PackedMeshes(ds)
    assert pk.obj[0].tolist()[:4] == [0, 9951, 0, 15728] and pk.obj[1, 0] == 9951
    assert pk.faces.max() < 9951 and pk.verts.shape == (9951 + 50, 3)
    assert abs(pk.radius[0] - np.linalg.norm(pk.verts[:9951], axis=1).max()) < 1e-7


def test_model_config_defaults_and_key_renames():
    from happypose_amd import models

    cfg = models.check_update_config(dict(backbone_str="vanilla_resnet34", multiview_type="front_3views", n_views=4,
                                          render_normals=True))
    assert cfg.multiview_type == "TCO+front_3views" and cfg.n_rendered_views == 4
    assert cfg.predict_pose_update and not cfg.predict_rendered_views_logits and not cfg.render_depth
    assert cfg.depth_normalization_type == "tCR_scale"  # configs older than depth_augmentation
    assert models.n_input_channels(cfg) == 27
    cfg2 = models.check_update_config(dict(backbone_str="vanilla_resnet34", n_rendered_views=4, render_normals=True,
                                           render_depth=True, input_depth=True, depth_augmentation=False,
                                           depth_normalization_type="tCR_scale_clamp_center", multiview_type="TCO+front_3views"))
    assert models.n_input_channels(cfg2) == 32 and cfg2.depth_normalization_type == "tCR_scale_clamp_center"
    old = models.check_update_config(dict(input_strategy="input=obs+one_render", render_normals=True))
    assert old.is_coarse_compat and old.predict_rendered_views_logits and not old.predict_pose_update
    assert models.n_input_channels(old) == 9
    sd = models.change_keys_of_older_models({"backbone.backbone.conv1.weight": 1, "backbone.head.0.weight": 2, "pose_fc.bias": 3})
    assert sd == {"backbone.conv1.weight": 1, "views_logits_head.weight": 2, "pose_fc.bias": 3}
    assert models._arch("efficientnet-b3") == "efficientnet-b3"
    with pytest.raises(ValueError):
        models._arch("efficientnet-b7")
    assert len(models.efficientnet_b3_blocks()) == 26 and len(models.pose_model_param_shapes("efficientnet-b3", 6)) == 574


def test_lights_and_render_argument_checks():
    from happypose_amd.renderer import LightNodeProxy, Panda3dLightData, SceneRootProxy, make_scene_lights

    lights = make_scene_lights()
    assert len(lights) == 7 and lights[0].light_type == "ambient" and lights[0].color[:3] == (0.1, 0.1, 0.1)
    assert Panda3dLightData("ambient").color == (1.0, 1.0, 1.0, 1.0)
    # every point light carries a positioning_function(root_node, light_node) like the reference's
    # (TB/renderer/panda3d_scene_renderer.py:121-141); called on the NodePath stand-ins it lands on +/- axis x radius x 10
    got = []
    for l in lights[1:]:
        assert l.light_type == "point" and l.color[:3] == (0.4, 0.4, 0.4) and callable(l.positioning_function)
        node = LightNodeProxy()
        l.positioning_function(SceneRootProxy((0.0, 0.0, 0.0), 0.2), node)
        got.append(tuple(round(v, 6) for v in node.pos))
    assert sorted(got) == sorted([(2.0, 0, 0), (-2.0, 0, 0), (0, 2.0, 0), (0, -2.0, 0), (0, 0, 2.0), (0, 0, -2.0)])
    # the stand-ins accept the spellings Panda3D offers, and refuse what needs a scene graph
    node = LightNodeProxy()
    node.set_pos(1, 2, 3)
    assert node.getPos() == (1.0, 2.0, 3.0)
    node.setPos((4.0, 5.0, 6.0))
    assert node.get_pos() == (4.0, 5.0, 6.0)
    root = SceneRootProxy((0.1, 0.0, 0.0), 0.5)
    assert root.get_bounds().get_radius() == 0.5 and root.getBounds().getCenter() == (0.1, 0.0, 0.0)
    with pytest.raises(NotImplementedError):
        node.lookAt(0, 0, 0)


def test_ypr_offset_rotates_the_render_mesh_only():
    """``RigidObject.ypr_offset_deg`` (TB/datasets/object_dataset.py:42, applied by get_object_node's setHpr,
    TB/renderer/panda3d_scene_renderer.py:210-217): the RENDER mesh is rotated (heading about Z, pitch about X, roll about
    Y), the MeshDataBase point table is not (TB/lib3d/rigid_mesh_database.py:109-111).  Checked against scipy's intrinsic
    Z-X-Y Euler composition, an independent statement of the same convention."""
    from scipy.spatial.transform import Rotation

    from happypose_amd.mesh_store import MeshDataBase, PackedMeshes, RigidObject, RigidObjectDataset, hpr_to_matrix
    from happypose_amd.synthetic import make_mesh

    m = make_mesh(2, n_lat=12, n_lon=16, tex_size=16)
    for ypr in ((0.0, -90.0, 0.0), (30.0, 20.0, -10.0)):
        plain = PackedMeshes(RigidObjectDataset([RigidObject("a", m)]))
        ds = RigidObjectDataset([RigidObject("a", m, ypr_offset_deg=ypr)])
        rot = PackedMeshes(ds)
        R = Rotation.from_euler("ZXY", ypr, degrees=True).as_matrix()
        np.testing.assert_allclose(hpr_to_matrix(ypr), R, atol=1e-12)
        np.testing.assert_allclose(rot.verts, plain.verts @ R.T.astype(np.float32), atol=2e-6)
        np.testing.assert_allclose(rot.normals, plain.normals @ R.T.astype(np.float32), atol=2e-6)
        assert np.array_equal(rot.faces, plain.faces) and np.array_equal(rot.uvs, plain.uvs)
        np.testing.assert_allclose(rot.bounds_radius, plain.bounds_radius, rtol=0.2)  # a rotated box: the same order
        pts = MeshDataBase.from_object_ds(ds).batched().points
        np.testing.assert_array_equal(pts, MeshDataBase.from_object_ds(RigidObjectDataset([RigidObject("a", m)])).batched().points)
    # axis checks of the convention: pitch turns +Y towards +Z, heading turns +X towards +Y (ShapeNet's (0, -90, 0) maps +Z to +Y)
    np.testing.assert_allclose(hpr_to_matrix((0, -90, 0)) @ np.array([0, 0, 1.0]), [0, 1, 0], atol=1e-12)
    np.testing.assert_allclose(hpr_to_matrix((0, 90, 0)) @ np.array([0, 1.0, 0]), [0, 0, 1], atol=1e-12)
    np.testing.assert_allclose(hpr_to_matrix((90, 0, 0)) @ np.array([1.0, 0, 0]), [0, 1, 0], atol=1e-12)


def test_synthetic_scene_is_seeded_and_in_view():
    from happypose_amd.synthetic import make_mesh, make_scene, named_weights

    a, b = make_scene(seed=2), make_scene(seed=2)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert a["TCO_hyp"].shape == (128, 4, 4) and a["images"].shape == (1, 3, 480, 640)
    R = a["TCO_hyp"][:, :3, :3]
    np.testing.assert_allclose(R @ np.swapaxes(R, 1, 2), np.tile(np.eye(3), (128, 1, 1)), atol=1e-5)
    m = make_mesh(1)
    assert m.vertices.shape == (8249, 3) and m.faces.shape == (16128, 3) and m.texture.shape == (1024, 1024, 4)
    w1 = named_weights({"a.weight": (4, 3, 3, 3), "bn.running_var": (4,)}, seed=0)
    w2 = named_weights({"bn.running_var": (4,), "a.weight": (4, 3, 3, 3)}, seed=0)
    assert np.array_equal(w1["a.weight"], w2["a.weight"]) and (w1["bn.running_var"] > 0).all()


def test_load_cfg_restricted_yaml_and_named_models(tmp_path):
    """config.yaml files of the reference are dumps of argparse.Namespace objects (read there with
    yaml.UnsafeLoader): the restricted loader maps those tags to attribute bags and refuses to
    construct anything else."""
    import yaml

    from happypose_amd import load_model as LM
    from happypose_amd.models import check_update_config, n_input_channels

    f = tmp_path / "config.yaml"
    f.write_text("!!python/object:argparse.Namespace\nbackbone_str: vanilla_resnet34\nn_views: 4\n"
                 "multiview_type: front_3views\nrender_normals: true\ninput_resize: !!python/tuple [540, 720]\n"
                 "renderer: panda3d\n")
    cfg = LM.load_cfg(f)
    assert cfg.backbone_str == "vanilla_resnet34" and cfg.input_resize == (540, 720)
    upd = check_update_config(cfg)
    assert upd.multiview_type == "TCO+front_3views" and n_input_channels(upd) == 27
    f.write_text("a: 1\nb: [2, 3]\n")  # plain mapping (OmegaConf-style configs)
    assert LM.load_cfg(f).b == [2, 3]
    f.write_text("x: !!python/object/apply:os.system ['echo pwned']\n")
    with pytest.raises(yaml.YAMLError):
        LM.load_cfg(f)
    m = LM.NAMED_MODELS
    assert set(m) == {"megapose-1.0-RGB", "megapose-1.0-RGBD", "megapose-1.0-RGB-multi-hypothesis",
                      "megapose-1.0-RGB-multi-hypothesis-icp"}
    assert m["megapose-1.0-RGBD"]["requires_depth"] and m["megapose-1.0-RGBD"]["refiner_run_id"] == "refiner-rgbd-288182519"
    assert m["megapose-1.0-RGB-multi-hypothesis-icp"]["inference_parameters"] == {
        "n_refiner_iterations": 5, "n_pose_hypotheses": 5, "run_depth_refiner": True}
    assert m["megapose-1.0-RGB"]["inference_parameters"] == {"n_refiner_iterations": 5, "n_pose_hypotheses": 1}
    # the coarse / scoring network's default plan: fp16 where the five best of 576 scored views go on (BASELINE config 5)
    assert {k: LM.default_coarse_precision(k) for k in m} == {
        "megapose-1.0-RGB": "f32", "megapose-1.0-RGBD": "f32", "megapose-1.0-RGB-multi-hypothesis": "f16",
        "megapose-1.0-RGB-multi-hypothesis-icp": "f16"}


def test_legacy_keys_and_config_defaults_golden(golden_dir):
    """``change_keys_of_older_models`` (TB/utils/models_compat.py:17-27) and ``check_update_config``
    (MP/training/pose_models_cfg.py:36-86) against what the reference's own functions returned
    (tools/gen_golden_loop.py, G10): SURVEY.md 8f-2."""
    import json

    from happypose_amd.models import change_keys_of_older_models, check_update_config

    g = np.load(golden_dir / "g10_loop.npz")
    keys = [str(k) for k in g["compat/keys_in"]]
    new = change_keys_of_older_models({k: i for i, k in enumerate(keys)})
    assert list(new.keys()) == [str(k) for k in g["compat/keys_out"]]
    assert list(new.values()) == g["compat/vals_out"].tolist()
    cfgs, outs = json.loads(str(g["cfg/in"])), json.loads(str(g["cfg/out"]))
    assert len(cfgs) == len(outs) == 5
    for c, want in zip(cfgs, outs):
        got = vars(check_update_config(dict(c)))
        for k, v in want.items():  # every field the reference sets / keeps has the reference's value
            assert k in got and got[k] == v, (c, k, got.get(k), v)
        # fields only this implementation adds are defaults the reference reads from TrainingConfig
        assert set(got) - set(want) <= {"views_inplane_rotations", "depth_normalization_type", "backbone_str", "renderer",
                                        "render_normals", "render_depth", "input_depth"}


def test_detector_oracle_shapes():
    """oracle/detector.py (torchvision ResNet-50 + FPN + RPN head restated): key list / parameter count of the reference's
    DetectorMaskRCNN backbone and the pyramid geometry on a small image."""
    from happypose_amd.synthetic import named_weights
    from oracle import detector as od

    s = od.param_shapes()
    assert len(s) == 340 and s["backbone.body.layer4.2.conv3.weight"] == (2048, 512, 1, 1)
    assert s["backbone.fpn.inner_blocks.3.0.weight"] == (256, 2048, 1, 1) and s["rpn.head.bbox_pred.bias"] == (12,)
    n_par = sum(int(np.prod(v)) for k, v in s.items() if not k.endswith("num_batches_tracked"))
    assert abs(n_par / 1e6 - 27.5) < 0.1  # 23.5 M (ResNet-50 without fc) + 3.3 M (FPN) + 0.6 M (RPN head)
    with torch.no_grad():
        out = od.backbone_fpn_rpn(torch.rand(1, 3, 64, 96), named_weights(s, seed=1))
    assert [tuple(f.shape[-2:]) for f in out["features"]] == [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]
    assert all(o.shape[1] == 3 for o in out["objectness"]) and all(d.shape[1] == 12 for d in out["deltas"])
    assert all(torch.isfinite(f).all() for f in out["features"])


def test_torch_ops_registered_with_shape_functions():
    """``torch.ops.happypose_amd.*`` come from the compiled operator library (``csrc/torch_library.cpp``), their Meta kernels
    give the output shapes, and there is no CPU kernel."""
    from happypose_amd import torch_ops

    o = torch.ops.happypose_amd
    assert torch_ops.LIBRARY.name == "libhappypose_amd_torch.so" and str(torch_ops.LIBRARY) in torch.ops.loaded_libraries
    for name in torch_ops.OPS:
        assert hasattr(o, name), name
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)
    i32 = dict(dtype=torch.int32)
    assert o.crop_roi_align(m(2, 3, 48, 64), m(5, 4), m(5, **i32), 24, 32).shape == (5, 3, 24, 32)
    assert o.pose_update(m(5, 4, 4), m(5, 3, 3), m(5, 9)).shape == (5, 4, 4)
    assert [t.shape[1] for t in o.rasterize(0, m(5, **i32), m(5, 4, 4), m(5, 3, 3), 24, 32, True, True)] == [3, 3, 1]
    prep = o.pose_prep(0, m(5, 4, 4), m(2, 3, 3), m(5, **i32), m(5, **i32), m(2000, **i32), m(200, **i32), 48, 64, 24, 32, "TCO+front_3views")
    assert prep[2].shape == (5, 4, 4, 4) and prep[5].shape == (5, 4, 3, 3)
    assert o.conv2d_nhwc(m(2, 8, 8, 16), m(32, 3, 3, 16), 2, 1).shape == (2, 4, 4, 32)
    with pytest.raises(ValueError):
        o.net_forward(12345, m(1, 240, 320, 8))  # an integer nobody announced is not dereferenced
    with pytest.raises(NotImplementedError):
        o.pose_update(torch.eye(4)[None], torch.eye(3)[None], torch.zeros(1, 9))


def test_mip_chain_matches_box_filter():
    """``mesh_store.mip_chain``: 2 x 2 box filter, rounded to nearest, halving down to 1 x 1; the packed texture pool holds
    level 0 followed by the chain and the object row records the number of levels."""
    from happypose_amd.mesh_store import PackedMeshes, mip_chain
    from happypose_amd.synthetic import make_object_dataset

    t = np.random.RandomState(0).randint(0, 256, size=(8, 4, 4)).astype(np.uint8)
    ch = mip_chain(t)
    assert [c.shape for c in ch] == [(4, 2, 4), (2, 1, 4), (1, 1, 4)]
    ref = (t.astype(np.int32).reshape(4, 2, 2, 2, 4).sum((1, 3)) + 2) // 4
    assert np.array_equal(ch[0], ref.astype(np.uint8))
    assert np.array_equal(ch[1][:, 0], ((ch[0].astype(np.int32)[0::2].sum(1) + ch[0].astype(np.int32)[1::2].sum(1) + 2) // 4).astype(np.uint8))
    pm = PackedMeshes(make_object_dataset(2, seed=1, tex_size=64))
    assert pm.obj[0, 7] == 7 and pm.obj[1, 4] == sum(4 * (64 >> k) ** 2 for k in range(7))
    assert pm.tex.size == 2 * pm.obj[1, 4]


def test_graph_cache_structure_helpers():
    """``graphs.flatten`` / ``unflatten`` round-trip the nested per-lane / per-iteration records (tensors, None, scalars)."""
    from happypose_amd.graphs import GraphCache, flatten, unflatten

    rec = [[dict(TCO=torch.ones(2, 4, 4), pose=None, render_time=0.5, parts=(torch.zeros(3), torch.arange(2)))], [dict(TCO=torch.eye(4))]]
    flat = []
    spec = flatten(rec, flat)
    assert len(flat) == 4 and all(isinstance(t, torch.Tensor) for t in flat)
    back = unflatten(spec, [t + 1 for t in flat])
    assert back[0][0]["pose"] is None and back[0][0]["render_time"] == 0.5
    assert torch.equal(back[0][0]["TCO"], torch.full((2, 4, 4), 2.0)) and torch.equal(back[0][0]["parts"][1], torch.arange(2) + 1)
    assert torch.equal(back[1][0]["TCO"], torch.eye(4) + 1)
    assert GraphCache.MAX_ENTRIES >= 2


def test_estimator_hands_small_chunks_to_the_lanes():
    """``_run_model_chunks_once``: a stage whose ``bsz_objects`` chunks are below the model's ``MIN_BATCH`` (and more than one)
    goes to ``forward_chunks`` in ONE call -- chunk order, slices and keyword arguments as the sequential loop would pass them;
    a model without lanes, a single chunk, or chunks at / above ``MIN_BATCH`` take the loop.  Same table either way."""
    from types import SimpleNamespace

    import pandas as pd

    from happypose_amd.pose_estimator import CosyPoseEstimator, ObservationTensor
    from happypose_amd.tensor_collection import PandasTensorCollection

    class Model:
        device = torch.device("cpu")
        mesh_db = None
        log: list = []

        def __call__(self, images, K, TCO, n_iterations, labels, im_ids):
            self.log.append(("call", len(labels)))
            out, T = {}, TCO.clone().float()
            for n in range(1, n_iterations + 1):
                Tn = T * 0.5 + images[im_ids.long()].mean(dim=(1, 2, 3))[:, None, None] + torch.as_tensor([float(l[3:]) for l in labels])[:, None, None]
                out[f"iteration={n}"] = SimpleNamespace(TCO_output=Tn, TCO_input=T, K_crop=K[im_ids.long()] * n, boxes_rend=Tn[:, 0, :4], boxes_crop=Tn[:, 1, :4])
                T = Tn
            return out

        def numerics_status(self):
            return 0

    class LaneModel(Model):
        MIN_BATCH = 32

        def forward_chunks(self, images, K, chunks, n_iterations=1, **kw):
            self.log.append(("chunks", [len(c[0]) for c in chunks]))
            return [Model.__call__(self, images, K, T, n_iterations, lab, ids) for lab, T, ids in chunks]

    rs = np.random.RandomState(0)
    B = 21
    infos = pd.DataFrame({"label": [f"obj{i % 4}" for i in range(B)], "batch_im_id": np.arange(B) % 2, "instance_id": np.arange(B)})
    obs = ObservationTensor(torch.as_tensor(rs.rand(2, 3, 4, 5).astype(np.float32)), torch.eye(3)[None].repeat(2, 1, 1))
    T0 = torch.as_tensor(rs.rand(B, 4, 4).astype(np.float32))

    def run(model, bsz):
        Model.log = []
        est = CosyPoseEstimator(refiner_model=model, coarse_model=model, bsz_objects=bsz)
        preds, _ = est.forward_refiner(obs, PandasTensorCollection(infos=infos.copy(), poses=T0.clone()), n_iterations=2)
        return preds, [e for e in Model.log if e[0] in ("call", "chunks")]

    ref, log = run(Model(), 8)
    assert log == [("call", 8), ("call", 8), ("call", 5)]
    got, log = run(LaneModel(), 8)
    assert log[0] == ("chunks", [8, 8, 5]) and len([e for e in log if e[0] == "chunks"]) == 1
    for k in ref:
        assert torch.equal(ref[k].poses, got[k].poses) and torch.equal(ref[k].K_crop, got[k].K_crop) and ref[k].infos.equals(got[k].infos)
    _, log = run(LaneModel(), 32)   # one chunk of 21: forward() decides by itself
    assert log == [("call", 21)]
    _, log = run(LaneModel(), 21)
    assert log == [("call", 21)]
    LaneModel.MIN_BATCH = 8          # chunks AT the threshold are forward()'s to split over the lanes
    _, log = run(LaneModel(), 8)
    assert log == [("call", 8), ("call", 8), ("call", 5)]


def test_bench_e2e_parity_is_relative_to_the_oracle_spread():
    """``bench.e2e_parity``: coarse logits are judged in units of the ORACLE's standard deviation over a detection's grid poses (an
    absolute tolerance was blind on the synthetic world), per detection; the top-5 sets and the final poses as before."""
    import importlib
    import sys

    root = str(Path(__file__).resolve().parent.parent)
    if root not in sys.path:
        sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    rs = np.random.RandomState(0)
    n_det, n_grid = 3, 48
    inst = np.repeat(np.arange(n_det), n_grid)
    cl = (5.6 + 0.05 * rs.normal(size=n_det * n_grid)) * np.repeat([1.0, 1.0, 1.0], n_grid)
    T = np.tile(np.eye(4, dtype=np.float32), (n_det, 1, 1))
    ref = {"coarse_df": pd.DataFrame({"coarse_logit": cl, "instance_id": inst}),
           "filtered_df": pd.DataFrame({"hypothesis_id": list(range(5)) * n_det}),
           "final_df": pd.DataFrame({"label": [f"obj{i}" for i in range(n_det)], "hypothesis_id": [1, 2, 3]}), "final_TCO": T}
    good = dict(coarse_logit=cl + 0.0003 * rs.normal(size=cl.shape), filtered_hyp=list(range(5)) * n_det, final_labels=[f"obj{i}" for i in range(n_det)],
                final_hyp=[1, 2, 3], final_poses=T.copy())
    p = bench.e2e_parity(good, ref, "f32")
    assert p["ok"] and p["final_hypothesis_agrees"] == n_det and p["coarse_logit_max_diff_over_spread"] < bench.COARSE_LOGIT_REL["f32"]
    assert len(p["coarse_logit_spread_per_detection"]) == n_det and all(0.03 < x < 0.07 for x in p["coarse_logit_spread_per_detection"])
    # a constant offset of a fifth of the spread on ONE detection: far inside the old absolute 5e-3 ... 5e-2, outside the relative bound
    bad = dict(good, coarse_logit=cl + np.where(inst == 1, 0.2 * cl[inst == 1].std(), 0.0))
    q = bench.e2e_parity(bad, ref, "f16")
    assert not q["ok"] and q["coarse_logit_max_diff_over_spread"] > bench.COARSE_LOGIT_REL["f16"] and q["coarse_logit_max_abs_diff"] < 2e-2


def test_bench_dump_outputs_writes_what_a_caller_receives(tmp_path, monkeypatch):
    """``bench.py --dump-outputs``: the tensors and numeric ``infos`` columns of the estimator's per-iteration tables and every
    tensor field of a predictor's result, one ``<name>.npy`` each -- float64 where the source is float64 or integer, float32
    otherwise -- and nothing beyond the 64 MB budget."""
    import importlib
    import sys

    from happypose_amd.pose_predictor import PosePredictorOutput
    from happypose_amd.tensor_collection import PandasTensorCollection

    root = str(Path(__file__).resolve().parent.parent)
    if root not in sys.path:
        sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    poses = torch.arange(32, dtype=torch.float32).reshape(2, 4, 4)
    infos = pd.DataFrame({"label": ["a", "b"], "instance_id": [0, 7], "coarse_logit": np.array([0.5, 0.25])})
    preds = {f"iteration={k}": PandasTensorCollection(infos, poses=poses + k) for k in (1, 2)}
    z = torch.zeros
    out = PosePredictorOutput(TCO_output=poses, TCO_input=poses - 1, renders=None, images_crop=None, TCV_O_input=poses, KV_crop=z(2, 1, 3, 3),
                              tCR=z(2, 3), labels=["a", "b"], K=z(2, 3, 3), K_crop=z(2, 3, 3), network_outputs={"pose": z(2, 9, dtype=torch.float16)},
                              boxes_rend=z(2, 4), boxes_crop=z(2, 4))
    arrays = dict(bench.collection_arrays("refiner", preds), **bench.predictor_arrays("forward", {"iteration=1": out}))
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    got = {p.stem: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert {"refiner_iteration1_poses", "refiner_iteration2_poses", "refiner_iteration2_instance_id", "refiner_iteration2_coarse_logit",
            "forward_iteration1_TCO_output", "forward_iteration1_TCO_input", "forward_iteration1_network_outputs_pose"} <= set(got)
    assert len(got) == 6 + 10 and not any("label" in k or "renders" in k for k in got)
    assert got["refiner_iteration2_poses"].dtype == np.float32 and np.array_equal(got["refiner_iteration2_poses"], (poses + 2).numpy())
    assert got["refiner_iteration1_instance_id"].dtype == np.float64 and got["refiner_iteration1_instance_id"].tolist() == [0.0, 7.0]
    assert got["refiner_iteration1_coarse_logit"].dtype == np.float64
    assert got["forward_iteration1_network_outputs_pose"].dtype == np.float32
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1024)
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "too_big"), arrays)
    assert not (tmp_path / "too_big").exists()
