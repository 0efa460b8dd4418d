"""Numerical guard of the fp16 plan: every fp16 launch that writes activations reports a value that was inf / NaN before
the activation or that overflowed the half it was rounded to (``HP_STATUS_NONFINITE``), and the Python layer repeats the
stage on an fp32 sibling network.

Bounds.  The mutations of (b) are chosen on the CPU from the fp64 restatement (``resnet_layers_ref``): the mutated layer's
``max|y|`` after the activation is at least ``2 x 65504`` (it must overflow a half whatever the fp16 plan's rounding of
weights and activations does to it: those errors are 1e-3 relative), every map of the unmutated control stays below
``0.5 x 65504``.  The band between the two is avoided on purpose: a value within half an ulp of 65504 is not the guard's
business.  (d) compares logits with ``torch.equal``: the repeat must BE the fp32 plan on its exact kernels."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from resnet_layers_ref import make_input, make_weights, module_layers, reference_network  # noqa: E402

F16_MAX = 65504.0
ARCHS = (("resnet18", 6), ("vanilla_resnet34", 9))
HW = (240, 320)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ a: input out of range
def _fill(xin, x, cin):
    xin.zero_()
    xin[..., :cin] = torch.as_tensor(x, device=xin.device).to(xin.dtype)


@pytest.mark.parametrize("route", ["f16in", "f32in"])
@pytest.mark.parametrize("arch,cin", ARCHS)
def test_input_out_of_range_sets_the_flag(dev, arch, cin, route):
    """A 7e4 patch in one sample (a depth plane in the wrong unit) is inf as a half: the stem that reads it -- the unfused
    5 x 5 stem + ``maxpool_f16`` of the WideResNet, the fused 7 x 7 stem of the ResNet-34 -- must report it, through
    ``hp_net_forward_f16in`` (fp16 records) and through ``hp_net_forward`` (fp32 records, ``cast_pad_f32_f16`` in front)."""
    from happypose_amd import ops

    net = ops.Net(arch, cin, make_weights(arch, cin), max_batch=2, device=dev, precision="f16")
    x = np.random.RandomState(1).uniform(0, 1, size=(2, HW[0], HW[1], cin)).astype(np.float32)
    if route == "f16in":
        xin = net.new_input(2)
        assert xin.dtype == torch.float16
    else:
        xin = torch.zeros((2, HW[0], HW[1], net.c_pad), dtype=torch.float32, device=dev)
    _fill(xin, x, cin)
    pose, logits, feats = net.forward(xin, want_pose=True, want_logits=True, want_features=True)
    assert net.status() == 0
    assert all(bool(torch.isfinite(t).all()) for t in (pose, logits, feats))
    assert net._sibling is None
    x[1, 100:140, 100:160, 2] = 7.0e4
    _fill(xin, x, cin)
    net.forward(xin, want_pose=True, want_logits=True)
    flags = net.status()
    print("flags", arch, route, flags)
    assert flags & ops.STATUS_NONFINITE, flags
    assert flags & ops.STATUS_EXACT_ONLY and net._sibling is not None  # the Python layer fell back
    assert net.status() == ops.STATUS_EXACT_ONLY


# ------------------------------------------------------------------------------------------------ b: overflow inside the network
# (layer-name suffix, what it covers); names resolved per arch below
CASES = ("conv1.weight",            # the stem: 5x5 + max-pool launch (WideResNet), fused 7x7 + pool (ResNet-34)
         "layer1.0.conv1.weight",   # 64-channel 3x3 (BN + ReLU prologue on the WideResNet)
         "layer1.0.conv2.weight",   # 64-channel 3x3 with a residual
         "layer2.0.conv1.weight",   # stride-2 3x3
         "layer2.0.downsample",     # 1x1 stride-2 shortcut
         "layer2.0.conv2.weight",   # 128-channel 3x3 with the shortcut as residual
         "layer3.1.conv1.weight",   # 256-channel 3x3 (prologue on the WideResNet)
         "layer4.1.conv2.weight")   # 512-channel 3x3, residual, the last map


def _layer_name(arch, case):
    if case == "layer2.0.downsample":
        return "backbone.layer2.0.downsample.0.weight" if arch == "vanilla_resnet34" else "backbone.layer2.0.downsample.weight"
    return "backbone." + case


_REF = {}


def _control(arch, cin):
    """weights, input and fp64 maps of the unmutated network (once per arch)"""
    if arch not in _REF:
        w = make_weights(arch, cin)
        x = make_input(1, HW, cin)
        maps = reference_network(arch, cin, w, x)
        _REF[arch] = (w, x, maps)
    return _REF[arch]


def _fold16(w, L):
    """the layer's weights as the fp16 plan rounds them (BN after the conv folded first): resnet_layers_ref.layer_ref"""
    wt = np.asarray(w[L["name"]], np.float64)
    if L["bn_after"]:
        g, v = (np.asarray(w[f"{L['bn_after']}.{k}"], np.float64) for k in ("weight", "running_var"))
        wt = wt * (g / np.sqrt(v + 1e-5)).reshape(-1, 1, 1, 1)
    return wt.astype(np.float16)


def _mutation(arch, cin, name):
    """Weights with layer ``name`` scaled so that its fp64 output reaches 2 x 65504 (chosen from the fp64 maps alone)."""
    w, x, maps = _control(arch, cin)
    layers, _, _ = module_layers(arch, cin, HW)
    L = next(l for l in layers if l["name"] == name)
    conv_maps = {k: v for k, v in maps.items() if k.endswith(".weight") or k == "pool"}
    worst = max(float(np.abs(v).max()) for v in conv_maps.values())
    assert worst <= 0.5 * F16_MAX, ("control out of range", worst)
    factor = 4.0 * F16_MAX / max(float(np.abs(maps[name]).max()), 1e-3)
    for _ in range(8):
        wm = dict(w)
        wm[name] = (np.asarray(w[name], np.float64) * factor).astype(np.float32)
        mm = reference_network(arch, cin, wm, x)
        if float(np.abs(mm[name]).max()) >= 2.0 * F16_MAX:
            break
        factor *= 2.0  # a residual / shift kept the map below the bound
    ymax = float(np.abs(mm[name]).max())
    print(f"MUTATION {arch} {name} factor {factor:.4g} max|y| {ymax:.4g} control worst {worst:.4g}")
    assert ymax >= 2.0 * F16_MAX, (name, ymax)
    assert all(np.isfinite(np.asarray(v, np.float64)).all() for v in mm.values()), "the fp64 restatement must stay finite"
    for l in layers:
        assert np.isfinite(_fold16(wm, l).astype(np.float64)).all(), ("fp16-rounded weights", l["name"])
    return wm, x


def _forward_status(dev, arch, cin, w, x):
    from happypose_amd import ops

    net = ops.Net(arch, cin, w, max_batch=2, device=dev, precision="f16")
    xin = net.new_input(1)
    _fill(xin, x, cin)
    net.forward(xin, want_pose=True, want_logits=True)
    torch.cuda.synchronize(dev)
    paths = {o["name"]: o["path"] for o in net.op_list() if o["kind"] == "conv"}
    return net.status(), paths


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("arch,cin", ARCHS)
def test_overflow_inside_the_network_sets_the_flag(dev, arch, cin, case):
    """One conv's weights scaled so that its stored output leaves the fp16 range (chosen from the fp64 maps, module docstring): the
    flag is set, and the unmutated control on the same input leaves it at 0.  (The network has ONE status word: where a layer
    follows the mutated one, the test cannot tell which of the two launches reported; ``layer4.1.conv2`` has no conv behind it.)"""
    from happypose_amd import ops

    name = _layer_name(arch, case)
    wm, x = _mutation(arch, cin, name)
    w, _, _ = _control(arch, cin)
    flags0, _ = _forward_status(dev, arch, cin, w, x)
    assert flags0 == 0, ("false alarm on the control", flags0)
    flags, paths = _forward_status(dev, arch, cin, wm, x)
    print("flags", arch, name, paths[name], flags)
    assert flags & ops.STATUS_NONFINITE, (name, paths[name], flags)


@pytest.mark.parametrize("arch,cin", ARCHS)
def test_mutated_layers_cover_every_f16_conv_path(dev, arch, cin):
    """The launch paths of the mutated layers are ALL the paths the plan's convs take: a kernel path added later without a
    case above fails here."""
    w, x, _ = _control(arch, cin)
    flags, paths = _forward_status(dev, arch, cin, w, x)
    assert flags == 0
    seen = {paths[_layer_name(arch, c)] for c in CASES}
    assert seen == set(paths.values()), (seen, set(paths.values()))
    assert all(p in ("conv_f16", "stem7_pool_f16") for p in seen), seen


# ------------------------------------------------------------------------------------------------ c: no false alarm at C5
def test_no_false_alarm_at_benchmark_batch(dev):
    """The fp16 plan on the C5 records (576 views; the construction of test_backbone_features_at_benchmark_batch_f16_plan):
    no flag, and no launch of a kernel with scratch (the guard must not have cost any instantiation its graph replay)."""
    from happypose_amd import ops
    import test_gpu_pipeline as tp

    bench = tp._bench()
    ds, renderer, scene, weights, model = bench.build_world(dev, "resnet34", seed=0, workload="C5", precision="f16", n_lanes=1)
    store = renderer.store
    images, K = torch.as_tensor(scene["images"], device=dev), torch.as_tensor(scene["K"], device=dev)
    labels = [store.labels[i] for i in scene["hyp_obj_ids"][:576]]
    T = torch.as_tensor(scene["TCO_hyp"][:576], device=dev)
    lane = model.lanes[0] if hasattr(model, "lanes") else model
    im_ids, obj_ids = lane._ids(images, K, labels, torch.zeros(576, dtype=torch.int32, device=dev))
    _, x, _, _, _ = lane._one_pass(images, K, im_ids, obj_ids, T, n_img_channels=lane._n_img, multiview_type="TCO", normalize=True,
                                   render_normals=lane.render_normals, render_depth=lane.render_depth, depth_mode=lane._depth_mode,
                                   want_pose=False, want_logits=True)
    assert x.dtype == torch.float16 and x.shape[0] == 576
    assert lane.backbone.status() == 0
    s0 = ops.scratch_launches()
    logits = lane.backbone.forward(x, want_pose=False, want_logits=True)[1]
    assert lane.backbone.status() == 0
    assert ops.scratch_launches() == s0
    assert bool(torch.isfinite(logits).all()) and lane.backbone._sibling is None


# ------------------------------------------------------------------------------------------------ d: the fallback
CCFG = dict(backbone_str="vanilla_resnet34", n_rendered_views=1, multiview_type="TCO", render_normals=True,
            predict_rendered_views_logits=True, predict_pose_update=False, depth_augmentation=False)
MID = "backbone.layer2.1.conv1.weight"
MID_FACTOR = 1.0e5  # He-scale weights (|w| < 1) stay finite as halves; an O(1) map x 1e5 leaves the fp16 range, not the fp32 one


@pytest.fixture(scope="module")
def world(dev):
    from happypose_amd.renderer import BatchRenderer
    from happypose_amd.synthetic import make_object_dataset, make_scene

    ds = make_object_dataset(3, seed=1, tex_size=256)
    renderer = BatchRenderer(ds, device=dev)
    return dict(renderer=renderer, store=renderer.store, scene=make_scene(n_detections=3, n_hypotheses=4, n_objects=3, seed=2))


def _nets(model):
    b = model.backbone
    return list(b.nets) if hasattr(b, "nets") else [b]


def _estimator(world, w, precision, **kw):
    from happypose_amd.models import create_model_pose
    from happypose_amd.pose_estimator import PoseEstimator

    coarse = create_model_pose(CCFG, world["renderer"], state_dict=w, max_batch=72, precision=precision, **kw)
    return PoseEstimator(refiner_model=None, coarse_model=coarse, bsz_objects=8, bsz_images=72, SO3_grid_size=72), coarse


def _stages(dev, world, est):
    """coarse logits of every detection x grid pose, then scoring logits of the first two hypotheses per detection"""
    import test_gpu_pipeline as tp
    from happypose_amd.pose_estimator import ObservationTensor, make_detections_from_object_data
    from oracle import geometry as G

    sc, store = world["scene"], world["store"]
    obs = ObservationTensor(torch.as_tensor(sc["images"][:, :3].copy(), device=dev), torch.as_tensor(sc["K"], device=dev))
    pts = store.mesh_db.points[sc["det_obj_ids"]]
    boxes = G.boxes_from_uv(G.project_points(pts, np.repeat(sc["K"], 3, 0), sc["TCO_det"]))
    det = make_detections_from_object_data(tp._labels(world, sc["det_obj_ids"]), boxes).to(dev)
    coarse, _ = est.forward_coarse_model(obs, det)
    cl = torch.as_tensor(coarse.infos.coarse_logit.values.copy())
    keep = np.flatnonzero(coarse.infos.hypothesis_id.values < 2)
    scored, _ = est.forward_scoring_model(obs, coarse[keep])
    return cl, torch.as_tensor(scored.infos.pose_logit.values.copy())


@pytest.mark.parametrize("variant", ["plain", "lanes2", "graphs"])
def test_estimator_repeats_an_overflowed_stage_on_the_fp32_plan(dev, world, variant):
    from happypose_amd import ops
    import test_gpu_pipeline as tp

    kw = dict(plain={}, lanes2=dict(n_lanes=2), graphs=dict(graphs=True))[variant]
    w = tp._weights("vanilla_resnet34", 9, pose=False, logits=1, seed=9, scale=1.0)
    wm = dict(w)
    wm[MID] = (np.asarray(w[MID], np.float64) * MID_FACTOR).astype(np.float32)
    assert np.isfinite(np.asarray(wm[MID]).astype(np.float16).astype(np.float64)).all()

    # unmutated: the sibling is never built, fp16 logits within the existing tolerance of the fp32 ones
    e16, m16 = _estimator(world, w, "f16", **kw)
    e32, m32 = _estimator(world, w, "f32", **kw)
    c16, s16 = _stages(dev, world, e16)
    c32, s32 = _stages(dev, world, e32)
    assert all(n._sibling is None for n in _nets(m16)) and m16.numerics_status() == 0
    tol = tp.C5_LOGIT_REL["f16"] * float(c32.reshape(3, 72).std(dim=1).min())  # per detection, against the spread of its 72 grid poses
    for a, b in ((c16, c32), (s16, s32)):  # (the scored rows are coarse hypotheses: the same scale)
        print("f16 vs f32 logits", float((a - b).abs().max()), "tol", tol)
        assert float((a - b).abs().max()) <= tol

    # one mid-network layer overflows the fp16 range: the stage is repeated on the sibling = the fp32 plan, forced exact
    b16, mb16 = _estimator(world, wm, "f16", **kw)
    b32, mb32 = _estimator(world, wm, "f32", **kw)
    mb32.backbone.force_exact(True)
    ref_c, ref_s = _stages(dev, world, b32)
    got_c, got_s = _stages(dev, world, b16)
    assert bool(torch.isfinite(got_c).all()) and bool(torch.isfinite(got_s).all())
    assert torch.equal(got_c, ref_c) and torch.equal(got_s, ref_s)
    assert mb16.numerics_status() == ops.STATUS_EXACT_ONLY
    assert all(n._on_sibling for n in _nets(mb16)), "every lane switches before the repeat"
    # a later call (graphs: replayed or re-captured on the fp32 plan) stays correct
    got_c2, got_s2 = _stages(dev, world, b16)
    assert torch.equal(got_c2, ref_c) and torch.equal(got_s2, ref_s)
    # back to the fp16 plan and to fp16 records
    mb16.backbone.force_exact(False)
    assert not any(n._on_sibling for n in _nets(mb16))
    lane = mb16.lanes[0] if hasattr(mb16, "lanes") else mb16
    assert lane._input_buffer(4).dtype == torch.float16
