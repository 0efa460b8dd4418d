"""The ResNet-34 / WideResNet-34 / -18 plans of csrc/net.cpp, layer by layer, against a plain fp64 restatement of the two
modules: every op's full NHWC map of every sample, not 512 pooled numbers.

The seam is ``hp_net_op_info`` / ``hp_net_set_taps`` (``ops.Net.op_list`` / ``set_taps``): a real plan runs through
``forward_chunk`` with its own launch choices -- fused stem + ReLU + max-pool, the 1x1 / stride-2 shortcut riding in the block's
3x3 / stride-2 launch, BN + ReLU prologues, the chained activation scale, tail split, chunks of ``max_batch`` -- and every op's
output is copied out right after the launch that wrote it.  The launch path of every op is read back and asserted, so a
silently un-fused stem or shortcut cannot pass as "tested".

Reference (tests/resnet_layers_ref.py: ``module_layers`` / ``layer_ref``): the module structure restated here (MP torchvision_resnet BasicBlock: conv -> BN
-> ReLU -> conv -> BN, + identity or conv1x1 -> BN, ReLU; wide_resnet BasicBlockV2: a = ReLU(BN(x)), shortcut conv1x1(a) or x,
conv(a) -> BN -> ReLU -> conv, + shortcut), un-folded BatchNorm with eps 1e-5, ``F.conv2d`` / ``F.max_pool2d`` in double.  It
walks ITS OWN structure and finds each GPU map by weight name; it never reads the plan's slot wiring, so a residual or a
shortcut wired to the wrong map fails here too.  Per-layer isolation: each layer's reference is computed from the maps the
kernels saw (the tapped input of that layer, the tapped residual), so nothing accumulates and the bound is that of one launch.

Bounds (``compare_network``; none tuned against the kernels):
  fp32 plan, conv (+ folded BN, prologue, residual, ReLU), fused stem -> pooled map, fused shortcut
        2e-5 x max|ref| of the map   (test_split_fp16_small_activations_keep_their_bits, _check_conv; also "direct", "igemm":
                                      test_conv3x3_kernel_families)
        4e-5 x max|ref| under ``set_conv_algo("winograd")`` / ``force_exact`` (test_conv3x3_kernel_families)
  fp16 plan: fp64 on the tapped fp16 input, BN folded in double and weights rounded to fp16 once, the prologue restated in
        fp16 (one rounding of x * s + b):  1.5e-3 x max(1, max|ref|)   (test_conv2d_f16_vs_fp64)
  un-fused max-pool (fp32 and fp16): bit-exact max of the tapped input
  head (mean, fc, pose, logits, features from the tapped last map): a-priori fp32 bound computed in double, u = 2^-24:
        a mean / dot product of n terms errs by at most (n + 2) u sum|a_i b_i| (+ |bias|), and an error e_c in its input
        adds sum_c |w_c| e_c: features = mean -> [fc] from the map; pose / logits from the features the kernels wrote
        (``head_check``).
Also printed per layer, NOT asserted: the worst per-output-channel ratio (the form of test_split_conv_dynamic_range).

Every comparison has teeth: tests/test_resnet_layers_reference.py (no GPU) feeds the same functions a mutated fp64 reference.

Measured on an MI355X: see CHANGELOG.md (worst ratio per group, which launches each group reached).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # also run as a script (the child interpreter of the shortcut-fusion A/B)
    sys.path.insert(0, ROOT)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from resnet_layers_ref import (FUSED_STEMS, TOL_EXACT, TOL_F16, TOL_SPLIT, compare_network, make_input, make_weights,  # noqa: E402
                               module_layers)


# ------------------------------------------------------------------------------------------------ the GPU side
def run_plan(dev, arch, cin, hw=(240, 320), n=3, max_batch=2, precision="f32", setup=None, w=None, x=None, seed=0, garbage=False):
    """One forward of a real plan with every conv / max-pool op tapped.  Also case g: pose / logits / features of the tapped
    forward are bit-identical to a forward of the same network without taps."""
    from happypose_amd import ops

    w = make_weights(arch, cin, seed) if w is None else w
    x = make_input(n, hw, cin, seed) if x is None else x
    net = ops.Net(arch, cin, w, max_batch=max_batch, device=dev, h=hw[0], w=hw[1], precision=precision)
    if setup:
        setup(net)
    xin = net.new_input(n)
    if garbage:  # the fused fp16 stem reads its real channels only
        xin[:] = torch.as_tensor(np.random.RandomState(9).uniform(-100, 100, size=tuple(xin.shape)), device=dev).to(xin.dtype)
    xin[..., :cin] = torch.as_tensor(x, device=dev).to(xin.dtype)
    plain = net.forward(xin, want_pose=True, want_logits=True, want_features=True)
    before = net.op_list()
    taps = net.set_taps([o["index"] for o in before if o["kind"] in ("conv", "maxpool")], n)
    out = net.forward(xin, want_pose=True, want_logits=True, want_features=True)
    torch.cuda.synchronize(dev)
    assert not (net.status() & ops.STATUS_NONFINITE)
    for a, b in zip(plain, out):
        assert torch.equal(a, b), "taps changed the outputs"
    ops_ = net.op_list()
    assert [(o["path"], o["materialised"]) for o in ops_] == [(o["path"], o["materialised"]) for o in before], "taps changed the launches"
    maps, paths = {}, {}
    for o in ops_:
        key = o["name"] if o["kind"] == "conv" else {"maxpool": "pool", "head": "head"}[o["kind"]]
        paths[key] = o["path"]
        if o["index"] in taps and o["materialised"]:
            maps[key] = taps[o["index"]].cpu().numpy()
    maps.update(pose=out[0].cpu().numpy(), logits=out[1].cpu().numpy(), features=out[2].cpu().numpy())
    net.set_taps([], 0)
    return dict(maps=maps, paths=paths, ops=ops_, x=xin.cpu().numpy(), w=w, elem=ops_[0]["elem_bytes"])


def check_op_list(arch, cin, hw, ops_):
    """The op list names every conv of the module with the module's geometry, one max-pool and one head."""
    layers, pool, _ = module_layers(arch, cin, hw)
    by = {o["name"]: o for o in ops_ if o["kind"] == "conv"}
    assert sorted(by) == sorted(L["name"] for L in layers) and len(by) == sum(o["kind"] == "conv" for o in ops_)
    for L in layers:
        o = by[L["name"]]
        got = tuple(o[k] for k in ("k", "stride", "pad", "act", "H", "W", "Cin", "Ho", "Wo", "Cout", "prologue"))
        assert got == (L["k"], L["stride"], L["pad"], int(L["relu"]), L["H"], L["W"], L["cin"], L["Ho"], L["Wo"], L["cout"], bool(L["bn_before"])), (L["name"], got)
    mp = [o for o in ops_ if o["kind"] == "maxpool"]
    assert len(mp) == 1 and (mp[0]["H"], mp[0]["W"], mp[0]["Ho"], mp[0]["Wo"], mp[0]["Cout"]) == (pool["H"], pool["W"], pool["Ho"], pool["Wo"], 64)
    assert [o["kind"] for o in ops_].count("head") == 1 and ops_[-1]["kind"] == "head"


def downs(paths):
    return {k: v for k, v in paths.items() if ".downsample." in k}


def assert_fused(paths, arch):
    """The stem ran fused with the pool and every stride-2 shortcut rode in its 3x3 launch (layer1 of a WideResNet has no
    stride: its 64 -> 64 blocks have no shortcut at all)."""
    assert paths["backbone.conv1.weight"] in FUSED_STEMS and paths["pool"] == "fused_away", paths["backbone.conv1.weight"]
    d = downs(paths)
    assert len(d) == 3 and all(v == "rode" for v in d.values()), d
    for k in d:
        assert paths[k.split(".downsample.")[0] + ".conv1.weight"] == "split3x3+shortcut"


def check_plan(label, arch, cin, got, tol, f16=False):
    check_op_list(arch, cin, got["x"].shape[1:3], got["ops"])
    assert got["elem"] == (2 if f16 else 4)
    print(f"PATHS {label} " + " ".join(f"{k.replace('backbone.', '').replace('.weight', '')}={v}" for k, v in got["paths"].items()))
    r = compare_network(arch, cin, got["w"], got["x"], got["maps"], tol, f16=f16, label=label)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    print(f"WORST {label} {max(r, key=r.get)} {max(r.values()):.4f}")
    assert not bad, bad
    return r


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the MI355X box"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ tests
PLANS_A = [("vanilla_resnet34", 9, "stem7_pool"), ("vanilla_resnet34", 27, "stem7_pool"), ("vanilla_resnet34", 32, "stem7_pool"),
           ("resnet34", 6, "stem_split_pool"), ("resnet18", 6, "stem_split_pool"), ("resnet18", 7, "igemm_split_pool")]


@pytest.mark.parametrize("arch,cin,stem", PLANS_A, ids=[f"{a}-{c}" for a, c, _ in PLANS_A])
def test_every_plan_240x320(dev, arch, cin, stem):
    """a. every plan at the product frame size, batch 3 in chunks 2 + 1: 7x7 stems with channel slabs of 8 (32), 4 (27 -> 28) and
    both (9 -> 12), the run-mode 5x5 stem, and a WideResNet whose 7 input channels take the generic fused stem."""
    got = run_plan(dev, arch, cin, seed=cin)
    assert got["paths"]["backbone.conv1.weight"] == stem
    assert_fused(got["paths"], arch)
    check_plan(f"a-{arch}-{cin}", arch, cin, got, TOL_SPLIT)


@pytest.mark.parametrize("hw", [(180, 250), (126, 202)], ids=["180x250", "126x202"])
@pytest.mark.parametrize("arch,cin", [("resnet34", 6), ("vanilla_resnet34", 27)])
def test_odd_frame_sizes(dev, arch, cin, hw):
    """b. 180 x 250 (maps 45x63, 23x32, 12x16, 6x8) and 126 x 202 (32x51, 16x26, 8x13, 4x7): odd maps, pooled maps that are no
    multiple of the stem tiles, stride-2 layers whose last row / column window hangs over the edge."""
    got = run_plan(dev, arch, cin, hw=hw, seed=hw[0])
    assert_fused(got["paths"], arch)
    check_plan(f"b-{arch}-{cin}-{hw[0]}x{hw[1]}", arch, cin, got, TOL_SPLIT)


SWITCHES = {
    "act_scale_off": (lambda net: net.set_act_scale(False), TOL_SPLIT, True),
    "tail_split_off": (lambda net: net.set_tail_split(False), TOL_SPLIT, True),
    "winograd": (lambda net: net.set_conv_algo("winograd"), TOL_EXACT, False),
    "direct": (lambda net: net.set_conv_algo("direct"), TOL_SPLIT, False),
    "igemm": (lambda net: net.set_conv_algo("igemm"), TOL_SPLIT, False),
    "force_exact": (lambda net: net.force_exact(True), TOL_EXACT, False),
}


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("arch,cin", [("resnet34", 6), ("vanilla_resnet34", 27)])
def test_switches(dev, arch, cin, switch):
    """c. one plan of each family under every per-network switch, at 180 x 250 (odd maps).  The exact-fp32 algorithms un-fuse the
    stem and the shortcuts: the max-pool row of the table applies, and no split-fp16 launch may be left."""
    setup, tol, fused = SWITCHES[switch]
    got = run_plan(dev, arch, cin, hw=(180, 250), setup=setup, seed=3)
    p = got["paths"]
    if fused:
        assert_fused(p, arch)
    else:
        assert p["backbone.conv1.weight"] not in FUSED_STEMS and p["pool"] == "maxpool" and "backbone.conv1.weight" in got["maps"]
        allowed = {"winograd": {"winograd", "patch", "generic"}, "force_exact": {"winograd", "patch", "generic"}, "direct": {"patch", "generic"},
                   "igemm": {"generic"}}[switch]
        convs = {k: v for k, v in p.items() if k not in ("pool", "head")}
        assert set(convs.values()) <= allowed, convs
        if switch in ("winograd", "force_exact"):
            assert "winograd" in convs.values()
    check_plan(f"c-{switch}-{arch}-{cin}", arch, cin, got, tol)


@pytest.mark.parametrize("arch,cin,n,hw", [("resnet34", 6, 1, (240, 320)), ("vanilla_resnet34", 27, 1, (240, 320)),
                                           ("resnet18", 6, 130, (48, 64)), ("vanilla_resnet34", 27, 130, (48, 64))])
def test_batch_1_and_130(dev, arch, cin, n, hw):
    """c. a batch of 1, and one of 130 at 48 x 64 (maps 12x16, 6x8, 3x4, 2x2): more than one item per block, tail tiles."""
    got = run_plan(dev, arch, cin, hw=hw, n=n, max_batch=n, seed=n)
    assert_fused(got["paths"], arch)
    check_plan(f"c-batch{n}-{arch}-{cin}", arch, cin, got, TOL_SPLIT)


AB_PLANS = [("resnet34", 6), ("vanilla_resnet34", 27)]


def _shortcut_maps(got, arch, cin):
    """name -> map of every down-sampling shortcut and of the block input it reads (what its reference needs)."""
    layers, _, _ = module_layers(arch, cin, got["x"].shape[1:3])
    out = {}
    for L in layers:
        if L["role"] == "down":
            out[L["name"]], out[L["src"]] = got["maps"][L["name"]], got["maps"][L["src"]]
    return out


@pytest.fixture(scope="module")
def unfused_shortcuts(tmp_path_factory):
    """The AB_PLANS with HP_NET_NO_SHORTCUT_FUSION=1.  Switches are read once per process: one child interpreter runs them and
    leaves the shortcut maps, their inputs and the launch paths in an .npz (the pattern of test_gpu_mbconv.unfused_maps)."""
    path = str(tmp_path_factory.mktemp("resnet_ab") / "unfused.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "dump-unfused", path], capture_output=True, text=True, timeout=900,
                       env={**os.environ, "HP_NET_NO_SHORTCUT_FUSION": "1"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(path)


@pytest.mark.parametrize("i", range(len(AB_PLANS)), ids=[f"{a}-{c}" for a, c in AB_PLANS])
def test_shortcut_fusion_ab(dev, unfused_shortcuts, i):
    """d. the shortcut maps with the shortcut riding in the 3x3 launch and as a launch of its own (HP_NET_NO_SHORTCUT_FUSION=1 in
    a child interpreter): both within the bound of their own inputs.  That the switch selected something is asserted from the
    launch-path record of both sides ("rode" here, "igemm_split" there).  Bit difference of the maps is printed, not asserted:
    measured on an MI355X, ALL three shortcut maps of BOTH plans (64, 128 and 256 input channels) are bit-identical on the two
    kernels -- the same fp16 half-products accumulated in the same order, the zero taps of the 3x3 twin adding exact zeros --
    so "not bit-identical" would reject two correct kernels, and "identical" would pin an accident of two schedules."""
    arch, cin = AB_PLANS[i]
    got = run_plan(dev, arch, cin, seed=40 + i)
    assert_fused(got["paths"], arch)
    new = _shortcut_maps(got, arch, cin)
    old = {k[len(f"{i}@map@"):]: unfused_shortcuts[k] for k in unfused_shortcuts.files if k.startswith(f"{i}@map@")}
    names = sorted(downs(got["paths"]))
    old_paths = [str(unfused_shortcuts[f"{i}@path@{k}"]) for k in names]
    assert old_paths == ["igemm_split"] * 3, old_paths
    for side, maps in (("fused", new), ("unfused", old)):
        r = compare_network(arch, cin, got["w"], got["x"], maps, TOL_SPLIT, only=names, label=f"d-{side}-{arch}-{cin}", head=False)
        assert sorted(r) == names and all(v <= 1.0 for v in r.values()), r
    same = [k for k in names if np.array_equal(new[k], old[k])]
    print(f"BITS d-{arch}-{cin} identical on both sides: {same}")


def small_activation_weights():
    """The network of test_split_fp16_small_activations_keep_their_bits: BN x 1e-4 in front of six convs, the conv x 1e4."""
    from happypose_amd.models import pose_model_param_shapes
    from happypose_amd.synthetic import predictor_weights

    w = predictor_weights(pose_model_param_shapes("resnet18", 6, pose_dim=9, n_views_logits=1), seed=4)
    blocks = ("layer1.1", "layer2.0", "layer2.1", "layer3.1", "layer4.0", "layer4.1")
    for blk in blocks:
        w[f"backbone.{blk}.bn2.weight"] = (w[f"backbone.{blk}.bn2.weight"] * 1e-4).astype(np.float32)
        w[f"backbone.{blk}.bn2.bias"] = (w[f"backbone.{blk}.bn2.bias"] * 1e-4).astype(np.float32)
        w[f"backbone.{blk}.conv2.weight"] = (w[f"backbone.{blk}.conv2.weight"] * 1e4).astype(np.float32)
    return w, [f"backbone.{b}.conv2.weight" for b in blocks]


def test_small_activations_every_layer(dev):
    """e. activations of ~1e-4 in front of six convs.  With the dynamic activation scale EVERY layer meets 2e-5 x max|ref| of its
    own map; without it exactly the six layers that read the small maps do not, each by at least the existing test's factor of
    10 (measured: 1.2 - 2.6 x the bound without, <= 0.04 with)."""
    w, small = small_activation_weights()
    x = np.random.RandomState(2).uniform(0, 1, size=(4, 240, 320, 6)).astype(np.float32)
    on = run_plan(dev, "resnet18", 6, n=4, max_batch=4, w=w, x=x)
    r_on = check_plan("e-scale-on", "resnet18", 6, on, TOL_SPLIT)
    off = run_plan(dev, "resnet18", 6, n=4, max_batch=4, w=w, x=x, setup=lambda net: net.set_act_scale(False))
    r_off = compare_network("resnet18", 6, w, off["x"], off["maps"], TOL_SPLIT, label="e-scale-off")
    failing = sorted(k for k, v in r_off.items() if v > 1.0)
    print("FAILING without the activation scale:", failing)
    assert failing, "the floor the scale removes is real"
    for k in failing:
        assert r_off[k] >= 10 * r_on[k], (k, r_off[k], r_on[k])
    assert failing == sorted(small), (failing, small)  # exactly the layers that read a ~1e-4 map


@pytest.mark.parametrize("arch,cin,stem,pool", [("vanilla_resnet34", 9, "stem7_pool_f16", "fused_away"), ("resnet34", 6, "conv_f16", "maxpool_f16")])
def test_fp16_plan(dev, arch, cin, stem, pool):
    """f. the whole fp16 plan, layer by layer: the fused fp16 7x7 stem (the C5 model) with garbage in the pad channels of its
    16-channel input record, and the 5x5 stem, which is not fused, so that launch_maxpool_f16 runs; the head on an fp16 map."""
    got = run_plan(dev, arch, cin, precision="f16", garbage=(arch == "vanilla_resnet34"), seed=16)
    p = got["paths"]
    assert (p["backbone.conv1.weight"], p["pool"]) == (stem, pool), (p["backbone.conv1.weight"], p["pool"])
    assert {v for k, v in p.items() if k not in ("backbone.conv1.weight", "pool", "head")} == {"conv_f16"}
    assert got["maps"]["pool"].dtype == np.float16 and got["x"].dtype == np.float16
    check_plan(f"f-{arch}-{cin}", arch, cin, got, TOL_F16, f16=True)


def test_tap_arguments(dev):
    """The seam's own contract: the head has no output map to tap, an unknown op is refused, and ``set_taps([], 0)`` clears."""
    from happypose_amd import ops

    net = ops.Net("resnet18", 6, make_weights("resnet18", 6), max_batch=2, device=dev, h=64, w=64)
    xin = net.new_input(2)
    ops_ = net.op_list()
    assert all(o["path"] == "none" for o in ops_) and ops_[-1]["kind"] == "head"
    with pytest.raises(AssertionError, match="no output map"):
        net.set_taps([len(ops_) - 1], 2)
    taps = net.set_taps([1], 2)
    net.forward(xin)
    net.set_taps([], 0)
    torch.cuda.synchronize(dev)
    kept = taps[1].clone()
    taps[1].zero_()
    net.forward(xin)
    torch.cuda.synchronize(dev)
    assert kept.abs().max() > 0 and taps[1].abs().max() == 0  # written while set, untouched once cleared


def test_taps_are_refused_while_the_stream_captures(dev):
    """A forward with taps set on a capturing stream is refused before its first launch (the header says so), the capture
    ends cleanly holding only what was recorded before, and with the taps cleared the network runs as before."""
    from happypose_amd import ops

    net = ops.Net("resnet18", 6, make_weights("resnet18", 6), max_batch=2, device=dev, h=64, w=64)
    xin = net.new_input(2)
    xin[..., :6] = torch.as_tensor(make_input(2, (64, 64), 6), device=dev)
    eager = net.forward(xin)[0].clone()  # first forward eager
    counter = torch.zeros(1, device=dev)
    net.set_taps([1], 2)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    refused = None
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            counter.add_(1)  # the graph is not empty
            try:
                net.forward(xin)
            except AssertionError as e:
                refused = str(e)
        finally:
            g.capture_end()
    assert refused is not None and "capturing" in refused, refused
    net.set_taps([], 0)
    g.replay()  # what was captured is the counter alone
    pose = net.forward(xin)[0]
    torch.cuda.synchronize(dev)
    assert float(counter) == 1.0
    assert torch.equal(pose, eager)


def _dump_unfused(path):
    dev = torch.device("cuda:0")
    out = {}
    for i, (arch, cin) in enumerate(AB_PLANS):
        got = run_plan(dev, arch, cin, seed=40 + i)
        for k, v in _shortcut_maps(got, arch, cin).items():
            out[f"{i}@map@{k}"] = v
        for k, v in downs(got["paths"]).items():
            out[f"{i}@path@{k}"] = np.array(v)
    np.savez(path, **out)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "dump-unfused", "usage: test_gpu_resnet_layers.py dump-unfused <out.npz>"
    _dump_unfused(sys.argv[2])
