"""The comparisons of tests/test_gpu_resnet_layers.py have teeth, and their bounds are attainable -- shown without a GPU: the
same comparison functions, parameters and frame sizes (case b: 126 x 202 and 180 x 250, batch 3), fed

* a MUTATED fp64 reference in the place of the kernels' maps (``layer_ref(mutate=...)``, each the way a kernel could be wrong):
  the mutated layer must miss its bound by at least 100x while every other layer -- whose reference is computed from the maps
  "the kernels saw", mutated ones included -- stays inside; and what the same mutation does to the pooled 512-vector relative
  to the whole-backbone check's 2e-4 x max|ref| (test_backbone_golden_g6) is printed: ``G6 <mutation> <layer> <x bound>``;
* PyTorch's own fp32 ``F.conv2d`` network: every fp32 bound of the table must hold for it, head included.

  prepad       prologue applied to the padding                  WideResNet conv1 (3x3 behind BN + ReLU)
  edge         last row / column of a stride-2 layer one off    layers whose input map is odd (45 x 63: both; 32 x 51: columns)
  rawshortcut  shortcut fed the un-activated block input        WideResNet shortcut
  resafter     residual added after the ReLU                    ResNet-34 conv2
  pool2        pooled-map window 2x2                            both
  eps          BatchNorm folded with eps 1e-3                   both (make_weights: running variances 0.01 .. 0.1)
  meanrow      head mean over one row too few                   both
"""
import numpy as np
import pytest
import torch

import resnet_layers_ref as t

MARGIN = 100.0
G6 = 2e-4

WIDE, VANILLA = ("resnet34", 6), ("vanilla_resnet34", 27)
# (plan, frame, layer, mutation)
CASES = [
    (WIDE, (126, 202), "backbone.layer1.1.conv1.weight", "prepad"),
    (WIDE, (126, 202), "backbone.layer2.0.conv1.weight", "prepad"),
    (WIDE, (126, 202), "backbone.layer2.0.conv1.weight", "edge"),
    (WIDE, (126, 202), "backbone.layer2.0.downsample.weight", "edge"),
    (WIDE, (180, 250), "backbone.layer2.0.conv1.weight", "edge"),
    (WIDE, (126, 202), "backbone.layer3.0.downsample.weight", "rawshortcut"),
    (WIDE, (126, 202), "backbone.layer3.0.conv1.weight", "eps"),
    (WIDE, (126, 202), "pool", "pool2"),
    (WIDE, (126, 202), "head", "meanrow"),
    (VANILLA, (126, 202), "backbone.layer4.0.conv1.weight", "edge"),
    (VANILLA, (126, 202), "backbone.layer1.0.conv2.weight", "resafter"),
    (VANILLA, (126, 202), "backbone.layer3.2.conv2.weight", "resafter"),
    (VANILLA, (126, 202), "backbone.conv1.weight", "eps"),
    (VANILLA, (126, 202), "backbone.layer2.0.downsample.0.weight", "eps"),
    (VANILLA, (126, 202), "backbone.layer4.2.conv2.weight", "eps"),
    (VANILLA, (126, 202), "pool", "pool2"),
    (VANILLA, (126, 202), "head", "meanrow"),
]

_cache = {}


def _reference(plan, hw):
    """(weights, input, chained fp64 maps) of a plan at a frame size -- the GPU file's parameters (seed = frame height)."""
    if (plan, hw) not in _cache:
        arch, cin = plan
        w = t.make_weights(arch, cin, hw[0])
        x = t.make_input(3, hw, cin, hw[0])
        _cache[(plan, hw)] = (w, x, t.reference_network(arch, cin, w, x))
    return _cache[(plan, hw)]


@pytest.mark.parametrize("plan,hw,layer,mutation", CASES, ids=[f"{p[0]}-{hw[0]}-{l.replace('backbone.', '')}-{m}" for p, hw, l, m in CASES])
def test_mutation_is_caught_at_its_layer(plan, hw, layer, mutation):
    arch, cin = plan
    w, x, ref = _reference(plan, hw)
    mut = t.reference_network(arch, cin, w, x, mutate=(layer, mutation))
    if layer == "backbone.conv1.weight":
        del mut[layer]  # as under pool fusion: the stem is only seen through the pooled map
    r = t.compare_network(arch, cin, w, x, mut, t.TOL_SPLIT, label=f"mut-{mutation}")
    hit = {"head": ["head.features"], "backbone.conv1.weight": ["pool"]}.get(layer, [layer])
    for k in hit:
        assert r[k] >= MARGIN, (k, r[k])
    others = {k: v for k, v in r.items() if k not in hit}
    assert max(others.values()) <= 0.01, max(others, key=others.get)  # neighbours: consistent with what they were fed
    d = np.abs(mut["features"] - ref["features"]).max() / (G6 * np.abs(ref["features"]).max())
    print(f"G6 {mutation} {arch} {hw[0]}x{hw[1]} {layer} {d:.3f} x the pooled-feature bound; {min(r[k] for k in hit):.0f} x its layer bound")


@pytest.mark.parametrize("plan", [WIDE, VANILLA], ids=["resnet34-6", "vanilla_resnet34-27"])
def test_fp32_bounds_are_attainable(plan):
    """PyTorch's fp32 ``F.conv2d`` / BatchNorm / pooling on the same inputs sits inside every fp32 bound of the table, the
    derived head bound included; the reference rounded to fp32 is far inside."""
    arch, cin = plan
    hw = (126, 202)
    w, x, ref = _reference(plan, hw)
    got = t.reference_network(arch, cin, w, x, dtype=torch.float32)
    assert got["pool"].dtype == np.float32
    r = t.compare_network(arch, cin, w, x, got, t.TOL_SPLIT, label="torch-fp32")
    assert max(r.values()) <= 1.0, (max(r, key=r.get), max(r.values()))
    del got["backbone.conv1.weight"]  # the fused-stem form of the comparison
    assert t.compare_network(arch, cin, w, x, got, t.TOL_SPLIT, only=["pool"], label="torch-fp32-fused")["pool"] <= 1.0
    r64 = t.compare_network(arch, cin, w, x, {k: v.astype(np.float32) if k != "pool" else v for k, v in ref.items()}, t.TOL_SPLIT, label="rounded", head=False)
    assert max(v for k, v in r64.items() if k != "pool") <= 0.01


def test_module_layers_match_the_oracle_shapes():
    """The structure restated in the GPU file names exactly the convolutions of the modules (oracle.backbones.param_shapes)."""
    from oracle import backbones as ob

    for arch, cin in (("vanilla_resnet34", 27), ("resnet34", 6), ("resnet18", 7)):
        layers, pool, last = t.module_layers(arch, cin, (240, 320))
        shapes = {"backbone." + k: v for k, v in ob.param_shapes(arch, cin).items() if len(v) == 4}
        assert {L["name"]: (L["cout"], L["cin"], L["k"], L["k"]) for L in layers} == shapes
        assert (pool["Ho"], pool["Wo"]) == (60, 80) and (layers[-1]["Ho"], layers[-1]["Wo"]) == (8, 10) and last == layers[-1]["name"]
