"""The MBConv kernels of EfficientNet-b3 (csrc/mbconv.hip, csrc/mbconv_front.hip), block by block, against a plain fp64
restatement of the block: full spatial maps, not pooled vectors.

The seam is the caller-described network (``ops.GraphNet``: ``hp_net_add_conv`` / ``hp_net_add_dwconv`` / ``hp_net_add_se``):
it appends the ops ``build_graph_efficientnet`` appends, and ``forward_chunk`` picks every launch as it does for the real
network -- fused front, strip pooling, the ``se_pool_kernel`` fallback.  A graph here is

    input -> [stem 1x1] -> [expand 1x1 + BN + swish] -> depthwise + BN + swish -> [SE -> gated 1x1 projection + BN (+ skip)]

The stem stands for the previous block's projection (no activation; its launch tracks the range of what it writes, as in the
real network); its output is read back and IS the block input of the reference, so it adds nothing to the error budget.

Reference (``reference``): ``F.conv2d`` in double, the asymmetric "same" padding as an explicit ``F.pad`` with the (lo, hi) pads
of a 300-pixel image (``SAME_PAD``), BatchNorm un-folded with eps 1e-3, ``x * sigmoid(x)``, mean over H x W, two linear layers,
sigmoid gate, 1x1 projection, optional skip.  The depthwise BatchNorm is handed to the library un-folded (``pack_dw`` folds it:
its folding is under test); the library's 1x1 layers take a bias only, so the test folds their BatchNorm in double and rounds
once to fp32 (6e-8, far inside the bounds).

Bounds (none of them tuned against the kernels):
  depthwise alone   per output channel 2e-5 of that channel's max|ref| (the form and number of test_split_conv_dynamic_range;
                    generous for fp32 FMAs over <= 25 taps)
  everything else   2e-5 x max(1, max|ref|) per split-fp16 GEMM on the path (test_conv2d_mbconv_features): 1 for depthwise ->
                    SE -> projection and for the depthwise map behind an expansion, 2 for the output of a whole block

Every comparison has teeth: tests/test_mbconv_reference.py (no GPU) runs the same comparison functions on the same cases
with a mutated reference in the place of the kernels' output and requires >= 100x the bound (``MUTATIONS``).

Which case reaches which kernel (launch selection: net.cpp forward_chunk, mbconv.hip launch_dwconv / dw_rows):

  dwconv_strip_kernel<3,1,8>       DW_CASES 0, 10; REAL_BLOCKS 0, 1
  dwconv_strip_kernel<3,1,4>       DW_CASES 1, 6;  BLOCK_STRIP 0; BLOCK_PLAIN 1
  dwconv_strip_kernel<3,2,8>       DW_CASES 2, 11; BLOCK_STRIP 1
  dwconv_strip_kernel<3,2,4>       DW_CASES 3, 9;  BLOCK_FRONT 3 with the front switched off
  dwconv_strip_kernel<5,1,4,true>  DW_CASES 4, 7;  BLOCK_STRIP 3, 4; BLOCK_PLAIN 0
  dwconv_strip_kernel<5,2,4,true>  DW_CASES 5, 8;  BLOCK_STRIP 2; BLOCK_PLAIN 2
  mbconv_front_kernel<3,1,32>      BLOCK_FRONT 0   mbconv_front_kernel<3,1,64>  BLOCK_FRONT 1
  mbconv_front_kernel<3,2,32>      BLOCK_FRONT 2   mbconv_front_kernel<3,2,64>  BLOCK_FRONT 3
  mbconv_front_kernel<5,2,32>      BLOCK_FRONT 4   mbconv_front_kernel<5,2,64>  BLOCK_FRONT 5
  pooled sums: strip partials      BLOCK_STRIP 0, 1, 2, 4; BLOCK_PLAIN
               tile partials       BLOCK_FRONT
               se_pool_kernel      BLOCK_STRIP 3 (33 strips of 4 rows)
The 26 real geometries (REAL_BLOCKS) repeat this at the sizes of the 240 x 320 plan.
Not covered: the ``n >= 65536`` branch of launch_dwconv to dwconv_swish_nhwc (unreachable from a network).

Measured on an MI355X, worst error / bound: 0.030 depthwise alone, 0.024 - 0.030 strip blocks, 0.017 fused / unfused blocks, 0.020 real
geometries (table in CHANGELOG.md).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # also run as a script (the child interpreter of the fused-front A/B)
    sys.path.insert(0, ROOT)

BN_EPS = 1e-3
TOL = 2e-5
# The two SE matrices are scaled 8x above He, the GEMMs He-style (gain about 1).  One row too many in a mean over Ho rows moves
# the pooled vector by about 1 / Ho of itself; with gain-1 SE weights the block output would move by 16x the bound on the
# 132-row map, 100x only at 4x (measured on the fp64 reference alone, tests/test_mbconv_reference.py), so a dead row summed by
# a ragged strip could hide inside the bound.  The GPU tests and the mutation test share these parameters.
SE_SCALE = 8.0
# (kernel, stride) -> (top / left, bottom / right) padding: Conv2dStaticSamePadding for image_size 300
SAME_PAD = {(3, 2): (0, 1), (5, 2): (1, 2), (3, 1): (1, 1), (5, 1): (2, 2)}


def out_size(h, k, s):
    lo, hi = SAME_PAD[(k, s)]
    return (h + lo + hi - k) // s + 1


# ------------------------------------------------------------------------------------------------ cases
# a. depthwise alone: input -> depthwise.  H, W = the input map; C channels
DW_CASES = [
    dict(k=3, s=1, H=60, W=80, C=32, n=1),                 # 0  8-row strips, ragged last strip (60 = 7 x 8 + 4)
    dict(k=3, s=1, H=15, W=20, C=576, n=3),                # 1  4-row strips, 15 = 3 x 4 + 3; 144 quads in 3 shares of 48
    dict(k=3, s=2, H=120, W=160, C=144, n=1),              # 2  pad 0 / 1, Ho = 60; 36 quads: 7 column phases, 4 idle lanes
    dict(k=3, s=2, H=30, W=40, C=240, n=3),                # 3  Ho = 15, Wo = 20
    dict(k=5, s=1, H=30, W=20, C=1152, n=1),               # 4  288 quads in shares of 58: the last workgroup has 56
    dict(k=5, s=2, H=15, W=20, C=2304, n=3),               # 5  pad 1 / 2, Ho = 7, Wo = 10; 9 shares of 64
    dict(k=3, s=1, H=1, W=3, C=144, n=3),                  # 6  Ho = 1, Wo = 3 < 7 column phases
    dict(k=5, s=1, H=7, W=3, C=36, n=5, max_batch=2),      # 7  C % 8 == 4; n > max_batch: chunks 2 + 2 + 1
    dict(k=5, s=2, H=13, W=5, C=32, n=1),                  # 8  odd input, Ho = 6, Wo = 2
    dict(k=3, s=2, H=59, W=19, C=240, n=3),                # 9  odd input: the bottom / right pad is never reached
    dict(k=3, s=1, H=30, W=10, C=2304, n=1),               # 10 8-row strips, 30 = 3 x 8 + 6
    dict(k=3, s=2, H=60, W=6, C=144, n=3),                 # 11 Ho = 30 (8-row strips), Wo = 3 < 7 column phases
]
# b. depthwise -> SE -> gated projection (+ skip): the strip partials, and se_pool_kernel where there are more than 32 strips
BLOCK_STRIP = [
    dict(k=3, s=1, H=15, W=20, C=144, cout=144, cse=6, n=3, skip=True),   # 0  ragged strips must not reach the partials
    dict(k=3, s=2, H=120, W=160, C=40, cout=24, cse=10, n=2),             # 1  8-row strips, 8 partials
    dict(k=5, s=2, H=15, W=20, C=816, cout=232, cse=34, n=3),             # 2  Ho = 7: 2 strips, the second with 3 rows
    dict(k=5, s=1, H=132, W=6, C=32, cout=32, cse=8, n=2, skip=True),     # 3  33 strips of 4 rows > 32: se_pool_kernel
    dict(k=5, s=1, H=15, W=20, C=1152, cout=136, cse=28, n=1),            # 4  last workgroup of 56 quads writes partials too
]
# c. whole block with expansion.  Fused front (mbconv_front_applicable): k3/s1, k3/s2, k5/s2 with Cin <= 32 and 32 < Cin <= 64
BLOCK_FRONT = [
    dict(k=3, s=1, H=30, W=40, cin=32, C=192, cout=32, cse=8, n=3, skip=True),   # 0  8 x 16 tiles: 30 and 40 do not divide
    dict(k=3, s=1, H=15, W=20, cin=48, C=288, cout=48, cse=12, n=2, skip=True),  # 1  Kpad 64
    dict(k=3, s=2, H=60, W=80, cin=24, C=144, cout=32, cse=6, n=3),              # 2  4 x 8 tiles, Ho = 30 does not divide
    dict(k=3, s=2, H=30, W=40, cin=48, C=288, cout=96, cse=12, n=2),             # 3  Ho = 15, Wo = 20: neither divides
    dict(k=5, s=2, H=30, W=39, cin=32, C=192, cout=48, cse=8, n=3),              # 4  odd width, Ho = 15, Wo = 19
    dict(k=5, s=2, H=15, W=20, cin=64, C=384, cout=80, cse=16, n=2),             # 5  Cin = Kpad = 64, Ho = 7, Wo = 10
]
# ... and where it does not hold: expansion, strip kernel and SE as separate launches
BLOCK_PLAIN = [
    dict(k=5, s=1, H=15, W=20, cin=32, C=192, cout=32, cse=8, n=3, skip=True),   # k5 / s1 is not instantiated
    dict(k=3, s=1, H=15, W=20, cin=96, C=576, cout=96, cse=24, n=2, skip=True),  # Cin > 64
    dict(k=5, s=2, H=15, W=20, cin=136, C=816, cout=232, cse=34, n=3),           # Cin > 64, stride 2
]


def real_blocks(h=240, w=320):
    """The 26 MBConv blocks of EfficientNet-b3 at the map sizes of the ``h x w`` plan (the eff_same_pad rule)."""
    from happypose_amd.models import efficientnet_b3_blocks

    H, W = out_size(h, 3, 2), out_size(w, 3, 2)  # the stem: 3x3 / stride 2
    cases = []
    for (k, s, e, cin, cout, cse) in efficientnet_b3_blocks():
        c = dict(k=k, s=s, H=H, W=W, C=cin * e, cout=cout, cse=cse, n=3, skip=(s == 1 and cin == cout))
        if e != 1:
            c["cin"] = cin
        cases.append(c)
        H, W = out_size(H, k, s), out_size(W, k, s)
    return cases, (H, W)


REAL_BLOCKS, REAL_LAST = real_blocks()


def case_id(c):
    return "k{k}s{s}_{H}x{W}_".format(**c) + (f"{c['cin']}-" if "cin" in c else "") + f"{c['C']}" + \
        (f"-{c['cout']}" if "cout" in c else "") + f"_n{c['n']}"


# ------------------------------------------------------------------------------------------------ parameters
def make_params(c, seed=0, se_scale=SE_SCALE, stem=None):
    """Random fp32 parameters of the case, He-scaled so that every layer's gain is about 1.  The BatchNorm statistics are
    random, with running variances of 0.01 .. 0.1 (so that eps 1e-3 matters: 0.5 - 5 % of the scale) and gammas that undo them."""
    rs = np.random.RandomState(1000 + seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    C, k = c["C"], c["k"]
    cb = c.get("cin", C)  # channels of the block input
    stem = ("cout" in c) if stem is None else stem

    def bn(ch):
        var = rs.uniform(0.01, 0.1, ch)
        return dict(weight=f(rs.uniform(0.5, 1.5, ch) * np.sqrt(var + BN_EPS)), bias=f(0.5 * rs.normal(size=ch)),
                    running_mean=f(0.3 * rs.normal(size=ch)), running_var=f(var))

    p = dict(case=c, stem=stem, cb=cb)
    p["x"] = f(rs.normal(size=(c["n"], c["H"], c["W"], 8 if stem else cb)))
    if stem:
        p["stem_w"], p["stem_b"] = f(rs.normal(size=(cb, 8)) / np.sqrt(8)), f(0.5 * rs.normal(size=cb))
    if "cin" in c:
        p["expand_w"], p["bn0"] = f(rs.normal(size=(C, cb)) / np.sqrt(cb)), bn(C)
    p["dw_w"], p["bn1"] = f(rs.normal(size=(C, 1, k, k)) / k), bn(C)
    if "cout" in c:
        cse, cout = c["cse"], c["cout"]
        p["se_w1"], p["se_b1"] = f(se_scale * rs.normal(size=(cse, C)) / np.sqrt(C)), f(0.5 * rs.normal(size=cse))
        p["se_w2"], p["se_b2"] = f(se_scale * rs.normal(size=(C, cse)) / np.sqrt(cse)), f(rs.normal(size=C))
        p["project_w"], p["bn2"] = f(rs.normal(size=(cout, C)) * 2.0 / np.sqrt(C)), bn(cout)  # x 2: the gate halves its input
    return p


# ------------------------------------------------------------------------------------------------ fp64 reference
MUTATIONS = ("sympad", "edge", "row", "nogate", "eps")


def _bn(t, b, eps):
    v = lambda a: torch.as_tensor(a).double().view(1, -1, 1, 1)  # noqa: E731
    return (t - v(b["running_mean"])) / torch.sqrt(v(b["running_var"]) + eps) * v(b["weight"]) + v(b["bias"])


def _swish(t):
    return t * torch.sigmoid(t)


def reference(p, x_block, mutate=None):
    """fp64 MBConv block on the block input ``x_block [n,H,W,Cb]``: ``{"dw": [n,Ho,Wo,C], "out": [n,Ho,Wo,Cout]}``.
    ``mutate`` breaks ONE thing, the way a kernel could (tests/test_mbconv_reference.py):
      sympad  symmetric padding k // 2 instead of the (lo, hi) pads
      edge    the padding repeats the border pixel instead of zeros: only border outputs differ
      row     the SE mean sums one output row too many (a ragged strip's dead row), still divided by Ho x Wo
      nogate  the gate left out
      eps     the depthwise BatchNorm folded with eps 1e-5"""
    assert mutate is None or mutate in MUTATIONS
    c = p["case"]
    k, s, C = c["k"], c["s"], c["C"]
    lo, hi = SAME_PAD[(k, s)]
    Ho, Wo = out_size(c["H"], k, s), out_size(c["W"], k, s)
    x = torch.as_tensor(x_block).double().permute(0, 3, 1, 2)
    t = x
    if "cin" in c:
        t = _swish(_bn(F.conv2d(t, torch.as_tensor(p["expand_w"]).double()[:, :, None, None]), p["bn0"], BN_EPS))
    if mutate == "sympad":
        tp = F.pad(t, (k // 2,) * 4)
    elif mutate == "edge":
        tp = F.pad(t, (lo, hi, lo, hi), mode="replicate")
    else:
        tp = F.pad(t, (lo, hi, lo, hi))  # (left, right, top, bottom)
    wd = torch.as_tensor(p["dw_w"]).double()

    def dw(inp):
        return _swish(_bn(F.conv2d(inp, wd, stride=s, groups=C), p["bn1"], 1e-5 if mutate == "eps" else BN_EPS))

    d = dw(tp)[:, :, :Ho, :Wo]
    assert d.shape[2:] == (Ho, Wo)
    res = {"dw": d.permute(0, 2, 3, 1).numpy()}
    if "cout" not in c:
        return res
    pooled = d.mean((2, 3))
    if mutate == "row":
        d1 = dw(F.pad(tp, (0, 0, 0, s)))[:, :, :Ho + 1, :Wo]
        assert d1.shape[2] == Ho + 1
        pooled = d1.sum((2, 3)) / (Ho * Wo)
    d64 = lambda a: torch.as_tensor(a).double()  # noqa: E731
    sq = _swish(pooled @ d64(p["se_w1"]).T + d64(p["se_b1"]))
    gate = torch.sigmoid(sq @ d64(p["se_w2"]).T + d64(p["se_b2"]))
    g = d if mutate == "nogate" else d * gate[:, :, None, None]
    y = _bn(F.conv2d(g, d64(p["project_w"])[:, :, None, None]), p["bn2"], BN_EPS)
    if c.get("skip"):
        y = y + x
    res["out"] = y.permute(0, 2, 3, 1).numpy()
    return res


def stem_reference(p):
    """The block input the stem makes of ``p["x"]`` (fp64; the GPU tests use the stem's own read-back output instead)."""
    if not p["stem"]:
        return p["x"].astype(np.float64)
    return p["x"].astype(np.float64) @ p["stem_w"].astype(np.float64).T + p["stem_b"].astype(np.float64)


# ------------------------------------------------------------------------------------------------ comparisons
def ratio_dw(y, ref):
    """Depthwise alone: worst over the output channels of max|y - ref| / (2e-5 x the channel's max|ref|); <= 1 passes."""
    C = ref.shape[-1]
    err = np.abs(np.asarray(y, np.float64) - ref).reshape(-1, C).max(0)
    scale = np.abs(ref).reshape(-1, C).max(0)
    assert (scale > 0).all()
    return float((err / (TOL * scale)).max())


def ratio_map(y, ref, gemms):
    """max|y - ref| / (gemms x 2e-5 x max(1, max|ref|)); <= 1 passes."""
    return float(np.abs(np.asarray(y, np.float64) - ref).max() / (gemms * TOL * max(1.0, np.abs(ref).max())))


# ------------------------------------------------------------------------------------------------ the GPU side
def _fold(w, b):
    """1x1 conv weight [Cout][Cin] + BatchNorm -> weight, bias (folded in double, rounded once)."""
    sc = b["weight"].astype(np.float64) / np.sqrt(b["running_var"].astype(np.float64) + BN_EPS)
    return (w.astype(np.float64) * sc[:, None]).astype(np.float32), (b["bias"] - b["running_mean"] * sc).astype(np.float32)


def build_net(p, dev, max_batch=None):
    """The case as a caller-described network.  Slots: 3 = block input (stem), 0 = expanded, 1 = depthwise, 2 = block output."""
    from happypose_amd import ops

    c = p["case"]
    k, s, C, H, W, cb = c["k"], c["s"], c["C"], c["H"], c["W"], p["cb"]
    Ho, Wo = out_size(H, k, s), out_size(W, k, s)
    sd, layers, outputs = {}, [], []
    src = -1
    if p["stem"]:
        sd["stem.weight"], sd["stem.bias"] = p["stem_w"], p["stem_b"]
        layers.append(dict(weight="stem.weight", bias="stem.bias", cin=8, cout=cb, k=1, H=H, W=W, src=-1, dst=3))
        src = 3
    blk_in = src
    if "cin" in c:
        sd["expand.weight"], sd["expand.bias"] = _fold(p["expand_w"], p["bn0"])
        layers.append(dict(weight="expand.weight", bias="expand.bias", cin=cb, cout=C, k=1, relu=2, H=H, W=W, src=src, dst=0))
        src = 0
    sd["blk._depthwise_conv.weight"] = p["dw_w"]
    sd.update({f"blk._bn1.{n}": v for n, v in p["bn1"].items()})
    layers.append(dict(kind="dw", weight="blk._depthwise_conv.weight", bn="blk._bn1", C=C, k=k, stride=s, pad=SAME_PAD[(k, s)][0],
                       H=H, W=W, Ho=Ho, Wo=Wo, src=src, dst=1))
    outputs.append((1, Ho, Wo, C))
    if "cout" in c:
        sd["blk._se_reduce.weight"], sd["blk._se_reduce.bias"] = p["se_w1"], p["se_b1"]
        sd["blk._se_expand.weight"], sd["blk._se_expand.bias"] = p["se_w2"], p["se_b2"]
        sd["project.weight"], sd["project.bias"] = _fold(p["project_w"], p["bn2"])
        layers.append(dict(kind="se", prefix="blk", C=C, Cse=c["cse"], H=Ho, W=Wo, src=1))
        assert not c.get("skip") or blk_in >= 0
        layers.append(dict(weight="project.weight", bias="project.bias", cin=C, cout=c["cout"], k=1, gated=True, H=Ho, W=Wo,
                           src=1, dst=2, res=blk_in if c.get("skip") else -1))
        outputs.append((2, Ho, Wo, c["cout"]))
    if p["stem"]:
        outputs.append((3, H, W, cb))
    return ops.GraphNet(p["x"].shape[-1], H, W, layers, outputs, sd, max_batch=max_batch or c.get("max_batch", c["n"]), device=dev)


def run_case(p, dev, x=None, net=None):
    """``{"dw", "out", "in"}`` maps of the case on the GPU (numpy); ``in`` = the block input the kernels saw."""
    net = net or build_net(p, dev)
    x = p["x"] if x is None else x
    maps = [m.cpu().numpy() for m in net.run(torch.as_tensor(x, device=dev))]
    got = {"dw": maps[0]}
    if "cout" in p["case"]:
        got["out"] = maps[1]
    got["in"] = maps[-1] if p["stem"] else x
    return got


def check_block(p, got, group, gemms_dw, gemms_out):
    """Both maps of a block against fp64 on the block input the kernels saw; returns the two error / bound ratios."""
    ref = reference(p, got["in"])
    r_dw = ratio_map(got["dw"], ref["dw"], gemms_dw) if gemms_dw else ratio_dw(got["dw"], ref["dw"])
    r_out = ratio_map(got["out"], ref["out"], gemms_out)
    print(f"RATIO {group} {case_id(p['case'])} dw {r_dw:.3f} out {r_out:.3f}")
    assert np.isfinite(got["out"]).all() and got["out"].shape == ref["out"].shape
    assert r_dw <= 1.0 and r_out <= 1.0, (r_dw, r_out)
    return r_dw, r_out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the MI355X box"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("i", range(len(DW_CASES)), ids=[case_id(c) for c in DW_CASES])
def test_depthwise_vs_fp64(dev, i):
    """a. input -> depthwise: the full map, per output channel."""
    p = make_params(DW_CASES[i], seed=i)
    got = run_case(p, dev)
    ref = reference(p, p["x"])["dw"]
    assert got["dw"].shape == ref.shape
    r = ratio_dw(got["dw"], ref)
    print(f"RATIO dw {case_id(p['case'])} {r:.3f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("i", range(len(BLOCK_STRIP)), ids=[case_id(c) for c in BLOCK_STRIP])
def test_depthwise_se_projection_vs_fp64(dev, i):
    """b. depthwise -> SE -> gated projection (+ skip): pooling partials of the strip kernel, or se_pool_kernel (case 3).  The
    depthwise map keeps its per-channel bound; one split-fp16 GEMM on the way to the block output."""
    p = make_params(BLOCK_STRIP[i], seed=20 + i)
    check_block(p, run_case(p, dev), "strip", 0, 1)


@pytest.mark.parametrize("i", range(len(BLOCK_PLAIN)), ids=[case_id(c) for c in BLOCK_PLAIN])
def test_block_unfused_vs_fp64(dev, i):
    """c. whole blocks the fused front does not take: expansion, strip kernel, SE, projection as separate launches."""
    p = make_params(BLOCK_PLAIN[i], seed=40 + i)
    check_block(p, run_case(p, dev), "plain", 1, 2)


def _front_params(i):
    return make_params(BLOCK_FRONT[i], seed=60 + i)


@pytest.fixture(scope="module")
def unfused_maps(tmp_path_factory):
    """The BLOCK_FRONT cases with HP_NO_MBCONV_FRONT=1.  Switches are read once per process: one child interpreter runs them
    all and leaves the maps in an .npz (the pattern of tools/stem_ab.py)."""
    path = str(tmp_path_factory.mktemp("mbconv_ab") / "unfused.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "dump-front", path], capture_output=True, text=True, timeout=900,
                       env={**os.environ, "HP_NO_MBCONV_FRONT": "1"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(path)


@pytest.mark.parametrize("i", range(len(BLOCK_FRONT)), ids=[case_id(c) for c in BLOCK_FRONT])
def test_block_fused_front_vs_fp64_and_unfused(dev, unfused_maps, i):
    """c. whole blocks whose expansion + depthwise + pooling sums run as ONE launch (mbconv_front_kernel), and the same case with
    the switch off: both sides within the fp64 bound, and the depthwise maps NOT bit-identical -- otherwise the switch selected
    nothing and the fused kernel is not what ran."""
    p = _front_params(i)
    got = run_case(p, dev)
    check_block(p, got, "front", 1, 2)
    old = {k: unfused_maps[f"{i}_{k}"] for k in ("dw", "out", "in")}
    assert np.array_equal(old["in"], got["in"])  # the stem is the same launch on both sides
    check_block(p, old, "front-off", 1, 2)
    assert not np.array_equal(old["dw"], got["dw"]), "HP_NO_MBCONV_FRONT changed nothing: which kernel ran?"


@pytest.fixture(scope="module")
def b3_plan_blocks(dev):
    """The 26 blocks as the op list of a finalized ``efficientnet-b3`` network at 240 x 320 states them (``hp_net_op_info``):
    one dict per depthwise op in the form of REAL_BLOCKS, the expansion before it and the squeeze-excitation / projection after it
    supplying cin, cse and cout."""
    from happypose_amd import ops
    from happypose_amd.models import pose_model_param_shapes
    from happypose_amd.synthetic import named_weights

    net = ops.Net("efficientnet-b3", 6, named_weights(pose_model_param_shapes("efficientnet-b3", 6, pose_dim=9), seed=0), max_batch=1, device=dev)
    ol = net.op_list()
    blocks = []
    for i, o in enumerate(ol):
        if o["kind"] != "dw":
            continue
        se, proj, prev = ol[i + 1], ol[i + 2], ol[i - 1]
        assert se["kind"] == "se" and proj["kind"] == "conv" and proj["name"].endswith("._project_conv.weight")
        assert o["pad"] == SAME_PAD[(o["k"], o["stride"])][0] and se["H"] == o["Ho"] * o["Wo"] and se["Cin"] == o["Cin"]
        c = dict(k=o["k"], s=o["stride"], H=o["H"], W=o["W"], C=o["Cin"], cout=proj["Cout"], cse=se["Cout"], n=3,
                 skip=proj["res_slot"] >= 0)
        if prev["kind"] == "conv" and prev["name"].endswith("._expand_conv.weight"):
            c["cin"] = prev["Cin"]
        blocks.append((c, (o["Ho"], o["Wo"])))
    return blocks


@pytest.mark.parametrize("i", range(len(REAL_BLOCKS)), ids=[f"b{i}_" + case_id(c) for i, c in enumerate(REAL_BLOCKS)])
def test_real_block_geometries_vs_fp64(dev, b3_plan_blocks, i):
    """d. each of the 26 blocks of EfficientNet-b3 at its map size in the 240 x 320 plan, batch 3.  The sizes follow the
    eff_same_pad rule here AND are read from the op list of a finalized network: the two must agree block by block, and the
    last one must be the 7 x 10 of the network's feature map."""
    assert len(REAL_BLOCKS) == 26 and REAL_LAST == (7, 10)
    assert [(c["H"], c["W"]) for c in REAL_BLOCKS[:2] + REAL_BLOCKS[2:3]] == [(120, 160)] * 3
    assert len(b3_plan_blocks) == 26 and b3_plan_blocks[i][0] == REAL_BLOCKS[i], (b3_plan_blocks[i][0], REAL_BLOCKS[i])
    assert b3_plan_blocks[-1][1] == REAL_LAST
    p = make_params(REAL_BLOCKS[i], seed=100 + i)
    expanded = "cin" in REAL_BLOCKS[i]
    check_block(p, run_case(p, dev), "real", 1 if expanded else 0, 2 if expanded else 1)


def test_fused_front_range_guard(dev):
    """e. A block input beyond the fp16 range (7e4) becomes inf in the fp16 halves the fused front stages.  The guard must flag
    it (STATUS_NONFINITE) and put the network on the exact-fp32 kernels, where the SAME input meets the bound -- the poisoned
    image and the clean ones each against their own scale.  (test_split_fp16_overflow_guard covers the ResNets only.)  The
    SE weights are small here, so that the gate is not a saturated sigmoid of a 1e4-sized argument: a saturated gate would
    make the block output a discontinuous function of the pooled sums, and no bound on round-off would mean anything."""
    from happypose_amd import ops

    c = dict(k=3, s=2, H=60, W=80, cin=24, C=144, cout=32, cse=6, n=3)
    p = make_params(c, seed=90, se_scale=1e-3, stem=False)
    net = build_net(p, dev)
    got = run_case(p, dev, net=net)
    assert net.status() == 0
    check_block(p, got, "guard-clean", 1, 2)
    x = p["x"].copy()
    x[1, 20:28, 30:42, :] = 7.0e4
    run_case(p, dev, x=x, net=net)
    flags = net.status()
    assert flags & ops.STATUS_NONFINITE and flags & ops.STATUS_EXACT_ONLY, flags
    got = run_case(p, dev, x=x, net=net)  # repeated: exact-fp32 kernels now
    assert net.status() == ops.STATUS_EXACT_ONLY
    ref = reference(p, x)
    for name, sel in (("poisoned", slice(1, 2)), ("clean", slice(0, 1)), ("clean", slice(2, 3))):
        r_dw, r_out = ratio_map(got["dw"][sel], ref["dw"][sel], 1), ratio_map(got["out"][sel], ref["out"][sel], 2)
        print(f"RATIO guard-exact {name} dw {r_dw:.3f} out {r_out:.3f}")
        assert np.isfinite(got["out"][sel]).all() and r_dw <= 1.0 and r_out <= 1.0, (name, r_dw, r_out)


def _dump_front(path):
    dev = torch.device("cuda:0")
    out = {}
    for i in range(len(BLOCK_FRONT)):
        for k, v in run_case(_front_params(i), dev).items():
            out[f"{i}_{k}"] = v
    np.savez(path, **out)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "dump-front", "usage: test_gpu_mbconv.py dump-front <out.npz>"
    _dump_front(sys.argv[2])
