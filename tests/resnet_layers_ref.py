"""fp64 restatement of the ResNet-34 / WideResNet modules, layer by layer, and the comparison functions built on it: shared by
tests/test_gpu_resnet_layers.py (the kernels' maps) and tests/test_resnet_layers_reference.py (mutated references, no GPU).
What is compared, with which bound and why: the docstring of tests/test_gpu_resnet_layers.py."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
TOL_SPLIT, TOL_EXACT, TOL_F16 = 2e-5, 4e-5, 1.5e-3
U32 = 2.0 ** -24
_LAYERS = {"vanilla_resnet34": [3, 4, 6, 3], "resnet34": [3, 4, 6, 3], "resnet18": [2, 2, 2, 2]}
_PLANES = [64, 128, 256, 512]
FUSED_STEMS = ("stem7_pool", "stem7_pool_f16", "stem_split_pool", "igemm_split_pool")


# ------------------------------------------------------------------------------------------------ parameters
def make_weights(arch, cin, seed=0):
    """``predictor_weights`` of the predictor (pose 9, one logit) with non-trivial BatchNorm statistics: running variances of
    0.01 .. 0.1 (eps 1e-5 vs 1e-3 then moves a scale by 0.5 - 5 %: a wrong eps cannot hide), gammas that undo them (the gain
    stays that of ``named_weights``), running means and betas of 0.3 sigma."""
    from happypose_amd.models import pose_model_param_shapes
    from happypose_amd.synthetic import predictor_weights

    w = predictor_weights(pose_model_param_shapes(arch, cin, pose_dim=9, n_views_logits=1), seed=seed, update_scale=0.05)
    for name in [k for k in w if k.endswith(".running_var")]:
        p = name[: -len(".running_var")]
        rs = np.random.RandomState((zlib.crc32(p.encode()) ^ (seed + 77)) & 0x7FFFFFFF)
        c = w[name].shape[0]
        var = rs.uniform(0.01, 0.1, c)
        w[name] = var.astype(np.float32)
        w[p + ".weight"] = (rs.uniform(0.5, 1.5, c) * np.sqrt(var + BN_EPS)).astype(np.float32)
        w[p + ".running_mean"] = (0.3 * rs.normal(size=c)).astype(np.float32)
        w[p + ".bias"] = (0.3 * rs.normal(size=c)).astype(np.float32)
    return w


def make_input(n, hw, cin, seed=0):
    return np.random.RandomState(500 + seed).uniform(-1, 1, size=(n, hw[0], hw[1], cin)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ module structure
def module_layers(arch, cin, hw):
    """The conv layers of the module in the order the module runs them, each with the NAMES of the maps it reads: ``src``
    (``"input"``, ``"pool"`` or a weight name) and ``res``; geometry from the module's own rules."""
    vanilla = arch == "vanilla_resnet34"
    k1 = 7 if vanilla else 5
    bb = "backbone."
    o = lambda h, k, s, p: (h + 2 * p - k) // s + 1  # noqa: E731
    H, W = o(hw[0], k1, 2, k1 // 2), o(hw[1], k1, 2, k1 // 2)
    L = [dict(name=bb + "conv1.weight", role="stem", src="input", res=None, bn_after=bb + "bn1", bn_before=None, k=k1, stride=2,
              pad=k1 // 2, relu=True, cin=cin, cout=64, H=hw[0], W=hw[1], Ho=H, Wo=W)]
    pool = dict(H=H, W=W, Ho=o(H, 3, 2, 1), Wo=o(W, 3, 2, 1))
    H, W = pool["Ho"], pool["Wo"]
    cur, inpl = "pool", 64
    for li, (planes, nb) in enumerate(zip(_PLANES, _LAYERS[arch]), start=1):
        for b in range(nb):
            s = 2 if (b == 0 and li > 1) else 1
            p = f"{bb}layer{li}.{b}"
            ds = s != 1 or inpl != planes
            Ho, Wo = o(H, 3, s, 1), o(W, 3, s, 1)
            g = dict(H=H, W=W, Ho=Ho, Wo=Wo, cin=inpl, cout=planes)
            c1, c2 = p + ".conv1.weight", p + ".conv2.weight"
            if vanilla:
                dn = p + ".downsample.0.weight"
                L.append(dict(g, name=c1, role="conv1", src=cur, res=None, bn_after=p + ".bn1", bn_before=None, k=3, stride=s, pad=1, relu=True))
                if ds:
                    L.append(dict(g, name=dn, role="down", src=cur, res=None, bn_after=p + ".downsample.1", bn_before=None, k=1, stride=s,
                                  pad=0, relu=False))
                L.append(dict(name=c2, role="conv2", src=c1, res=dn if ds else cur, bn_after=p + ".bn2", bn_before=None, k=3, stride=1,
                              pad=1, relu=True, cin=planes, cout=planes, H=Ho, W=Wo, Ho=Ho, Wo=Wo))
            else:
                dn = p + ".downsample.weight"
                if ds:  # the module computes the shortcut first, on the activated input
                    L.append(dict(g, name=dn, role="down", src=cur, res=None, bn_after=None, bn_before=p + ".bn1", k=1, stride=s, pad=0,
                                  relu=False))
                L.append(dict(g, name=c1, role="conv1", src=cur, res=None, bn_after=p + ".bn2", bn_before=p + ".bn1", k=3, stride=s, pad=1,
                              relu=True))
                L.append(dict(name=c2, role="conv2", src=c1, res=dn if ds else cur, bn_after=None, bn_before=None, k=3, stride=1, pad=1,
                              relu=False, cin=planes, cout=planes, H=Ho, W=Wo, Ho=Ho, Wo=Wo))
            cur, inpl, H, W = c2, planes, Ho, Wo
    return L, pool, cur


# ------------------------------------------------------------------------------------------------ fp64 reference, one layer
MUTATIONS = ("prepad", "edge", "rawshortcut", "resafter", "pool2", "eps", "meanrow")


def _nchw(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _v(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype).view(1, -1, 1, 1)


def _affine32(w, p):
    """scale, shift of a BatchNorm as the library folds it: fp32 IEEE operations (net.cpp bn_affine)."""
    g, b, m, v = (np.asarray(w[f"{p}.{k}"], np.float32) for k in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(v + np.float32(BN_EPS))
    return s, b - m * s


def _bn(t, w, p, eps, dtype):
    return (t - _v(w[p + ".running_mean"], dtype)) / torch.sqrt(_v(w[p + ".running_var"], dtype) + eps) * _v(w[p + ".weight"], dtype) + \
        _v(w[p + ".bias"], dtype)


def layer_ref(w, L, src, res=None, mutate=None, f16=False, dtype=torch.float64):
    """One conv layer of the module on the NHWC map ``src`` (+ ``res``): NHWC, ``dtype``.  ``mutate`` breaks ONE thing, the
    way a kernel could (tests/test_resnet_layers_reference.py):
      prepad       the BN + ReLU prologue applied to the zero padding too (the border sees relu(shift))
      edge         the last output row / column of a stride-2 layer on an odd map reads one pixel off
      rawshortcut  the shortcut fed the un-activated block input
      resafter     the residual added after the ReLU
      eps          the BatchNorm after the conv folded with eps 1e-3
    fp16 plan (``f16``): BN folded in double, weights rounded to fp16 once, prologue = one fp16 rounding of x * s + b with the
    fp16 scale / shift the library uploads."""
    assert mutate is None or mutate in MUTATIONS
    x = _nchw(src, dtype)
    wt = torch.as_tensor(np.asarray(w[L["name"]])).to(dtype)
    pad = L["pad"]

    def prologue(t):
        if not L["bn_before"] or mutate == "rawshortcut":
            return t
        if f16:
            s, b = (a.astype(np.float16).astype(np.float64) for a in _affine32(w, L["bn_before"]))
            y = (t.numpy() * s.reshape(1, -1, 1, 1) + b.reshape(1, -1, 1, 1)).astype(np.float16)  # exact in double, one rounding
            return torch.as_tensor(np.maximum(y, np.float16(0)).astype(np.float64))
        return F.relu(_bn(t, w, L["bn_before"], BN_EPS, dtype))

    def core(t):
        if mutate == "prepad":
            y = F.conv2d(prologue(F.pad(t, (pad,) * 4)), wt_eff, stride=L["stride"])
        else:
            y = F.conv2d(prologue(t), wt_eff, stride=L["stride"], padding=pad)
        if f16 and L["bn_after"]:
            return y + shift16
        return _bn(y, w, L["bn_after"], 1e-3 if mutate == "eps" else BN_EPS, dtype) if L["bn_after"] else y

    wt_eff, shift16 = wt, None
    if f16:
        if L["bn_after"]:
            g, b, m, v = (np.asarray(w[f"{L['bn_after']}.{k}"], np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
            sc = g / np.sqrt(v + BN_EPS)
            wt_eff = wt * torch.as_tensor(sc).view(-1, 1, 1, 1)
            shift16 = torch.as_tensor(b - m * sc).view(1, -1, 1, 1)
        wt_eff = torch.as_tensor(wt_eff.numpy().astype(np.float16).astype(np.float64))
    y = core(x)
    if mutate == "edge":
        assert L["stride"] == 2
        if L["H"] % 2:
            y[:, :, -1, :] = core(F.pad(x, (0, 0, 1, 0))[:, :, :-1])[:, :, -1, :]
        if L["W"] % 2:
            y[:, :, :, -1] = core(F.pad(x, (1, 0, 0, 0))[:, :, :, :-1])[:, :, :, -1]
    if res is not None:
        r = _nchw(res, dtype)
        y = F.relu(y) + r if (mutate == "resafter" and L["relu"]) else y + r
        if L["relu"] and mutate != "resafter":
            y = F.relu(y)
    elif L["relu"]:
        y = F.relu(y)
    assert tuple(y.shape[2:]) == (L["Ho"], L["Wo"])
    return _nhwc(y)


def pool_ref(src, mutate=None):
    """3x3 / stride-2 / pad-1 max-pool of an NHWC map, in the map's own type (a max is exact).  pool2: a 2x2 window."""
    t = torch.as_tensor(np.ascontiguousarray(src)).permute(0, 3, 1, 2)
    t = t.float() if t.dtype == torch.float16 else t
    y = F.max_pool2d(t, 2, 2, 0, ceil_mode=True) if mutate == "pool2" else F.max_pool2d(t, 3, 2, 1)
    return _nhwc(y).astype(np.asarray(src).dtype)


def head_ref(arch, w, last, mutate=None, dtype=np.float64):
    """mean -> [fc] -> pose / logits from the last map (NHWC).  meanrow: the mean sums one row too few."""
    x = np.asarray(last, dtype)
    n, H, W, C = x.shape
    mean = (x[:, :-1].sum((1, 2)) if mutate == "meanrow" else x.sum((1, 2))) / dtype(H * W)
    f = mean
    if arch == "vanilla_resnet34":
        f = mean @ np.asarray(w["backbone.fc.weight"], dtype).T + np.asarray(w["backbone.fc.bias"], dtype)
    return dict(features=f, pose=f @ np.asarray(w["pose_fc.weight"], dtype).T + np.asarray(w["pose_fc.bias"], dtype),
                logits=f @ np.asarray(w["views_logits_head.weight"], dtype).T + np.asarray(w["views_logits_head.bias"], dtype))


def head_check(arch, w, last, got):
    """{"features" | "pose" | "logits": worst |got - ref| / bound}: the a-priori fp32 bound of the module docstring.  Features
    from the last map (mean, and through the fc with the mean's bound carried along: the pooled vector is not an output);
    pose and logits from the FEATURES THE KERNELS WROTE, one dot product each -- isolation as for the layers.  (Chained from
    the map through two 512-term products of absolute values, the bound of the pose is so loose that a mean over one row too
    few stayed at 70x: tests/test_resnet_layers_reference.py.)"""
    x = np.asarray(last, np.float64)
    n, H, W, C = x.shape
    ref = head_ref(arch, w, last)
    e = (H * W + 2) * U32 * np.abs(x).sum((1, 2)) / (H * W)  # [n, C]: error bound of the mean
    f = x.sum((1, 2)) / (H * W)

    def lin(f, e, wn, bn_):
        A, b = np.abs(np.asarray(w[wn], np.float64)), np.abs(np.asarray(w[bn_], np.float64))
        return (A.shape[1] + 2) * U32 * (np.abs(f) @ A.T + b) + e @ A.T

    if arch == "vanilla_resnet34":
        e = lin(f, e, "backbone.fc.weight", "backbone.fc.bias")
    fg = np.asarray(got["features"], np.float64)
    for k, wn in (("pose", "pose_fc"), ("logits", "views_logits_head")):
        ref[k] = fg @ np.asarray(w[wn + ".weight"], np.float64).T + np.asarray(w[wn + ".bias"], np.float64)
    bound = dict(features=e, pose=lin(fg, 0 * e, "pose_fc.weight", "pose_fc.bias"), logits=lin(fg, 0 * e, "views_logits_head.weight", "views_logits_head.bias"))
    out = {}
    for k in ("features", "pose", "logits"):
        assert np.asarray(got[k]).shape == ref[k].shape and (bound[k] > 0).all()
        out[k] = float((np.abs(np.asarray(got[k], np.float64) - ref[k]) / bound[k]).max())
    return out


# ------------------------------------------------------------------------------------------------ comparisons
def ratio_map(y, ref, tol, floor=0.0):
    """(max|y - ref| / (tol x max(floor, max|ref|)), the worst of the same per output channel against the channel's own
    max|ref|).  <= 1 passes the first; the second is printed only."""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    assert np.isfinite(y).all()
    err = np.abs(y - ref)
    scale = max(floor, np.abs(ref).max())
    assert scale > 0
    C = ref.shape[-1]
    cs = np.abs(ref).reshape(-1, C).max(0)
    ce = err.reshape(-1, C).max(0)
    chan = float((ce[cs > 0] / (tol * np.maximum(cs[cs > 0], floor))).max())
    return float(err.max() / (tol * scale)), chan


def compare_network(arch, cin, w, x, maps, tol, f16=False, only=None, label="", head=True):
    """Every layer of the module against ``layer_ref`` on the maps in ``maps`` (name -> NHWC array: weight names, ``"pool"``,
    ``"features"`` / ``"pose"`` / ``"logits"``).  ``x``: the network input as the kernels saw it (channels past ``cin`` are
    padding).  A stem whose map is absent was fused with the pool: the pooled map is then compared with conv -> max-pool of the
    input at the conv bound; otherwise the pooled map must be the bit-exact max of the stem map.  Returns {layer: ratio}."""
    hw = x.shape[1:3]
    layers, _, last = module_layers(arch, cin, hw)
    floor = 1.0 if f16 else 0.0
    out = {}

    def put(name, r, c=None):
        out[name] = r
        print(f"RATIO {label} {name} {r:.4f}" + (f" chan {c:.4f}" if c is not None else ""))

    for L in layers:
        if only is not None and L["name"] not in only and not (L["role"] == "stem" and "pool" in only):
            continue
        src = x[..., :cin] if L["src"] == "input" else maps[L["src"]]
        res = None if L["res"] is None else maps[L["res"]]
        if L["role"] == "stem":
            ref = layer_ref(w, L, src, f16=f16)
            if L["name"] in maps:
                put(L["name"], *ratio_map(maps[L["name"]], ref, tol, floor))
                exact = bool(np.array_equal(pool_ref(maps[L["name"]]), maps["pool"]))
                put("pool", 0.0 if exact else float("inf"))
            else:
                put("pool", *ratio_map(maps["pool"], pool_ref(ref), tol, floor))
            continue
        put(L["name"], *ratio_map(maps[L["name"]], layer_ref(w, L, src, res, f16=f16), tol, floor))
    if head and only is None:
        for k, r in head_check(arch, w, maps[last], maps).items():
            put("head." + k, r)
    return out


def reference_network(arch, cin, w, x, mutate=None, dtype=torch.float64):
    """All maps of the module, chained (name -> NHWC), in ``dtype``; ``mutate = (layer name | "pool" | "head", kind)`` breaks
    that one layer and everything downstream sees it."""
    layers, _, last = module_layers(arch, cin, x.shape[1:3])
    npd = np.float64 if dtype == torch.float64 else np.float32
    m = lambda name: mutate[1] if (mutate and mutate[0] == name) else None  # noqa: E731
    maps = {}
    for L in layers:
        src = x[..., :cin] if L["src"] == "input" else maps[L["src"]]
        maps[L["name"]] = layer_ref(w, L, src, None if L["res"] is None else maps[L["res"]], mutate=m(L["name"]), dtype=dtype)
        if L["role"] == "stem":
            maps["pool"] = pool_ref(maps[L["name"]], mutate=m("pool"))
    maps.update(head_ref(arch, w, maps[last], mutate=m("head"), dtype=npd))
    return maps
