"""What every network plan launches, op by op, and what it computes: the record that pins the conv kernel choice
 across a change of the host code (GPU box).

    python tools/net_paths.py dump OUT.json        every combination below, each group in a fresh child process
    python tools/net_paths.py compare A.json B.json [--paths-only KEY ...]
    python tools/net_paths.py golden DUMP.json tests/golden/net_paths.json    the path part of a dump, without the hashes

Uses nothing but the ``ops.Net`` / ``ops.conv2d_nhwc`` API, so the same file runs against another build of the library:
``HAPPYPOSE_AMD_LIB=/path/to/libhappypose_amd.so python tools/net_paths.py dump OUT.json``.

Networks: every ``ops.ARCH`` entry with the weights and inputs of the layer tests (``tests/resnet_layers_ref.py`` at 240 x 320,
3 samples through ``max_batch=2``: one full and one ragged chunk; the EfficientNet plan of ``tests/test_gpu_mbconv.py``; the
FPN plan of ``tests/test_gpu_detector.py``), each precision the plan has, each of ``ops.CONV_ALGOS``, ``force_exact`` off
and on.  One record per combination: per op ``[name, kind, path, materialised]``, the sha256 of every output, and of a
second forward with profiling on the launch count and the two FLOP sums of ``profile_collect`` as hex doubles.  The fp32
ResNets run again with ``HP_NET_NO_SHORTCUT_FUSION=1`` and with ``HP_PROFILE_LAYERS=1``: the library reads those once, at
start-up, hence the child processes.  Single layers: the case table of ``test_conv3x3_kernel_families`` and the default
case list of ``tools/conv_fuzz.py`` under every ``select_conv_algo`` family, sha256 of ``y``."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HW, N, MAX_BATCH = (240, 320), 3, 2
RESNETS = [("vanilla_resnet34", 9), ("resnet34", 6), ("resnet18", 6)]
NETS = [(a, c, p) for a, c in RESNETS for p in ("f32", "f16")] + [("efficientnet-b3", 6, "f32"), ("resnet50-fpn", 3, "f32")]
# group -> (environment of the child, the networks it runs)
GROUPS = {"plain": ({}, NETS),
          "no_shortcut_fusion": ({"HP_NET_NO_SHORTCUT_FUSION": "1"}, [(a, c, "f32") for a, c in RESNETS]),
          "profile_layers": ({"HP_PROFILE_LAYERS": "1"}, [(a, c, "f32") for a, c in RESNETS]),
          "layers": ({}, [])}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def make_net(arch, cin, precision, dev):
    """-> (net, input [n, h, w, cin] as numpy, n)"""
    import numpy as np
    from happypose_amd import ops

    if arch == "resnet50-fpn":  # DetectorBackbone's network on preprocessed images (the plan is what matters here)
        from happypose_amd.synthetic import named_weights
        from oracle import detector as od

        w = named_weights(od.param_shapes(), seed=3)
        w = {k: v for k, v in w.items() if k.startswith(("backbone.", "rpn.head."))}
        x = np.random.RandomState(5).uniform(-1, 1, size=(2, 128, 160, 3)).astype(np.float32)
        return ops.Net(arch, 3, w, max_batch=2, device=dev, h=128, w=160), x, 2
    from resnet_layers_ref import make_input, make_weights

    if arch == "efficientnet-b3":
        from happypose_amd.models import pose_model_param_shapes
        from happypose_amd.synthetic import named_weights

        w = named_weights(pose_model_param_shapes(arch, cin, pose_dim=9), seed=0)
    else:
        w = make_weights(arch, cin, 0)
    net = ops.Net(arch, cin, w, max_batch=MAX_BATCH, device=dev, h=HW[0], w=HW[1], precision=precision)
    return net, make_input(N, HW, cin, 0), N


def run_net(arch, cin, precision, dev, algos=None, exact=(False, True)):
    """One network, the algorithms switched through ``set_conv_algo``: {key: record}."""
    import torch
    from happypose_amd import ops

    net, x, n = make_net(arch, cin, precision, dev)
    fpn = arch == "resnet50-fpn"
    out = {}
    for ex in exact:
        net.force_exact(ex)
        xin = net.new_input(n)  # (an fp16 plan forced exact takes fp32 records: its fp32 sibling runs)
        xin[..., :cin] = torch.as_tensor(x, device=dev).to(xin.dtype)
        for algo in algos or ops.CONV_ALGOS:
            net.set_conv_algo(algo)
            res = net.forward(xin, want_pose=not fpn, want_logits=not fpn and net.n_logits > 0, want_features=not fpn)
            maps = net.feature_maps(n) if fpn else [t for t in res if t is not None]
            torch.cuda.synchronize(dev)
            rec = dict(ops=[[o["name"], o["kind"], o["path"], o["materialised"]] for o in net.op_list()],
                       status=net.status(), sha256=[sha(t) for t in maps])
            net.set_profiling(True)
            net.forward(xin, want_pose=not fpn, want_features=not fpn)
            _, launches, flops, mfma = net.profile_collect()
            net.set_profiling(False)
            rec["profile"] = [launches, float(flops).hex(), float(mfma).hex()]
            out[f"{arch}-{cin}/{precision}/{algo}/{'exact' if ex else 'default'}"] = rec
    return out


def fuzz_cases(n_cases=60, seed=0):
    """The shapes of tools/conv_fuzz.py's first loop (same generator, same draws)."""
    import numpy as np

    rs = np.random.RandomState(seed)
    for case in range(n_cases):
        kind = ["s1", "s1", "s2", "other"][case % 4]
        h, w = int(rs.randint(2, 70)), int(rs.randint(2, 100))
        cin, cout = 32 * int(rs.randint(1, 9)), 32 * int(rs.randint(1, 9))
        k, s, p = 3, 1, 1
        if kind == "s2":
            cin, cout, s = 64 * int(rs.randint(1, 5)), 128 * int(rs.randint(1, 4)), 2
        elif kind == "other":
            k = int(rs.choice([1, 2, 5, 7]))
            s, p = int(rs.randint(1, 3)), k // 2
            cin = 4 * int(rs.randint(1, 17))
            h, w = max(h, k), max(w, k)
        n = int(rs.choice([1, 2, 3, 5, 17, 40, 129]))
        if n * h * w * max(cin, cout) > 3e8:
            n = max(1, int(3e8 // (h * w * max(cin, cout))))
        pre, res, bias, relu = (bool(rs.randint(2)) for _ in range(4))
        yield dict(n=n, h=h, w=w, cin=cin, cout=cout, k=k, s=s, p=p, bias=bias, res=res, pre=pre, relu=relu)


def run_layers(dev):
    import numpy as np
    import torch
    from happypose_amd import ops
    import test_gpu_kernels as tk

    table = [m for m in tk.test_conv3x3_kernel_families.pytestmark if m.name == "parametrize" and m.args[0] == "case"][0].args[1]
    out = {}
    for src, cases in (("families", table), ("fuzz", list(fuzz_cases()))):
        for i, c in enumerate(cases):
            g = torch.Generator(device=dev)
            g.manual_seed(3)
            rn = lambda *shape: torch.randn(*shape, generator=g, device=dev)  # noqa: E731
            ho, wo = (c["h"] + 2 * c["p"] - c["k"]) // c["s"] + 1, (c["w"] + 2 * c["p"] - c["k"]) // c["s"] + 1
            x = rn(c["n"], c["h"], c["w"], c["cin"])
            w = rn(c["cout"], c["k"], c["k"], c["cin"]) / float(np.sqrt(c["cin"] * c["k"] ** 2))
            bias = rn(c["cout"]) if c["bias"] else None
            res = rn(c["n"], ho, wo, c["cout"]) if c["res"] else None
            pre = (torch.rand(c["cin"], generator=g, device=dev) + 0.5, rn(c["cin"])) if c["pre"] else (None, None)
            args = [x, w, c["s"], c["p"], bias, res, pre[0], pre[1], c["relu"]]
            for algo in ops.CONV_ALGOS:
                ops.select_conv_algo(algo)
                out[f"layer/{src}{i:02d}/{algo}"] = dict(case=c, sha256=[sha(ops.conv2d_nhwc(*args))])
            ops.select_conv_algo("auto")
    return out


def child(group, path):
    import torch

    dev = torch.device("cuda:0")
    out = {}
    if group == "layers":
        out = run_layers(dev)
    for arch, cin, precision in GROUPS[group][1]:
        out.update({f"{group}/{k}": v for k, v in run_net(arch, cin, precision, dev).items()})
    with open(path, "w") as f:
        json.dump(out, f)


def dump(path):
    merged = {}
    for group, (env, _) in GROUPS.items():
        part = f"{path}.{group}.part"
        subprocess.run([sys.executable, os.path.abspath(__file__), "child", group, part], env={**os.environ, **env}, check=True,
                       timeout=600)
        with open(part) as f:
            merged.update(json.load(f))
        os.remove(part)
    with open(path, "w") as f:
        json.dump(merged, f, indent=0, sort_keys=True)
    print(f"{len(merged)} records -> {path}")


def path_part(d):
    """The part of a dump that does not depend on the arithmetic, in the form of tests/golden/net_paths.json: per network the
    ops ``[name, kind]``, the distinct ``(paths, materialised)`` tables, and per record its table and its accounting."""
    nets, tables, records = {}, [], {}
    for k in sorted(d):
        v = d[k]
        if "ops" not in v:
            continue
        nets.setdefault("/".join(k.split("/")[1:3]), [o[:2] for o in v["ops"]])
        t = dict(paths=[o[2] for o in v["ops"]], materialised="".join("01"[bool(o[3])] for o in v["ops"]))
        if t not in tables:
            tables.append(t)
        records[k] = dict(table=tables.index(t), profile=v["profile"])
    return dict(nets=nets, tables=tables, records=records)


def golden_ops(g, key):
    """The ``ops`` list of record ``key`` as a dump states it, from the golden's form."""
    t = g["tables"][g["records"][key]["table"]]
    return [[n, k, p, m == "1"] for (n, k), p, m in zip(g["nets"]["/".join(key.split("/")[1:3])], t["paths"], t["materialised"])]


def compare(a_path, b_path, paths_only=()):
    with open(a_path) as f:
        a = json.load(f)
    with open(b_path) as f:
        b = json.load(f)
    bad = sorted(set(a) ^ set(b))
    for k in sorted(set(a) & set(b)):
        ra, rb = a[k], b[k]
        if k in paths_only:
            ra, rb = ({f: v for f, v in r.items() if f != "sha256"} for r in (ra, rb))
        if ra != rb:
            bad.append(k)
            print("DIFFERS", k, [f for f in set(ra) | set(rb) if ra.get(f) != rb.get(f)])
    print(f"{len(a)} / {len(b)} records, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "child":
        child(sys.argv[2], sys.argv[3])
    elif cmd == "dump":
        dump(sys.argv[2])
    elif cmd == "compare":
        rest = sys.argv[4:]
        sys.exit(compare(sys.argv[2], sys.argv[3], rest[1:] if rest[:1] == ["--paths-only"] else ()))
    elif cmd == "golden":
        with open(sys.argv[2]) as f:
            g = path_part(json.load(f))
        with open(sys.argv[3], "w") as f:
            json.dump(g, f, sort_keys=True, separators=(",", ":"))
    else:
        sys.exit(__doc__)
