"""Times head training's device path (csrc/head_train.hip) -- head backward over two refiner iterations, the gradient norm and the
fused optimiser step -- at the workload's own sizes against a plain-torch restatement on the same device tensors.

    python tools/head_train_bench.py [--calls 50] [--rounds 7] [--warmup 3]

Shapes: B = 576 and 4608 hypotheses; C = 512 with the 512 x 512 fc in front of the heads (torchvision ResNet-34, MegaPose),
C = 512 without (ResNet-34 / 18, CosyPose) and C = 1536 (EfficientNet-b3); 9 pose rows, and 4 logits rows with a NULL gradient
on the fc path.  The baseline: ``d_out.T @ feat`` per iteration, ``(d_out @ W).T @ pooled`` for the fc, ``clip_grad_norm_`` and
``torch.optim.Adam(fused=False)`` (the reference's optimiser; foreach as torch chooses).

Method (as tools/batch_data_bench.py): every shape is warmed up, both sides' gradients are compared once (1e-4 relative to the
largest entry), then each side runs ``--calls`` calls between two device events, ``--rounds`` times, alternating inside a round;
the figure is the median over the rounds of the time per call, with minimum and maximum.  The time is the call as a user makes
it (argument checks, workspace allocation through torch's caching allocator, launches), not the kernels alone.  Prints one JSON
line.  Needs a GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from happypose_amd import ops  # noqa: E402

N_ITERATIONS = 2
POSE_DIM = 9


def event_ms(fn, calls: int) -> float:
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def case(B: int, C: int, fc: bool, n_logits: int, a) -> dict:
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(B + C)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    O = POSE_DIM + n_logits
    feats, d_poses = [rnd(B, C) for _ in range(N_ITERATIONS)], [rnd(B, POSE_DIM) / B for _ in range(N_ITERATIONS)]
    pooled = [rnd(B, 512) for _ in range(N_ITERATIONS)] if fc else None
    n = O * C + O + (512 * 512 + 512 if fc else 0)
    p0 = rnd(n) * 0.05
    max_norm = torch.full((1,), 1000.0, device=dev)

    # the library
    p, grad, m, v, sq = p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(1, device=dev)
    W, gW, gb = p[:O * C].view(O, C), grad[:O * C].view(O, C), grad[O * C:O * C + O]
    gfw, gfb = (grad[O * C + O:O * C + O + 512 * 512].view(512, 512), grad[O * C + O + 512 * 512:]) if fc else (None, None)
    step = [0]

    def ours():
        for k in range(N_ITERATIONS):
            res = ops.head_backward(feats[k], d_poses[k], W, n_logits=n_logits, dW=gW, db=gb, accumulate=k > 0, return_d_feat=fc)
            if fc:
                ops.fc_backward(res[2], pooled[k], dW=gfw, db=gfb, accumulate=k > 0)
        ops.grad_sq_norm(grad, out=sq)
        step[0] += 1
        ops.adamw_step(p, grad, m, v, lr=3e-4, step=step[0], sq_norm=sq, max_norm=max_norm)

    # plain torch on the same tensors
    tp = [p0[:O * C].view(O, C).clone().requires_grad_(), p0[O * C:O * C + O].clone().requires_grad_()]
    if fc:
        tp += [p0[O * C + O:O * C + O + 512 * 512].view(512, 512).clone().requires_grad_(), p0[O * C + O + 512 * 512:].clone().requires_grad_()]
    opt = torch.optim.Adam(tp, lr=3e-4, fused=False)
    zeros = torch.zeros(B, n_logits, device=dev) if n_logits else None

    def base():
        for k in range(N_ITERATIONS):
            d_out = d_poses[k] if zeros is None else torch.cat([d_poses[k], zeros], 1)
            grads = [d_out.T @ feats[k], d_out.sum(0)]
            if fc:
                d_feat = d_out @ tp[0].detach()
                grads += [d_feat.T @ pooled[k], d_feat.sum(0)]
            for t, gr in zip(tp, grads):
                t.grad = gr if k == 0 else t.grad + gr
        torch.nn.utils.clip_grad_norm_(tp, max_norm=1000.0)
        opt.step()

    for _ in range(a.warmup):
        ours(), base()
    ref = torch.cat([t.grad.reshape(-1) for t in tp])
    err = float((grad - ref).abs().max() / ref.abs().max())
    assert err < 1e-4, f"the two sides disagree: {err}"
    torch.cuda.synchronize()
    t = {"hip": [], "torch": []}
    for _ in range(a.rounds):
        t["hip"].append(event_ms(ours, a.calls))
        t["torch"].append(event_ms(base, a.calls))
    out = {k: {"median_ms": round(statistics.median(x), 4), "min_ms": round(min(x), 4), "max_ms": round(max(x), 4)} for k, x in t.items()}
    return dict(B=B, C=C, fc=fc, n_logits=n_logits, n_params=n, grad_rel_diff=err, **out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "head_train_bench needs a GPU"
    cases = [case(B, C, fc, nl, a) for B in (576, 4608) for C, fc, nl in ((512, True, 4), (512, False, 0), (1536, False, 0))]
    print(json.dumps({"n_iterations": N_ITERATIONS, "calls": a.calls, "rounds": a.rounds, "warmup": a.warmup, "cases": cases}))


if __name__ == "__main__":
    main()
