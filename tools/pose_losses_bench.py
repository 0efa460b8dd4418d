#!/usr/bin/env python3
"""Time one forward plus backward of MegaPose's disentangled refiner loss on the device: ``happypose_amd.losses`` (three launches,
a workspace of B x S x 12 bytes) beside a plain-torch restatement of the same formula with autograd (three ``[B, S, N, 3]``
temporaries, kept for the backward pass), at ``B = 512, S = 64, N = 2000``; both ``torch.cuda.max_memory_allocated`` figures.

A tool, not a test: it prints what it measures and attaches no threshold.  Usage:  python tools/pose_losses_bench.py [--rows 512]
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from happypose_amd import losses  # noqa: E402


def torch_symmetric(gt, pred, pts):
    a = pts[:, None] @ gt[:, :, :3, :3].transpose(-1, -2) + gt[:, :, None, :3, 3]
    b = pts @ pred[:, :3, :3].transpose(-1, -2) + pred[:, None, :3, 3]
    return (b[:, None] - a).flatten(-2, -1).abs().mean(-1).min(dim=1)[0]


def torch_refiner_loss(gt_all, T_in, out, K, pts, tCR):
    """loss_refiner_CO_disentangled_reference_point restated from include/happypose_amd.h in plain torch."""
    gt = gt_all[:, 0]
    xr, yr = out[:, :3], out[:, 3:6]
    x = xr / xr.norm(dim=-1, keepdim=True)
    z = torch.cross(x, yr, dim=-1)
    z = z / z.norm(dim=-1, keepdim=True)
    dR = torch.stack((x, torch.cross(z, x, dim=-1), z), -1)
    fxy = torch.stack((K[:, 0, 0], K[:, 1, 1]), 1)
    q = ((gt[:, :3, :3] @ T_in[:, :3, :3].transpose(1, 2)) @ (T_in[:, :3, 3] - tCR).unsqueeze(-1)).squeeze(-1)
    ztgt = (gt[:, 2, 3] - q[:, 2]) / tCR[:, 2] * tCR[:, 2]
    orn, xy, zz = gt.clone(), gt.clone(), gt.clone()
    orn[:, :3, :3] = dR @ T_in[:, :3, :3]
    xy[:, :2, 3] = q[:, :2] + (out[:, 6:8] / fxy + tCR[:, :2] / tCR[:, 2:3]) * ztgt[:, None]
    zz[:, 2, 3] = q[:, 2] + out[:, 8] * tCR[:, 2]
    return torch_symmetric(gt_all, orn, pts) + torch_symmetric(gt_all, xy, pts) + torch_symmetric(gt_all, zz, pts)


def measure(fn, repeat):
    """Median milliseconds of ``fn`` (ending in a synchronise) after one warm-up, and the peak memory it allocated on top of what
    was live before."""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3, int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--symmetries", type=int, default=64)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=10)
    args = ap.parse_args()
    b, s, n, dev = args.rows, args.symmetries, args.points, "cuda"
    g = torch.Generator().manual_seed(0)
    ang = 2 * np.pi * torch.arange(s) / s
    sym = torch.eye(4).repeat(s, 1, 1)
    sym[:, 0, 0], sym[:, 0, 1], sym[:, 1, 0], sym[:, 1, 1] = ang.cos(), -ang.sin(), ang.sin(), ang.cos()
    T_gt = torch.eye(4).repeat(b, 1, 1)
    T_gt[:, :3, 3] = torch.rand(b, 3, generator=g) * torch.tensor([0.3, 0.3, 0.7]) + torch.tensor([-0.15, -0.15, 0.5])
    gt = (T_gt[:, None] @ sym[None]).to(dev)
    T_in = T_gt.clone()
    T_in[:, :3, 3] += (torch.rand(b, 3, generator=g) - 0.5) * 0.06
    T_in = T_in.to(dev)
    out0 = torch.cat([torch.randn(b, 6, generator=g), 3 * torch.randn(b, 2, generator=g), 1 + 0.05 * torch.randn(b, 1, generator=g)], 1).to(dev)
    K = torch.tensor([[600.0, 0, 120], [0, 600.0, 90], [0, 0, 1]]).repeat(b, 1, 1).to(dev)
    pts = ((torch.rand(b, n, 3, generator=g) - 0.5) * 0.1).to(dev)
    tCR = T_in[:, :3, 3].clone()
    up = torch.ones(b, device=dev)
    grads = {}

    def step(name, fn):
        o = out0.clone().requires_grad_(True)
        fn(o).backward(up)
        grads[name] = o.grad

    hip = lambda: step("hip", lambda o: losses.loss_refiner_CO_disentangled_reference_point(gt, T_in, o, K, pts, tCR)[0])  # noqa: E731
    plain = lambda: step("torch", lambda o: torch_refiner_loss(gt, T_in, o, K, pts, tCR))  # noqa: E731
    hip_ms, hip_bytes = measure(hip, args.repeat)
    torch_ms, torch_bytes = measure(plain, max(1, args.repeat // 2))
    print(json.dumps({"rows": b, "symmetries": s, "points": n, "hip_fwd_bwd_ms": round(hip_ms, 3), "torch_fwd_bwd_ms": round(torch_ms, 3),
                      "hip_peak_bytes": hip_bytes, "torch_peak_bytes": torch_bytes,
                      "max_abs_grad_diff": float((grads["hip"] - grads["torch"]).abs().max())}), flush=True)


if __name__ == "__main__":
    main()
