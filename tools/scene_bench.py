#!/usr/bin/env python3
"""Time the scene merge on the device: ``ops.scene_compose`` and ``ops.scene_visibility`` for 8 and 32 layers at 480 x 640 beside a
plain-torch restatement on the same device (stack the layers, ``where(depth > 0, depth, inf)``, ``argmin``, ``gather``; counts by
comparison and ``sum``).  The layers are synthetic discs with random depths: the kernels do not care what drew them.

A tool, not a test: it prints what it measures and attaches no threshold.  Usage:  python tools/scene_bench.py [--repeat 20]
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

from happypose_amd import ops  # noqa: E402


def torch_compose(rgb, nrm, depth):
    key = torch.where(depth > 0, depth, torch.full_like(depth, float("inf")))[:, 0]
    best, win = key.min(0)
    cov = best < float("inf")
    idx = win[None, None].expand(1, 3, -1, -1)
    pick = lambda x: torch.where(cov[None], torch.gather(x, 0, idx)[0], torch.zeros_like(x[0]))  # noqa: E731
    return {"rgb": pick(rgb)[None], "normals": pick(nrm)[None], "depth": torch.where(cov, best, torch.zeros_like(best))[None, None],
            "ids": torch.where(cov, win, torch.full_like(win, -1)).to(torch.int32)[None], "mask": cov.to(torch.uint8)[None, None]}


def torch_visibility(depth, ids):
    n = depth.shape[0]
    vis = ids[0][None] == torch.arange(n, device=depth.device, dtype=torch.int32)[:, None, None]
    return torch.stack([(depth[:, 0] > 0).sum((1, 2)), vis.sum((1, 2))], 1).to(torch.int32)  # the two counts (no boxes)


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    args = ap.parse_args()
    dev, (h, w) = "cuda", (480, 640)
    rs = np.random.RandomState(0)
    yy, xx = np.mgrid[:h, :w]
    for n in (8, 32):
        depth = np.zeros((n, 1, h, w), np.float32)
        for l in range(n):
            cx, cy, r = rs.uniform(100, w - 100), rs.uniform(100, h - 100), rs.uniform(60, 160)
            disc = (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
            depth[l, 0][disc] = rs.uniform(0.4, 1.2) + 1e-4 * (xx + yy)[disc]
        depth = torch.as_tensor(depth, device=dev)
        rgb = torch.rand((n, 3, h, w), device=dev) * (depth > 0)
        nrm = torch.rand((n, 3, h, w), device=dev) * (depth > 0)
        off = torch.as_tensor([0, n], dtype=torch.int32, device=dev)
        got, want = ops.scene_compose(off, rgb, nrm, depth), torch_compose(rgb, nrm, depth)
        same = all(torch.equal(got[k], want[k]) for k in want)
        table = ops.scene_visibility(off, depth, got["ids"])
        same = same and torch.equal(table[:, :2], torch_visibility(depth, got["ids"]))
        print(json.dumps({"layers": n, "resolution": [h, w], "equal_to_torch": bool(same),
                          "compose_hip_ms": round(timed(lambda: ops.scene_compose(off, rgb, nrm, depth), args.repeat), 4),
                          "compose_torch_ms": round(timed(lambda: torch_compose(rgb, nrm, depth), args.repeat), 4),
                          "visibility_hip_ms": round(timed(lambda: ops.scene_visibility(off, depth, got["ids"]), args.repeat), 4),
                          "visibility_torch_counts_ms": round(timed(lambda: torch_visibility(depth, got["ids"]), args.repeat), 4)}), flush=True)


if __name__ == "__main__":
    main()
