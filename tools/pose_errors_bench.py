#!/usr/bin/env python3
"""Time ADD-S on the device: 64 rows at 2 000 and 20 000 points, ``ops.pose_errors`` (one launch) beside a plain-torch restatement
of the same definition (pairwise differences, argmin, gather) cut into chunks of ground-truth points that fit in memory.

A tool, not a test: it prints what it measures and attaches no threshold.  Usage:  python tools/pose_errors_bench.py [--rows 64]
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


def torch_add_s(T_pred, T_gt, pts, chunk_bytes=1 << 30):
    """norm_avg [b] of ADD-S in plain torch; the [b, chunk, P, 3] temporary stays below ``chunk_bytes``."""
    b, n = pts.shape[0], pts.shape[1]
    pred = pts @ T_pred[:, :3, :3].transpose(1, 2) + T_pred[:, None, :3, 3]
    gt = pts @ T_gt[:, :3, :3].transpose(1, 2) + T_gt[:, None, :3, 3]
    chunk = max(1, chunk_bytes // (b * n * 12))
    total = torch.zeros(b, device=pts.device)
    for j0 in range(0, n, chunk):
        d = gt[:, j0:j0 + chunk, None] - pred[:, None]
        assign = (d * d).sum(-1).argmin(2)
        picked = torch.gather(d, 2, assign[..., None, None].expand(-1, -1, 1, 3)).squeeze(2)
        total += torch.norm(picked, dim=-1).sum(-1)
    return total / n


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
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda"
    rs = np.random.RandomState(0)
    for n in (2000, 20000):
        pts = torch.as_tensor(rs.uniform(-0.08, 0.08, (1, n, 3)), dtype=torch.float32, device=dev)
        T_gt = torch.eye(4, device=dev).repeat(args.rows, 1, 1)
        T_gt[:, :3, 3] = torch.as_tensor(rs.uniform([-0.1, -0.1, 0.5], [0.1, 0.1, 1.2], (args.rows, 3)), dtype=torch.float32, device=dev)
        T_pred = T_gt.clone()
        T_pred[:, :3, 3] += torch.as_tensor(rs.normal(scale=0.006, size=(args.rows, 3)), dtype=torch.float32, device=dev)
        ids = torch.arange(args.rows, dtype=torch.int32, device=dev)
        zeros, mode = torch.zeros_like(ids), torch.full_like(ids, ops.POSE_ERR_MODES["ADD-S"])
        sym = torch.eye(4, device=dev)[None, None]
        one, cnt = torch.ones(1, dtype=torch.int32, device=dev), torch.full((1,), n, dtype=torch.int32, device=dev)
        kernel = lambda: ops.pose_errors_tables(ids, ids, zeros, mode, T_pred, T_gt, pts, sym, one, cnt)["norm_avg"]  # noqa: E731
        plain = lambda: torch_add_s(T_pred, T_gt, pts.expand(args.rows, -1, -1))  # noqa: E731
        diff = float((kernel() - plain()).abs().max())
        print(json.dumps({"rows": args.rows, "points": n, "hip_ms": round(timed(kernel, args.repeat), 3),
                          "torch_chunked_ms": round(timed(plain, max(1, args.repeat // 2)), 3), "max_abs_diff_m": diff,
                          "workspace_bytes": ops.pose_errors_workspace_bytes(args.rows, n)}), flush=True)


if __name__ == "__main__":
    main()
