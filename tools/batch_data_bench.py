"""Times the three launches of the data sets' batch assembly (csrc/batch_data.hip) against a plain-torch restatement on the same
device tensors: B = 32 frames of 480 x 640 with 12 objects each.

    python tools/batch_data_bench.py [--batch 32] [--height 480] [--width 640] [--ids 12] [--calls 50] [--rounds 7] [--warmup 3]

Method: every shape is warmed up, the outputs of both sides are compared once (bit for bit, TCO to 1e-5), then each side runs
`--calls` calls between two device events, `--rounds` times, the two sides alternating inside a round; the figure is the median
over the rounds of the time per call, with the minimum and maximum.  The time is the call as a user makes it (argument checks,
output allocation through torch's caching allocator, launch), not the kernel alone; kernel-level times need a profiler run of
their own.  `bytes` is what the algorithm has to move, computed from the shapes, and `GB_per_s` that over the call time.  The
baseline is the torch restatement, not the reference (which does this work with NumPy on the host, one image at a time).  Prints
one JSON line.  Needs a GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from happypose_amd import ops  # noqa: E402


def event_ms(fn, calls: int) -> float:
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def compare(ours, base, warmup: int, calls: int, rounds: int) -> dict:
    for _ in range(warmup):
        ours(), base()
    torch.cuda.synchronize()
    t = {"hip": [], "torch": []}
    for _ in range(rounds):
        t["hip"].append(event_ms(ours, calls))
        t["torch"].append(event_ms(base, calls))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in t.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--ids", type=int, default=12)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "batch_data_bench needs a GPU"
    B, h, w, n = a.batch, a.height, a.width, a.ids
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    # blocks of 40 x 40 pixels with ids 0 .. n: objects of a plausible size rather than noise; every fourth frame is empty
    seg = np.kron(rng.integers(0, n + 1, (B, (h + 39) // 40, (w + 39) // 40)), np.ones((40, 40), np.int64))[:, :h, :w].astype(np.int32)
    seg[3::4] = 0
    rgb = torch.as_tensor(rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)).to(dev)
    depth = torch.as_tensor(rng.uniform(0.3, 2.0, (B, h, w)).astype(np.float32)).to(dev)
    seg = torch.as_tensor(seg).to(dev)
    ids = torch.arange(1, n + 1, dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
    boxes, n_px = ops.seg_boxes(seg, ids)
    q, _ = np.linalg.qr(rng.standard_normal((B * (n + 1), 3, 3)))
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    T = np.tile(np.eye(4, dtype=np.float32), (B * (n + 1), 1, 1))
    T[:, :3, :3], T[:, :3, 3] = q, rng.uniform(-1, 1, (B * (n + 1), 3))
    TWC, TWO = torch.as_tensor(T[:B]).to(dev), torch.as_tensor(T[B:].reshape(B, n, 4, 4)).to(dev)
    min_area = 100.0
    result = {"batch": B, "height": h, "width": w, "ids": n, "calls": a.calls, "rounds": a.rounds, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0)}

    # ---- select (return_first_object: the one choice plain torch can restate without this library's random stream) ----
    def select_hip():
        return ops.pose_batch_select(n_px, boxes, TWC, TWO, min_area=min_area, first=True)

    def select_torch():
        b = boxes.long()
        ok = (n_px > 0) & (((b[..., 3] - b[..., 1]) * (b[..., 2] - b[..., 0])).double() >= min_area)
        valid = ok.any(1)
        chosen = torch.where(valid, ok.int().argmax(1), -1)
        at = chosen.clamp(min=0)
        rows = torch.arange(B, device=dev)
        Ti = torch.zeros_like(TWC)
        Ti[:, :3, :3] = TWC[:, :3, :3].transpose(1, 2)
        Ti[:, :3, 3] = -(TWC[:, :3, :3].transpose(1, 2) @ TWC[:, :3, 3:]).squeeze(2)
        Ti[:, 3, 3] = 1
        TCO = (Ti[:, :, :, None] * TWO[rows, at][:, None]).sum(2) * valid[:, None, None]
        bbox = boxes[rows, at].float() * valid[:, None]
        dst = (torch.cumsum(valid.int(), 0) - valid.int()).int()
        return chosen.int(), valid, bbox, TCO, dst, valid.sum().int().reshape(1)

    g, t = select_hip(), select_torch()
    assert all(torch.equal(x, y) for x, y in zip(g[:3] + g[4:], t[:3] + t[4:])) and (g[3] - t[3]).abs().max() < 1e-5
    chosen, valid, _, _, dst, n_valid = g
    n_rows = int(n_valid.item())
    result["select"] = compare(select_hip, select_torch, a.warmup, a.calls, a.rounds)

    # ---- gather ----
    def gather_hip():
        return ops.batch_gather_chw(rgb, valid, dst, n_rows, depth=depth)

    def gather_torch():
        return rgb[valid].permute(0, 3, 1, 2).contiguous(), depth[valid]

    assert all(torch.equal(x, y) for x, y in zip(gather_hip(), gather_torch()))
    result["gather"] = compare(gather_hip, gather_torch, a.warmup, a.calls, a.rounds)
    result["gather"]["bytes"] = 2 * n_rows * h * w * (3 + 4)

    # ---- masks: the slots with pixels and area > 50, as DetectionDataset keeps them (the layout is the host's, outside the timing) ----
    tb = torch.cat([boxes, n_px[..., None]], 2).cpu().numpy().astype(np.int64)
    keep = (tb[..., 4] > 0) & ((tb[..., 3] - tb[..., 1]) * (tb[..., 2] - tb[..., 0]) > 50)
    slot_row = np.where(keep, np.cumsum(keep.reshape(-1)).reshape(keep.shape) - 1, -1).astype(np.int32)
    G = int(keep.sum())
    slot_row_d, keep_d = torch.as_tensor(slot_row).to(dev), torch.as_tensor(keep).to(dev)

    def masks_hip():
        return ops.instance_masks(seg, ids, slot_row_d, G)

    def masks_torch():
        return torch.cat([(seg[b][None] == ids[b][keep_d[b]][:, None, None]) for b in range(B)]).to(torch.uint8)

    assert torch.equal(masks_hip(), masks_torch())
    result["masks"] = compare(masks_hip, masks_torch, a.warmup, max(a.calls // 5, 1), a.rounds)
    result["masks"]["bytes"] = G * h * w + int(keep.any(1).sum()) * h * w * 4
    result["masks"]["G"] = G
    for part in ("gather", "masks"):
        for side in ("hip", "torch"):
            result[part][side]["GB_per_s"] = result[part]["bytes"] / result[part][side]["median_ms"] / 1e6
    for part in ("select", "gather", "masks"):
        result[part]["torch_over_hip"] = result[part]["torch"]["median_ms"] / result[part]["hip"]["median_ms"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
