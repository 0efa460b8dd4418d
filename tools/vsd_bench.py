#!/usr/bin/env python3
"""Time BOP's visible-surface discrepancy at 640 x 480 with BOP's 10 taus: ``evaluation.vsd`` end to end (depth-only renders of
the distinct poses + one ``hp_vsd`` launch), the bare ``hp_vsd`` launch on those renders, and the same four steps of the
definition (include/happypose_amd.h) written with plain torch ops on the device on the SAME depth maps.  The scene is seeded:
``--gts`` ground truths of synthetic objects in one frame, ``--per-gt`` estimates each, shifted by about a centimetre; the measured depth is the
ground-truth composite.  Information, not a threshold.

Usage:  python tools/vsd_bench.py [--gts 8] [--per-gt 8] [--repeats 20]
Prints one JSON line: milliseconds per call (median and minimum of the repeats after a warm-up call, host clock around a device
synchronise), the kernel's algorithmic bytes (three float32 reads per pixel per row) over the bare launch's time as a rate and as
a fraction of the 6.3 TB/s a streaming read achieves on an MI355X, and whether the torch restatement gave the same integers.
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

from happypose_amd import evaluation as E, ops  # noqa: E402
from happypose_amd.synthetic import make_object_dataset, random_rotations  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes / s: a float4 streaming read on an MI355X


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), float(np.min(out)), res


def torch_vsd(est_layer, gt_layer, frame, diameter, depth_test, depth_layers, K, delta, taus, bsz=16):
    """The definition with torch ops, ``bsz`` rows at a time (a [bsz, n_tau, H, W] temporary)."""
    h, w = depth_test.shape[1:]
    dev = depth_test.device
    u = torch.arange(w, device=dev, dtype=torch.float32)[None, None, :]
    v = torch.arange(h, device=dev, dtype=torch.float32)[None, :, None]
    f = torch.sqrt(((u - K[:, 0, 2, None, None]) / K[:, 0, 0, None, None]) ** 2 + ((v - K[:, 1, 2, None, None]) / K[:, 1, 1, None, None]) ** 2 + 1)
    taus = torch.as_tensor(taus, device=dev, dtype=torch.float32)[None, :, None, None]
    counts, cost = [], []
    for i in range(0, len(est_layer), bsz):
        fr = frame[i:i + bsz]
        st, se, sg = depth_test[fr] * f[fr], depth_layers[est_layer[i:i + bsz]] * f[fr], depth_layers[gt_layer[i:i + bsz]] * f[fr]
        free = st == 0
        vg = (sg > 0) & ((sg - st <= delta) | free)
        ve = ((se > 0) & ((se - st <= delta) | free)) | (vg & (se > 0))
        inter = vg & ve
        q = (sg - se).abs() / diameter[i:i + bsz, None, None]
        cost.append((inter[:, None] & (q[:, None] >= taus)).sum((2, 3)))
        counts.append(torch.stack([(vg | ve).sum((1, 2)), inter.sum((1, 2)), ve.sum((1, 2)), vg.sum((1, 2))], 1))
    counts, cost = torch.cat(counts), torch.cat(cost)
    n_u = counts[:, :1].float()
    errors = torch.where(n_u > 0, (cost + counts[:, :1] - counts[:, 1:2]).float() / n_u.clamp(min=1), torch.ones_like(n_u))
    return {"errors": errors, "cost": cost, "counts": counts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gts", type=int, default=8)
    ap.add_argument("--per-gt", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--resolution", default="480x640")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "vsd_bench measures on the GPU only"
    dev = torch.device("cuda")
    h, w = (int(x) for x in args.resolution.split("x"))
    ds = make_object_dataset(4, seed=1, tex_size=64)
    store = ops.MeshStore(ds, dev)
    rs = np.random.RandomState(3)
    n_gt, per = args.gts, args.per_gt
    gt = np.tile(np.eye(4, dtype=np.float32), (n_gt, 1, 1))
    gt[:, :3, :3] = random_rotations(rs, n_gt)
    gt[:, :3, 3] = np.stack([rs.uniform(-0.25, 0.25, n_gt), rs.uniform(-0.18, 0.18, n_gt), rs.uniform(0.5, 0.9, n_gt)], 1)
    gt_labels = np.asarray(store.labels)[np.arange(n_gt) % len(store.labels)]
    gt_of = np.repeat(np.arange(n_gt), per)
    pred = gt[gt_of].copy()
    pred[:, :3, 3] += rs.normal(0, 0.01, (len(pred), 3)).astype(np.float32)
    labels = gt_labels[gt_of]
    K = torch.tensor([[[600.0, 0, w / 2], [0, 600.0, h / 2], [0, 0, 1]]])
    _, _, gt_dep, _ = ops.rasterize(store, store.ids_of(list(gt_labels)), torch.as_tensor(gt), K.expand(n_gt, 3, 3), (h, w), render_depth=True, render_rgb=False)
    far = torch.where(gt_dep > 0, gt_dep, torch.full_like(gt_dep, 1e9)).amin(0)
    depth = torch.where(far < 1e8, far, torch.full_like(far, 1.2))  # the composite in front of a wall at 1.2 m
    pred_t, gt_t = torch.as_tensor(pred), torch.as_tensor(gt[gt_of])
    taus = E.BOP_VSD_TAUS
    n = len(labels)

    line = {"resolution": f"{h}x{w}", "rows": n, "ground_truths": n_gt, "n_tau": len(taus), "repeats": args.repeats}
    line["vsd_total_ms"], line["vsd_total_min_ms"], (errors, det) = timed(
        lambda: E.vsd(pred_t, gt_t, labels, depth, K, store, layer_budget_bytes=1 << 40, return_details=True), args.repeats)
    line["layers"] = int(det["depth_layers"].shape[0])
    cols = [torch.as_tensor(det[k], device=dev) for k in ("est_layer", "gt_layer", "frame")]
    diameter = torch.as_tensor([store.mesh_db.infos[label]["diameter_m"] for label in labels], dtype=torch.float32, device=dev)
    Kd = K.to(dev)
    i32 = [c.to(torch.int32) for c in cols]
    line["hp_vsd_ms"], line["hp_vsd_min_ms"], out = timed(
        lambda: ops.vsd_tables(*i32, diameter, depth, det["depth_layers"], Kd, E.BOP_VSD_DELTA, taus), args.repeats)
    line["torch_ms"], line["torch_min_ms"], ref = timed(
        lambda: torch_vsd(*cols, diameter, depth, det["depth_layers"], Kd, E.BOP_VSD_DELTA, taus), args.repeats)
    algorithmic_bytes = 3 * 4 * h * w * n
    line["algorithmic_bytes"] = algorithmic_bytes
    line["hp_vsd_algorithmic_TBps"] = algorithmic_bytes / (line["hp_vsd_ms"] * 1e-3) / 1e12
    line["hp_vsd_fraction_of_hbm"] = algorithmic_bytes / (line["hp_vsd_ms"] * 1e-3) / HBM_ACHIEVABLE
    line["distinct_bytes"] = 4 * h * w * (line["layers"] + 1)  # what the call reads when every shared image is fetched once
    line["speedup_vs_torch"] = line["torch_ms"] / line["hp_vsd_ms"]
    line["same_counts_as_torch"] = bool(torch.equal(out["counts"].long(), ref["counts"]) and torch.equal(out["cost"].long(), ref["cost"]))
    line["mean_error"] = float(errors.mean())
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in line.items()}), flush=True)


if __name__ == "__main__":
    main()
