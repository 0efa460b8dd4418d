#!/usr/bin/env python3
"""Time the detection / segmentation scoring of one evaluation batch: ``--frames`` frames x ``--preds`` predictions x ``--gts``
ground truths of one label at 480 x 640.  Three steps on the device -- ``ops.mask_pack`` (predictions and ground truths),
``ops.det_iou`` on the packed masks (every pair of a frame, one launch) and ``ops.det_match`` at COCO's ten thresholds -- against
the same three results written with plain torch ops on the same device: the mask IoU as ``(m1[:, None] & m2[None]).sum((-1, -2))``
over ``--chunk`` predictions at a time (a ``[chunk, G, H, W]`` temporary), the matching as the literal greedy loop vectorised over
frames and thresholds.  Packing is also timed from a buffer that starts at an odd byte, which takes the byte-load (ballot) kernel
instead of the 8-byte-load (fold) kernel.  Information, not a threshold.

Usage:  python tools/det_eval_bench.py [--frames 8] [--preds 100] [--gts 15] [--iters 10]
Prints one JSON line: milliseconds per call (median of 5 windows of ``--iters`` calls each, ``torch.cuda.Event`` pairs around the
window, after a warm-up window), the bytes per pair packed against unpacked, and whether both sides gave the same integers.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from happypose_amd import evaluation as E, ops  # noqa: E402

WINDOWS = 5


def timed(fn, iters):
    """Milliseconds per call: the median of ``WINDOWS`` event-timed windows of ``iters`` calls, after one warm-up window."""
    for _ in range(iters):
        res = fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            res = fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / iters)
    return float(np.median(out)), res


def make_masks(rs, n, h, w):
    """Ellipses of 40 - 160 pixels across, as instance masks are."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.zeros((n, h, w), bool)
    for k in range(n):
        cx, cy, rx, ry = rs.uniform(60, w - 60), rs.uniform(60, h - 60), rs.uniform(20, 80), rs.uniform(20, 80)
        out[k] = ((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2 <= 1
    return out


def torch_mask_iou(pred, gt, frames, n_pred, n_gt, chunk):
    """``[frames * n_pred * n_gt]`` inter, union and IoU with plain torch ops, ``chunk`` predictions at a time."""
    inter = []
    for f in range(frames):
        g = gt[f * n_gt:(f + 1) * n_gt]
        for p0 in range(0, n_pred, chunk):
            p = pred[f * n_pred + p0:f * n_pred + min(p0 + chunk, n_pred)]
            inter.append((p[:, None] & g[None]).sum((-1, -2)).reshape(-1))
    inter = torch.cat(inter)
    area_p, area_g = pred.sum((-1, -2)), gt.sum((-1, -2))
    union = (area_p.reshape(frames, n_pred, 1) + area_g.reshape(frames, 1, n_gt)).reshape(-1) - inter
    return inter, union, torch.where(union > 0, inter.float() / union.clamp(min=1).float(), torch.zeros_like(inter, dtype=torch.float32))


def torch_match(iou, frames, n_pred, n_gt, thr):
    """COCO's greedy matching without ignored ground truths, all frames and thresholds at once: one step per detection."""
    iou = iou.reshape(frames, 1, n_pred, n_gt)
    thr = thr.reshape(1, -1, 1)
    free = torch.ones((frames, thr.shape[1], n_gt), dtype=torch.bool, device=iou.device)
    pos = torch.arange(n_gt, device=iou.device)
    det_match = []
    for d in range(n_pred):
        v = iou[:, :, d]
        ok = free & (v >= thr)
        best = torch.where(ok, v, v.new_tensor(-1.0)).amax(-1, keepdim=True)
        m = torch.where(ok & (v == best), pos, pos.new_tensor(-1)).amax(-1)  # the highest position among the equal best
        det_match.append(m)
        free = free & (pos != m[..., None])
    return torch.stack(det_match, -1)  # [frames, n_thr, n_pred]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--preds", type=int, default=100)
    ap.add_argument("--gts", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=10, help="predictions per [chunk, G, H, W] temporary of the torch restatement")
    ap.add_argument("--resolution", default="480x640")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "det_eval_bench measures on the GPU only"
    dev = torch.device("cuda")
    h, w = (int(x) for x in args.resolution.split("x"))
    F, D, G = args.frames, args.preds, args.gts
    rs = np.random.RandomState(0)
    gt_np = make_masks(rs, F * G, h, w)
    pred_np = make_masks(rs, F * D, h, w)
    for f in range(F):  # the first predictions of a frame are its ground truths, the rest are clutter
        pred_np[f * D:f * D + min(D, G)] = np.roll(gt_np[f * G:f * G + min(D, G)], 3, axis=2)
    pred, gt = torch.as_tensor(pred_np, device=dev), torch.as_tensor(gt_np, device=dev)
    odd = torch.zeros(pred.numel() + 1, dtype=torch.bool, device=dev)
    odd[1:] = pred.reshape(-1)
    pred_odd = odd[1:].view(F * D, h, w)
    pred_idx = (np.arange(F)[:, None, None] * D + np.arange(D)[None, :, None] + np.zeros((1, 1, G), int)).reshape(-1)
    gt_idx = (np.arange(F)[:, None, None] * G + np.zeros((1, D, 1), int) + np.arange(G)[None, None, :]).reshape(-1)
    pred_idx, gt_idx = torch.as_tensor(pred_idx, dtype=torch.int32, device=dev), torch.as_tensor(gt_idx, dtype=torch.int32, device=dev)
    thr = E.COCO_IOU_THRESHOLDS
    thr_d = torch.as_tensor(ops.coco_thresholds(thr), device=dev)
    n_det, n_gt, ignore = np.full(F, D), np.full(F, G), np.zeros(F * G, bool)

    line = {"resolution": f"{h}x{w}", "frames": F, "preds_per_frame": D, "gts_per_frame": G, "pairs": F * D * G, "iters": args.iters, "windows": WINDOWS}
    line["pack_ms"], (pp, pg) = timed(lambda: (ops.mask_pack(pred), ops.mask_pack(gt)), args.iters)
    line["pack_pred_fold_ms"], _ = timed(lambda: ops.mask_pack(pred), args.iters)
    line["pack_pred_ballot_ms"], pp_odd = timed(lambda: ops.mask_pack(pred_odd), args.iters)
    line["det_iou_ms"], out = timed(lambda: ops.det_iou(pred_idx, gt_idx, packed_pred=pp, packed_gt=pg), args.iters)
    line["det_match_ms"], tables = timed(lambda: ops.det_match(out["mask_iou"], n_det, n_gt, ignore, thr), args.iters)
    line["packed_total_ms"] = line["pack_ms"] + line["det_iou_ms"] + line["det_match_ms"]
    torch_iters = line["torch_iters"] = max(1, args.iters // 5)  # the restatement is slow: shorter windows
    line["torch_iou_ms"], (t_inter, t_union, t_iou) = timed(lambda: torch_mask_iou(pred, gt, F, D, G, args.chunk), torch_iters)
    line["torch_match_ms"], t_match = timed(lambda: torch_match(t_iou, F, D, G, thr_d), torch_iters)
    line["torch_total_ms"] = line["torch_iou_ms"] + line["torch_match_ms"]
    line["speedup_vs_torch"] = line["torch_total_ms"] / line["packed_total_ms"]
    w64 = ops.mask_pack_words(h, w)
    line["bytes_per_pair_packed"] = 2 * 8 * w64
    line["bytes_per_pair_unpacked"] = 2 * h * w
    line["det_iou_read_TBps"] = line["bytes_per_pair_packed"] * F * D * G / (line["det_iou_ms"] * 1e-3) / 1e12  # mostly L2 hits: pairs share masks
    line["same_packing_fold_and_ballot"] = bool(torch.equal(pp[0], pp_odd[0]) and torch.equal(pp[1], pp_odd[1]))
    line["same_counts_as_torch"] = bool(torch.equal(out["inter"].long(), t_inter) and torch.equal(out["union"].long(), t_union))
    line["same_iou_bits_as_torch"] = bool(torch.equal(out["mask_iou"].view(torch.int32), t_iou.view(torch.int32)))
    line["same_matches_as_torch"] = bool(torch.equal(tables["det_match"].reshape(len(thr), F, D).permute(1, 0, 2).long(), t_match))
    line["matched_at_0.5"] = int((tables["det_match"][0] >= 0).sum())
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in line.items()}), flush=True)


if __name__ == "__main__":
    main()
