"""Time one loss layer of ``h_maskrcnn`` against a plain-torch restatement of the same formulas on the same device.

480 x 640, B = 8: 76 740 anchors per image, 8 ground truths per image, 512 RoIs per image (128 of them positive, 21 classes).
Both sides do: anchor matching (0.7 / 0.3, low-quality matches), anchor targets, the RPN losses on 256 sampled anchors per image,
the Fast R-CNN losses on the RoIs, the mask targets and the mask loss, each loss with its gradient at the network outputs.  The
sampled rows are drawn once and shared, so the comparison is of arithmetic, not of samplers.  5 warm-up calls, the median of 30,
a device synchronise around each.  Prints one JSON line.

    python tools/det_losses_bench.py
"""

import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, A, G, R, POS, C, M, H, W = 8, 76740, 8, 512, 128, 21, 28, 480, 640
BETA = 1.0 / 9.0


def make(dev):
    rng = np.random.default_rng(0)
    c = rng.uniform((0, 0), (W, H), (B * A, 2))
    s = rng.uniform(16, 400, (B * A, 2))
    anchors = torch.tensor(np.concatenate([c - s / 2, c + s / 2], 1), dtype=torch.float32, device=dev)
    c = rng.uniform((100, 100), (W - 100, H - 100), (B * G, 2))
    s = rng.uniform(40, 200, (B * G, 2))
    gt = torch.tensor(np.concatenate([c - s / 2, c + s / 2], 1), dtype=torch.float32, device=dev)
    masks = torch.zeros((B * G, H, W), dtype=torch.uint8, device=dev)
    for i, (x1, y1, x2, y2) in enumerate(gt.round().long().tolist()):
        masks[i, max(y1, 0):y2, max(x1, 0):x2] = 1
    t = lambda *shape: torch.tensor(rng.standard_normal(shape), dtype=torch.float32, device=dev)  # noqa: E731
    labels = torch.tensor(rng.integers(1, C, B * R) * (np.arange(B * R) % R < POS), dtype=torch.int64, device=dev)
    pos = torch.where(labels > 0)[0]
    image_of_pos = (pos // R).to(torch.int32)
    mask_match = (image_of_pos * G + torch.tensor(rng.integers(0, G, pos.numel()), device=dev)).to(torch.int32)
    jitter = torch.tensor(rng.uniform(-8, 8, (pos.numel(), 4)), dtype=torch.float32, device=dev)
    return dict(anchors=anchors, image_of=torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(A), gt=gt,
                gt_off=[G * b for b in range(B + 1)], objectness=t(B * A), deltas=t(B * A, 4) * 0.3, logits=t(B * R, C),
                reg=t(B * R, 4 * C) * 0.3, labels=labels, targets=t(B * R, 4) * 0.3, mask_logits=t(pos.numel(), C, M, M), masks=masks,
                mask_match=mask_match, mask_rois=gt[mask_match.long()] + jitter, mask_labels=labels[pos])


def ours(d, sampled):
    from happypose_amd import ops

    match, _ = ops.det_assign(d["anchors"], d["image_of"], d["gt"], d["gt_off"], 0.7, 0.3, True)
    enc = torch.where(match >= 0, match, d["image_of"] * G)
    rpn_targets = ops.det_box_encode(d["anchors"], enc, d["gt"], (1, 1, 1, 1))
    rpn_labels = torch.where(match >= 0, 1, torch.where(match == -1, 0, -1)).to(torch.int32)
    l1 = ops.loss_rpn(d["objectness"], d["deltas"], rpn_labels, rpn_targets, sampled)
    l2 = ops.loss_fastrcnn(d["logits"], d["reg"], d["labels"], d["targets"], C)
    mt = ops.det_mask_targets(d["masks"], d["mask_match"], d["mask_rois"], M)
    l3 = ops.loss_mask(d["mask_logits"], d["mask_labels"], mt)
    return l1[0], l2[0], l3[0]


def _iou(g, b):
    a1, a2 = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(g[:, None, 2:], b[None, :, 2:]) - torch.max(g[:, None, :2], b[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (a1[:, None] + a2[None] - inter)


def _encode(g, p):
    ew, eh, gw, gh = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1], g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    return torch.stack([((g[:, 0] + 0.5 * gw) - (p[:, 0] + 0.5 * ew)) / ew, ((g[:, 1] + 0.5 * gh) - (p[:, 1] + 0.5 * eh)) / eh,
                        torch.log(gw / ew), torch.log(gh / eh)], 1)


def _roi_align_fixed(masks, rois, ratio=2):
    """Plain torch has no adaptive roi_align: a fixed grid of ``ratio`` x ``ratio`` samples per bin through ``grid_sample``-free
    gathers (fewer samples than the adaptive ratio takes on large rois, so this side is favoured)."""
    n = rois.shape[0]
    steps = (torch.arange(M * ratio, device=rois.device) + 0.5) / (M * ratio)
    w, h = (rois[:, 2] - rois[:, 0]).clamp(min=1), (rois[:, 3] - rois[:, 1]).clamp(min=1)
    xs, ys = rois[:, 0:1] + steps[None] * w[:, None], rois[:, 1:2] + steps[None] * h[:, None]

    def taps(v, size):
        ok = (v >= -1) & (v <= size)
        v = v.clamp(min=0)
        lo = v.floor().clamp(max=size - 1)
        hi = (lo + 1).clamp(max=size - 1)
        frac = torch.where(lo >= size - 1, torch.zeros_like(v), v - lo)
        return lo.long(), hi.long(), frac, ok

    x0, x1, fx, okx = taps(xs, W)
    y0, y1, fy, oky = taps(ys, H)
    m = masks.float()
    i = torch.arange(n, device=rois.device)[:, None, None]
    val = ((1 - fy)[:, :, None] * (1 - fx)[:, None] * m[i, y0[:, :, None], x0[:, None]] + (1 - fy)[:, :, None] * fx[:, None] * m[i, y0[:, :, None], x1[:, None]]
           + fy[:, :, None] * (1 - fx)[:, None] * m[i, y1[:, :, None], x0[:, None]] + fy[:, :, None] * fx[:, None] * m[i, y1[:, :, None], x1[:, None]])
    val = val * (oky[:, :, None] & okx[:, None])
    return val.reshape(n, M, ratio, M, ratio).mean((2, 4))


def plain_torch(d, sampled):
    match = torch.empty(B * A, dtype=torch.int64, device=d["anchors"].device)
    for b in range(B):  # torchvision's per-image loop
        q = _iou(d["gt"][G * b:G * (b + 1)], d["anchors"][A * b:A * (b + 1)])
        vals, m = q.max(0)
        allm = m.clone()
        m[vals < 0.3] = -1
        m[(vals >= 0.3) & (vals < 0.7)] = -2
        restore = torch.where(q == q.max(1).values[:, None])[1]
        m[restore] = allm[restore]
        match[A * b:A * (b + 1)] = torch.where(m >= 0, m + G * b, m)
    rpn_targets = _encode(d["gt"][torch.where(match >= 0, match, d["image_of"].long() * G)], d["anchors"])
    lab = (match >= 0).float()
    obj, dlt = d["objectness"].detach().requires_grad_(), d["deltas"].detach().requires_grad_()
    s = sampled.long()
    sp = s[lab[s] > 0]
    l_obj = F.binary_cross_entropy_with_logits(obj[s], lab[s])
    l_rbox = F.smooth_l1_loss(dlt[sp], rpn_targets[sp], beta=BETA, reduction="sum") / s.numel()
    x, r = d["logits"].detach().requires_grad_(), d["reg"].detach().requires_grad_()
    l_cls = F.cross_entropy(x, d["labels"])
    pos = torch.where(d["labels"] > 0)[0]
    l_box = F.smooth_l1_loss(r.reshape(-1, C, 4)[pos, d["labels"][pos]], d["targets"][pos], beta=BETA, reduction="sum") / d["labels"].numel()
    ml = d["mask_logits"].detach().requires_grad_()
    mt = _roi_align_fixed(d["masks"][d["mask_match"].long()], d["mask_rois"])
    l_mask = F.binary_cross_entropy_with_logits(ml[torch.arange(ml.shape[0]), d["mask_labels"]], mt)
    (l_obj + l_rbox + l_cls + l_box + l_mask).backward()
    return torch.stack([l_obj, l_rbox]), torch.stack([l_cls, l_box]), l_mask.reshape(1)


def median_ms(fn, *args):
    for _ in range(5):
        fn(*args)
    times = []
    for _ in range(30):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(*args)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    from happypose_amd import ops

    dev = torch.device("cuda:0")
    d = make(dev)
    match, _ = ops.det_assign(d["anchors"], d["image_of"], d["gt"], d["gt_off"], 0.7, 0.3, True)
    labels = torch.where(match >= 0, 1, torch.where(match == -1, 0, -1))
    picked = ops.det_sample(labels, d["image_of"], B, 256, 0.5, seed=1, stream=1)
    sampled = torch.cat([p for p, _ in picked] + [n for _, n in picked]).to(torch.int32)
    a, b = ours(d, sampled), plain_torch(d, sampled)
    out = dict(tool="det_losses_bench", device=torch.cuda.get_device_name(0), B=B, anchors_per_image=A, gt_per_image=G, rois_per_image=R,
               sampled_anchors=int(sampled.numel()), losses_hip=[float(v) for t in a for v in t], losses_torch=[float(v) for t in b for v in t.detach()],
               hip_ms=round(median_ms(ours, d, sampled), 3), torch_ms=round(median_ms(plain_torch, d, sampled), 3))
    out["speedup"] = round(out["torch_ms"] / out["hip_ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
