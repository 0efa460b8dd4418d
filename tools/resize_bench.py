"""Times CropResizeToAspectTransform on the device: B = 32 frames of 1080 x 1920 to 480 x 640 -- the aspect crop (this size is too
wide for 4 : 3, so the reference's crop pads it to 1440 rows), RGB bilinear, segmentation and depth nearest, K, and the modal boxes
of 16 ids per image -- and its parts on their own.

    python tools/resize_bench.py [--batch 32] [--height 1080] [--width 1920] [--out-height 480] [--out-width 640] [--ids 16]
                                 [--repeats 30] [--warmup 5]

Method, as tools/augment_bench.py: after the warm-up calls each timed call is bracketed by a device synchronise and timed with the
host clock; median, minimum and maximum of the repeats, in one process.  The time includes the host's coefficient tables (cached
after the first call), their upload and the allocation of outputs and the intermediate through torch's caching allocator.  Beside
it the same work runs through Pillow and NumPy on the host, one image at a time, as the reference does (no transfers counted),
where Pillow imports.  Prints one JSON line.  Needs a GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from happypose_amd import augmentations as A  # noqa: E402
from happypose_amd import ops  # noqa: E402


def timed(fn, warmup: int, repeats: int, sync=True) -> dict:
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out-height", type=int, default=480)
    ap.add_argument("--out-width", type=int, default=640)
    ap.add_argument("--ids", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resize_bench needs a GPU"
    B, h, w, out_hw = a.batch, a.height, a.width, (a.out_height, a.out_width)
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    depth = rng.uniform(0.3, 2.0, (B, h, w)).astype(np.float32)
    # blocks of 40 x 40 pixels with ids 0 .. ids: objects of a plausible size rather than noise
    seg = np.kron(rng.integers(0, a.ids + 1, (B, (h + 39) // 40, (w + 39) // 40)), np.ones((40, 40), np.int64))[:, :h, :w].astype(np.int32)
    K = np.tile(np.array([[1000.0, 0, w / 2], [0, 1000.0, h / 2], [0, 0, 1]], np.float32), (B, 1, 1))
    ids = [list(range(1, a.ids + 1))] * B
    batch = A.ObservationBatch(rgb=torch.as_tensor(rgb).cuda(), depth=torch.as_tensor(depth).cuda(), segmentation=torch.as_tensor(seg).cuda(),
                               K=torch.as_tensor(K), object_ids=ids)
    T = A.CropResizeToAspectTransform(out_hw)
    box = T.crop_box(h, w)
    rect = None if box is None else tuple(int(round(v)) for v in box)
    result = {"batch": B, "height": h, "width": w, "out": list(out_hw), "ids": a.ids, "crop": rect, "repeats": a.repeats, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0)}
    out = T.apply(batch, {})
    parts = {"crop_resize_to_aspect": lambda: T.apply(batch, {}),
             "resize_rgb_bilinear": lambda: ops.resize_rgb(batch.rgb, out_hw, "bilinear", crop=rect),
             "resize_rgb_bicubic": lambda: ops.resize_rgb(batch.rgb, out_hw, "bicubic", crop=rect),
             "resize_nearest_segmentation": lambda: ops.resize_nearest(batch.segmentation, out_hw, crop=rect),
             "resize_nearest_depth": lambda: ops.resize_nearest(batch.depth, out_hw, crop=rect),
             "seg_boxes": lambda: ops.seg_boxes(out.segmentation, ids)}
    for name, fn in parts.items():
        result[name] = timed(fn, a.warmup, a.repeats)
    result["crop_resize_to_aspect"]["ms_per_frame"] = result["crop_resize_to_aspect"]["median_ms"] / B
    try:
        from PIL import Image
    except ImportError:
        result["pillow"] = "Pillow does not import on this machine"
    else:
        def host():
            for b in range(B):
                ims = [Image.fromarray(rgb[b]), Image.fromarray(seg[b]), Image.fromarray(depth[b])]
                if box is not None:
                    ims = [im.crop(box) for im in ims]
                size = (out_hw[1], out_hw[0])
                np.asarray(ims[0].resize(size, resample=Image.BILINEAR))
                s = np.asarray(ims[1].resize(size, resample=Image.NEAREST))
                np.asarray(ims[2].resize(size, resample=Image.NEAREST))
                for i in np.unique(s):  # make_detections_from_segmentation
                    where = np.where(s == i)
                    np.array([np.min(where[1]), np.min(where[0]), np.max(where[1]), np.max(where[0])])

        result["pillow"] = timed(host, 1, a.host_repeats, sync=False)
        result["pillow"]["note"] = "host, one image at a time, no transfers counted"
    print(json.dumps(result))


if __name__ == "__main__":
    main()
