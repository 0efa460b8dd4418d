"""Times the augmentation chains on the device: the full RGB chain (blur, sharpness, contrast, brightness, color) and the
strongest depth chain (level 2) on B = 32 frames of 480 x 640 with EVERY apply flag set.

    python tools/augment_bench.py [--batch 32] [--height 480] [--width 640] [--repeats 30] [--warmup 5]

Method: parameters are drawn once on the host (seeded); after the warm-up calls each timed call is bracketed by a device
synchronise and timed with the host clock; the median of the repeats is reported, in one process.  The time includes the upload
of the per-image parameter arrays and the allocation of outputs and workspaces through torch's caching allocator.  Beside it the
same RGB chain runs through Pillow on the host (one image at a time, as the reference does) where Pillow imports; the depth chain
has no reference timing (the reference needs OpenCV).  Prints one JSON line.  Needs a GPU: there is no fallback.
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


def every_image(chain):
    """The chain's transforms with probability 1 at every level."""
    out = []
    for aug in chain:
        inner = every_image(aug.transform) if isinstance(aug.transform, list) else aug.transform
        out.append(A.SceneObservationAugmentation(inner, p=1.0))
    return out


def timed(fn, warmup: int, repeats: int) -> dict:
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "augment_bench needs a GPU"
    B, h, w = a.batch, a.height, a.width
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    depth = rng.uniform(0.3, 2.0, (B, h, w)).astype(np.float32)
    depth[rng.random((B, h, w)) < 0.2] = 0
    seg = (rng.random((B, h, w)) < 0.4).astype(np.int32)
    batch = A.ObservationBatch(rgb=torch.as_tensor(rgb).cuda(), depth=torch.as_tensor(depth).cuda(), segmentation=torch.as_tensor(seg).cuda())
    result = {"batch": B, "height": h, "width": w, "repeats": a.repeats, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for name, chain in (("rgb_chain", every_image(A.make_rgb_augmentations())), ("depth_chain_level2", every_image(A.make_depth_augmentations(2)))):
        params = [aug.draw(B, np.random.default_rng(1)) for aug in chain]

        def run(chain=chain, params=params):
            out = batch
            for aug, p in zip(chain, params):
                out = aug.apply(out, p)
            return out

        result[name] = timed(run, a.warmup, a.repeats)
        result[name]["ms_per_frame"] = result[name]["median_ms"] / B
    try:
        from PIL import Image, ImageEnhance, ImageFilter
    except ImportError:
        result["pillow_rgb_chain"] = "Pillow does not import on this machine"
    else:
        p = [aug.draw(B, np.random.default_rng(1)) for aug in every_image(A.make_rgb_augmentations())][0]["inner"]
        k, fs = p[0]["inner"]["k"], [q["inner"]["factor"] for q in p[1:]]
        enh = [ImageEnhance.Sharpness, ImageEnhance.Contrast, ImageEnhance.Brightness, ImageEnhance.Color]

        def host():
            for b in range(B):
                im = Image.fromarray(rgb[b]).filter(ImageFilter.GaussianBlur(int(k[b])))
                for e, f in zip(enh, fs):
                    im = e(im).enhance(float(f[b]))
                np.asarray(im)

        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            host()
            ts.append((time.perf_counter() - t0) * 1e3)
        result["pillow_rgb_chain"] = {"median_ms": statistics.median(ts), "note": "host, one image at a time, no transfers counted"}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
