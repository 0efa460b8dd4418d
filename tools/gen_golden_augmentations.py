"""Records Pillow's own results for the RGB augmentations into tests/golden/g14_augmentations.npz.

    python tools/gen_golden_augmentations.py

Seeded random uint8 images (each with one pure black and one pure white pixel where it has room), one smooth gradient image and
two images whose mean gray lies just below and just above .5 go through ImageEnhance.{Brightness, Color, Contrast, Sharpness},
ImageFilter.GaussianBlur and ImageFilter.SMOOTH.  Keys: ``in|<case>`` and ``out|<case>|<op>|<parameter>``.  Every enhancer
factor runs on every case up to 40 x 33; the 5 x 1031 line (wider than any tile of the kernels) takes two factors, to keep the
file small.  Needs Pillow; the tests need only the file.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
from PIL import Image, ImageEnhance, ImageFilter
import PIL

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

SIZES = [(1, 1), (2, 9), (3, 5), (13, 17), (40, 33), (5, 1031)]
FACTORS = [0, 0.1, 0.37, 1, 1.5, 6, 20, 50]
WIDE_FACTORS = [0.37, 6]
RADII = [1, 2, 3]
ENHANCERS = {"brightness": ImageEnhance.Brightness, "color": ImageEnhance.Color, "contrast": ImageEnhance.Contrast,
             "sharpness": ImageEnhance.Sharpness}


def gray(x):
    c = x.astype(np.int64)
    return (c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16


def cases() -> dict:
    rng = np.random.default_rng(14)
    out = {}
    for h, w in SIZES:
        x = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if h * w >= 2:
            x[0, 0], x[-1, -1] = 0, 255
        out[f"random_{h}x{w}"] = x
    yy, xx = np.meshgrid(np.arange(40), np.arange(33), indexing="ij")
    out["gradient_40x33"] = np.stack([(yy * 255) // 39, (xx * 255) // 32, ((yy + xx) * 255) // 71], axis=-1).astype(np.uint8)
    # Contrast: a mean gray whose fractional part is within 0.01 of .5, on either side (one gray pixel is tuned)
    for name, target in (("mean_below_half_13x17", 110), ("mean_above_half_13x17", 111)):
        x = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
        x[6, 8] = 0
        x[6, 8] = (target - int(gray(x).sum())) % 221
        frac = gray(x).sum() / 221 % 1
        assert abs(frac - 0.5) < 0.01 and (frac < 0.5) == (target == 110), frac
        out[name] = x
    return out


def main() -> None:
    data = {}
    zero = {f: False for f in FACTORS}
    full = {f: False for f in FACTORS}
    for name, x in cases().items():
        data[f"in|{name}"] = x
        im = Image.fromarray(x)
        data[f"out|{name}|smooth|0"] = np.asarray(im.filter(ImageFilter.SMOOTH))
        for k in RADII:
            data[f"out|{name}|blur|{k}"] = np.asarray(im.filter(ImageFilter.GaussianBlur(k)))
        for f in (WIDE_FACTORS if x.shape[1] > 1024 else FACTORS):
            for op, enh in ENHANCERS.items():
                y = np.asarray(enh(im).enhance(f))
                data[f"out|{name}|{op}|{f!r}"] = y
                zero[f] |= bool((y == 0).any())
                full[f] |= bool((y == 255).any())
    for f in FACTORS:  # every factor has a case that reaches 0 and one that reaches 255
        assert zero[f] and full[f], (f, zero[f], full[f])
    data["pillow_version"] = np.array(PIL.__version__)
    path = ROOT / "tests" / "golden" / "g14_augmentations.npz"
    np.savez_compressed(path, **data)
    print(path, path.stat().st_size, "bytes,", len(data), "arrays")


if __name__ == "__main__":
    main()
