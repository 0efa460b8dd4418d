"""Records Pillow's own results for the frame resizes into tests/golden/g15_resize.npz.

    python tools/gen_golden_resize.py

The cases and the seeded inputs are ``GOLDEN_CASES`` / ``golden_inputs()`` of tests/resize_ref.py: the smallest sizes at which
each path of the kernels is taken (both passes, one, none; windows clipped at both ends; the crop that rounds a half; the crop
that pads; a line whose window is longer than a default band).  Every case goes through ``Image.resize`` with BILINEAR, BICUBIC
and no filter argument (Pillow's default) on RGB, and with NEAREST on modes I and F; a case with a crop rectangle goes through
``Image.crop`` first.  Keys: ``in|<kind>|<input>``, ``rgb|<case>|<filter>``, ``i32|<case>``, ``f32|<case>`` and
``crop_round|<h>x<w>``, the rectangle ``Image.crop`` makes of the float box of the aspect crop.  Needs Pillow; the tests need only
the file.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import PIL
from PIL import Image

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import resize_ref as ref  # noqa: E402

PIL_FILTER = {ref.BILINEAR: Image.BILINEAR, ref.BICUBIC: Image.BICUBIC}


def main() -> None:
    inputs = ref.golden_inputs()
    data = {f"in|{kind}|{name}": x for kind, table in inputs.items() for name, x in table.items()}
    low = high = False
    for case, (src, (oh, ow), box, crop) in ref.GOLDEN_CASES.items():
        def run(x, **kw):
            im = Image.fromarray(x)
            if crop is not None:
                im = im.crop(crop)
            return np.asarray(im.resize((ow, oh), box=box, **kw))

        for f in ref.GOLDEN_FILTERS:
            data[f"rgb|{case}|{f}"] = y = run(inputs["rgb"][src], resample=PIL_FILTER[f])
            if "checker" in case and f == ref.BICUBIC:
                low |= bool((y == 0).any())
                high |= bool((y == 255).any())
        data[f"rgb|{case}|default"] = run(inputs["rgb"][src])
        if src in inputs["i32"]:
            si, sf = Image.fromarray(inputs["i32"][src]), Image.fromarray(inputs["f32"][src])
            assert si.mode == "I" and sf.mode == "F"
            data[f"i32|{case}"] = run(inputs["i32"][src], resample=Image.NEAREST).astype(np.int32)
            data[f"f32|{case}"] = run(inputs["f32"][src], resample=Image.NEAREST).astype(np.float32)
    assert low and high  # the bicubic overshoot is clipped on both sides somewhere
    # what Image.crop makes of the aspect crop's float box: the size of the cropped image says how each edge was rounded
    for h, w in ((40, 33), (33, 40), (20, 40)):
        box = ref.aspect_crop_box(h, w, (24, 32))
        im = Image.fromarray(np.zeros((h, w), np.uint8)).crop(box)
        data[f"crop_round|{h}x{w}"] = np.array([*box, im.size[1], im.size[0]], np.float64)
    data["pillow_version"] = np.array(PIL.__version__)
    path = ROOT / "tests" / "golden" / "g15_resize.npz"
    np.savez_compressed(path, **data)
    print(path, path.stat().st_size, "bytes,", len(data), "arrays")


if __name__ == "__main__":
    main()
