"""The comparisons of tests/test_gpu_mbconv.py have teeth -- shown without a GPU and without breaking a kernel: the same
comparison functions, on the same cases, with a MUTATED fp64 reference in the place of the kernels' output.  Each mutation is a
mistake an MBConv kernel could make at a border (test_gpu_mbconv.reference); each must miss the bound by at least 100x.

  sympad  symmetric padding instead of the (lo, hi) pads       stride-2 cases (at stride 1 the pads ARE symmetric)
  edge    border pixel repeated into the padding               all cases: only border outputs differ
  row     the SE mean sums a ragged strip's dead row           cases with SE
  nogate  the gate left out                                    cases with SE
  eps     depthwise BatchNorm folded with eps 1e-5             all cases

The parameters are the GPU tests' own (``make_params``, the same seeds): the SE weights are scaled ``SE_SCALE`` = 8x above He
for ``row`` -- one row more in a mean over Ho rows moves the pooled vector by about 1 / Ho of itself, and with gain-1 weights
the gate would move the output by only 16x the bound on the 132-row map of the se_pool_kernel case (100x at 4x, 155x at 8x)."""
import numpy as np
import pytest

import test_gpu_mbconv as t

MARGIN = 100.0

# the tests of this file need no GPU: drop the module-wide mark of the file the helpers come from
pytestmark = []


def _mutations(c):
    m = ["eps"] + (["sympad"] if c["s"] == 2 else [])
    if not ((c["k"], c["s"]) == (3, 2) and c["H"] % 2 and c["W"] % 2):  # pad 0 / 1 on an odd map: no output reaches the padding
        m.append("edge")
    return m + (["row", "nogate"] if "cout" in c else [])


@pytest.mark.parametrize("i", range(len(t.DW_CASES)), ids=[t.case_id(c) for c in t.DW_CASES])
def test_depthwise_comparison_has_teeth(i):
    p = t.make_params(t.DW_CASES[i], seed=i)
    ref = t.reference(p, p["x"])["dw"]
    assert t.ratio_dw(ref.astype(np.float32), ref) <= 0.01  # rounding the reference to fp32 is far inside the bound
    for m in _mutations(p["case"]):
        r = t.ratio_dw(t.reference(p, p["x"], mutate=m)["dw"], ref)
        assert r >= MARGIN, (m, r)


BLOCKS = [("strip", c, 20 + i, 0, 1) for i, c in enumerate(t.BLOCK_STRIP)] + \
         [("plain", c, 40 + i, 1, 2) for i, c in enumerate(t.BLOCK_PLAIN)] + \
         [("front", c, 60 + i, 1, 2) for i, c in enumerate(t.BLOCK_FRONT)]


@pytest.mark.parametrize("group,c,seed,gemms_dw,gemms_out", BLOCKS, ids=[g + "-" + t.case_id(c) for g, c, _, _, _ in BLOCKS])
def test_block_comparison_has_teeth(group, c, seed, gemms_dw, gemms_out):
    p = t.make_params(c, seed=seed, se_scale=t.SE_SCALE)
    x = t.stem_reference(p)
    ref = t.reference(p, x)
    assert t.ratio_map(ref["out"].astype(np.float32), ref["out"], gemms_out) <= 0.01
    for m in _mutations(c):
        mut = t.reference(p, x, mutate=m)
        r_out = t.ratio_map(mut["out"], ref["out"], gemms_out)
        assert r_out >= MARGIN, (m, "out", r_out)
        if m in ("edge", "eps", "sympad"):  # what the depthwise map's own comparison must catch
            r_dw = t.ratio_map(mut["dw"], ref["dw"], gemms_dw) if gemms_dw else t.ratio_dw(mut["dw"], ref["dw"])
            assert r_dw >= MARGIN, (m, "dw", r_dw)
        else:
            assert np.array_equal(mut["dw"], ref["dw"])


def test_same_pad_table_is_the_300_pixel_rule():
    """SAME_PAD restates Conv2dStaticSamePadding for image_size 300 from its definition; the 240 x 320 plan ends at 7 x 10."""
    for (k, s), (lo, hi) in t.SAME_PAD.items():
        o = -(-300 // s)
        total = max((o - 1) * s + k - 300, 0)
        assert (lo, hi) == (total // 2, total - total // 2)
    assert len(t.REAL_BLOCKS) == 26 and t.REAL_LAST == (7, 10)
    assert sorted({(c["H"], c["W"]) for c in t.REAL_BLOCKS}) == [(7, 10), (15, 20), (30, 40), (60, 80), (120, 160)]
