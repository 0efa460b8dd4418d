"""The NumPy restatement of the augmentations (tests/augmentations_ref.py) against Pillow's recorded results
(tests/golden/g14_augmentations.npz, tools/gen_golden_augmentations.py): byte for byte, every case, nothing left out -- and live
against Pillow where it imports.  The depth restatements, which have no reference on this machine, get checks of their own."""

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import augmentations_ref as R  # noqa: E402

OPS = {"brightness": R.OP_BRIGHTNESS, "color": R.OP_COLOR, "contrast": R.OP_CONTRAST, "sharpness": R.OP_SHARPNESS}


def restate(x, op, param):
    if op == "smooth":
        return R.smooth(x)
    if op == "blur":
        return R.gaussian_blur(x, int(param))
    return R.enhance(x, OPS[op], float(param))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(golden_dir / "g14_augmentations.npz"))


def test_restatement_equals_the_golden_byte_for_byte(golden):
    outs = [k for k in golden if k.startswith("out|")]
    assert len(outs) >= 250 and {k.split("|")[2] for k in outs} == set(OPS) | {"blur", "smooth"}
    differing = {}
    for key in outs:
        _, case, op, param = key.split("|")
        n = int((restate(golden[f"in|{case}"], op, param) != golden[key]).sum())
        if n:
            differing[key] = n
    assert not differing, differing


def test_golden_covers_the_edges(golden):
    """Every factor saturates at 0 and at 255 somewhere; Contrast has a mean just below and just above .5; the wide line is there."""
    for f in ("0", "0.1", "0.37", "1", "1.5", "6", "20", "50"):
        outs = [golden[k] for k in golden if k.startswith("out|") and k.endswith(f"|{f}") and k.split("|")[2] in OPS]
        assert len(outs) >= 4 and any((o == 0).any() for o in outs) and any((o == 255).any() for o in outs), f
    fr = [R.gray(golden[f"in|mean_{s}_half_13x17"]).astype(np.int64).sum() / 221 % 1 for s in ("below", "above")]
    assert 0.49 <= fr[0] < 0.5 <= fr[1] <= 0.51
    for s, up in (("below", 0), ("above", 1)):  # the rounding of the mean goes down below .5 and up above it
        x = golden[f"in|mean_{s}_half_13x17"]
        assert R.contrast_mean(x) == int(R.gray(x).astype(np.int64).sum()) // 221 + up
    assert golden["in|random_5x1031"].shape == (5, 1031, 3)


def test_blur_parameters():
    got = [R.blur_params(k) for k in (1, 2, 3)]
    assert [g[0] for g in got] == [0, 1, 2]
    assert [np.float32(g[3]) for g in got] == [np.float32(0.25000003), np.float32(1.375), np.float32(2.4166667)]
    for r, ww, fw, _ in got:
        assert 0 <= fw and (2 * r + 1) * ww + 2 * fw in ((1 << 24) - 1, 1 << 24)


def test_live_against_pillow():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance, ImageFilter

    enh = {"brightness": ImageEnhance.Brightness, "color": ImageEnhance.Color, "contrast": ImageEnhance.Contrast,
           "sharpness": ImageEnhance.Sharpness}
    rng = np.random.default_rng(5)
    for h, w in ((7, 6), (31, 45)):
        x = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        im = Image.fromarray(x)
        assert (np.asarray(im.filter(ImageFilter.SMOOTH)) == R.smooth(x)).all()
        for k in (1, 2, 3, 4):
            assert (np.asarray(im.filter(ImageFilter.GaussianBlur(k))) == R.gaussian_blur(x, k)).all(), k
        for f in (0.05, 0.9, 2.5, 33.0):
            for op, e in enh.items():
                assert (np.asarray(e(im).enhance(f)) == R.enhance(x, OPS[op], f)).all(), (op, f)


# ---- depth ---------------------------------------------------------------------------------------------------------------------------
def _depth(h, w, seed, holes=0.3):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.3, 2.0, (h, w)).astype(np.float32)
    d[rng.random((h, w)) < holes] = 0
    return d


@pytest.mark.parametrize("fraction", [0.0, 0.2, 0.9, 1.0])
def test_missing_drops_exactly_m(fraction):
    d = _depth(9, 13, 1)
    n_valid = int((d > 0).sum())
    out, dropped = R.missing(d, fraction, seed=77, image=2)
    assert int(dropped.sum()) == int(fraction * n_valid) and not dropped[d <= 0].any()
    assert (out[dropped] == 0).all() and (out[~dropped] == d[~dropped]).all()
    assert (R.missing(d, fraction, 77, 3)[1] != dropped).any() or dropped.sum() in (0, n_valid)


def test_missing_is_uniform_enough():
    d = np.ones((64, 80), np.float32)
    _, dropped = R.missing(d, 0.5, seed=3, image=0)
    assert dropped.sum() == 2560 and abs(dropped[:32].sum() - 1280) < 150  # 4 sigma of a hypergeometric draw is about 100


def test_normals_have_unit_variance():
    for dtype in (np.float32, np.float64):
        n = R.normals(R.words(200000, 9, 0, R.STREAM_NOISE), dtype)
        assert np.isfinite(n).all() and abs(n.mean()) < 0.01 and abs(n.std() - 1) < 0.01
    assert np.abs(R.normals(R.words(4096, 9, 1, 1), np.float32) - R.normals(R.words(4096, 9, 1, 1), np.float64)).max() < 1e-5


def test_bicubic_weights_sum_to_one_and_interpolate():
    t = np.linspace(0, 1, 101)
    w = R.cubic_weights(t, np.float64)
    assert np.abs(w.sum(axis=1) - 1).max() < 1e-15
    assert np.allclose(w[0], [0, 1, 0, 0]) and np.allclose(w[-1], [0, 0, 1, 0])
    g = np.random.default_rng(0).normal(size=(4, 6))
    assert np.array_equal(R.bicubic_upsample(g, 4, 6), g)  # identity: same size, every fraction is 0
    assert np.allclose(R.bicubic_upsample(np.full((2, 3), 0.7), 9, 13), 0.7, atol=1e-15)  # a constant stays a constant
    assert np.allclose(R.bicubic_upsample(np.array([[1.5]]), 5, 4), 1.5)  # a 1 x 1 grid: every tap is the one cell


def test_correlated_noise_zero_grid_and_invalid_pixels():
    d = _depth(20, 30, 4)
    d[0, 0], d[0, 1] = np.nan, -1.0
    d[0, 2] = 1.0
    assert np.array_equal(R.correlated_noise(d, 0.01, 0, 3, 1, 0), d.astype(np.float64), equal_nan=True)
    for out in (R.correlated_noise(d, 0.01, 2, 3, 1, 0), R.gaussian_noise(d, 0.01, 1, 0)):
        assert np.isnan(out[0, 0]) and out[0, 1] == -1.0 and out[0, 2] != 1.0 and (out[d == 0] == 0).all()
        assert np.abs(out - d)[d > 0].max() < 0.1


def test_ellipses_cover_and_last_wins():
    d = np.ones((21, 31), np.float32)
    u = (10 * 31 + 15 + 0.5) / d.size  # the centre pixel (15, 10)
    table = np.array([[u, 6, 3, 0, 0.25], [u, 2, 2, 0, -0.5]], np.float32)
    assert (R.ellipse_centres(d, table[:, 0]) == [[15, 10], [15, 10]]).all()
    out, covered, q = R.ellipses(d, table, 2, noise=True)
    assert covered[10, 21] and not covered[10, 22] and covered[13, 15] and not covered[14, 15]
    assert out[10, 15] == 0.5 and out[10, 20] == 1.25 and out[0, 0] == 1.0  # the second ellipse wins where both cover
    out, covered, _ = R.ellipses(d, table, 2, noise=False)
    assert (out[covered] == 0).all() and (out[~covered] == 1).all()
    rot = table.copy()
    rot[:, 3] = 90
    assert R.ellipses(d, rot, 1, False)[1][16, 15] and not R.ellipses(d, rot, 1, False)[1][10, 19]  # the long axis now runs along y
    table[0, 1] = 0  # rx = 0: half a pixel wide, the centre column alone
    c = R.ellipses(d, table, 1, False)[1]
    assert c[:, 15].sum() == 7 and c.sum() == 7
    assert not R.ellipses(np.zeros_like(d), table, 2, False)[1].any() and not R.ellipses(d, table, 0, False)[1].any()


def test_depth_blur_definition():
    d = _depth(8, 13, 6, holes=0.2)
    assert np.array_equal(R.depth_blur(d, 1), d.astype(np.float64))
    b4 = R.depth_blur(d, 4)
    assert np.isclose(b4[4, 6], d[2:6, 4:8].astype(np.float64).sum() / 16)  # k = 4 covers x - 2 .. x + 1
    assert np.isclose(R.depth_blur(d, 3)[0, 0], d[np.ix_([1, 0, 1], [1, 0, 1])].astype(np.float64).sum() / 9)  # reflect-101
    assert np.allclose(R.depth_blur(np.full((7, 7), 0.5, np.float32), 7), 0.5)
    with pytest.raises(AssertionError):
        R.depth_blur(d[:3], 4)
