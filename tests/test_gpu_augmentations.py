"""The augmentation kernels (csrc/augment.hip) on the device.

RGB: every case of tests/golden/g14_augmentations.npz (Pillow's own output) byte for byte, no tolerance, on the LDS path and on
the general path of the blur; a mixed batch; in-place calls where the header allows them.  Depth: the integer-defined transforms
(masks, missing pixels, ellipse coverage) exactly against tests/augmentations_ref.py, the float ones within 4 x the largest
difference between the restatement in float32 and in float64 on that case, floor one float32 ulp of the value.  The yardsticks
and measured errors are printed (CHANGELOG: "Training-image augmentations").

Shapes: 1 x 1 .. 40 x 33 and the 5 x 1031 line (wider than the 1024-pixel LDS line) for RGB -- H W a multiple of 4 (dword
path) and not (byte path); 7 x 11 / 33 x 65 (odd, more than one workgroup), 9 x 13 and 64 x 80 (5120 pixels: 5 strides of the
one-workgroup-per-image kernels, 80 groups of 64) for depth."""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import augmentations_ref as R  # noqa: E402

from happypose_amd import augmentations as A  # noqa: E402
from happypose_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPS = {"brightness": R.OP_BRIGHTNESS, "color": R.OP_COLOR, "contrast": R.OP_CONTRAST, "sharpness": R.OP_SHARPNESS}
SEED = 0x1234567F9ABCDEF1


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return torch.equal(bits(a), bits(b))


def twice(fn):
    """The call's result, after checking that a second call gives the same bits."""
    a, b = fn(), fn()
    assert same(a, b)
    return a


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(golden_dir / "g14_augmentations.npz"))


def _cases(golden):
    return sorted(k.split("|")[1] for k in golden if k.startswith("in|"))


CASES = ["gradient_40x33", "mean_above_half_13x17", "mean_below_half_13x17", "random_13x17", "random_1x1", "random_2x9", "random_3x5",
         "random_40x33", "random_5x1031"]


def test_case_list_is_the_golden(golden):
    assert _cases(golden) == CASES


@pytest.mark.parametrize("case", CASES)
def test_rgb_enhance_equals_pillow(golden, case):
    """All enhancer outputs of the case in ONE batch (the same frame B times, each with its own op and factor), plus SMOOTH as
    Sharpness at factor 0."""
    x = golden[f"in|{case}"]
    keys = [k for k in golden if k.startswith(f"out|{case}|") and k.split("|")[2] in OPS] + [f"out|{case}|smooth|0"]
    op = [OPS.get(k.split("|")[2], R.OP_SHARPNESS) for k in keys]
    f = [float(k.split("|")[3]) for k in keys]
    rgb = dev(np.stack([x] * len(keys)))
    out = twice(lambda: ops.aug_rgb_enhance(rgb, op, f)).cpu().numpy()
    differing = {k: int((out[i] != golden[k]).sum()) for i, k in enumerate(keys) if (out[i] != golden[k]).any()}
    assert not differing, differing


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_rgb_blur_equals_pillow(golden, case, general):
    """Radii 1, 2, 3 in one batch; ``general`` forces the one-launch-per-pass path (the 5 x 1031 rows take it anyway)."""
    x = golden[f"in|{case}"]
    rgb = dev(np.stack([x] * 3))
    out = twice(lambda: ops.aug_rgb_blur(rgb, [1, 2, 3], force_general=general)).cpu().numpy()
    for i, k in enumerate((1, 2, 3)):
        assert (out[i] == golden[f"out|{case}|blur|{k}"]).all(), (k, int((out[i] != golden[f"out|{case}|blur|{k}"]).sum()))


def test_rgb_mixed_batch(golden):
    """B = 3 with different ops and factors and one apply = 0: the untouched image comes back bit for bit, each of the others
    equals its single-image result and Pillow."""
    names = ["random_13x17", "mean_above_half_13x17", "mean_below_half_13x17"]
    rgb = dev(np.stack([golden[f"in|{n}"] for n in names]))
    op, f, flags = ["contrast", "sharpness", "color"], [1.5, 6.0, 0.37], [True, False, True]
    out = ops.aug_rgb_enhance(rgb, op, f, flags)
    assert torch.equal(out[1], rgb[1])
    for i in (0, 2):
        assert torch.equal(out[i], ops.aug_rgb_enhance(rgb[i:i + 1].contiguous(), op[i], f[i])[0])
        assert (out[i].cpu().numpy() == golden[f"out|{names[i]}|{op[i]}|{f[i]!r}"]).all()
    out = ops.aug_rgb_blur(rgb, [3, 1, 2], [True, False, True])
    assert torch.equal(out[1], rgb[1])
    for i, k in ((0, 3), (2, 2)):
        assert torch.equal(out[i], ops.aug_rgb_blur(rgb[i:i + 1].contiguous(), k)[0])
        assert (out[i].cpu().numpy() == golden[f"out|{names[i]}|blur|{k}"]).all()
    for call in (lambda o: ops.aug_rgb_enhance(rgb, op, f, out=o), lambda o: ops.aug_rgb_blur(rgb, 2, out=o)):
        with pytest.raises(ValueError):
            call(rgb)  # a neighbourhood: not in place


def _masks(h, w, rng):
    seg = rng.integers(0, 3, (4, h, w)).astype(np.int32)
    seg[1] = 0  # all background
    seg[2] = rng.integers(1, 5, (h, w))  # no background
    return seg


@pytest.mark.parametrize("h,w", [(7, 11), (33, 65), (8, 12)])
def test_background_and_dropouts_exact(h, w):
    rng = np.random.default_rng(h)
    seg = _masks(h, w, rng)
    rgb, bg = rng.integers(0, 256, (4, h, w, 3), dtype=np.uint8), rng.integers(0, 256, (4, h, w, 3), dtype=np.uint8)
    depth = rng.uniform(0.2, 3, (4, h, w)).astype(np.float32)
    flags = [True, True, True, False]
    d_rgb, d_bg, d_seg, d_depth = dev(rgb), dev(bg), dev(seg), dev(depth)
    want_rgb = np.stack([R.replace_background(rgb[i], seg[i], bg[i]) if flags[i] else rgb[i] for i in range(4)])
    out = twice(lambda: ops.aug_replace_background(d_rgb, d_seg, d_bg, flags))
    assert (out.cpu().numpy() == want_rgb).all() and (want_rgb[1] == bg[1]).all() and (want_rgb[2] == rgb[2]).all()
    for s in (seg, None):
        want = np.stack([R.depth_mask(depth[i], None if s is None else s[i]) if flags[i] else depth[i] for i in range(4)])
        out = twice(lambda: ops.aug_depth_mask(d_depth, None if s is None else d_seg, flags))
        assert (out.cpu().numpy() == want).all()
        inplace = d_depth.clone()
        assert ops.aug_depth_mask(inplace, None if s is None else d_seg, flags, out=inplace) is inplace and same(inplace, out)
    inplace = d_rgb.clone()
    ops.aug_replace_background(inplace, d_seg, d_bg, flags, out=inplace)
    assert (inplace.cpu().numpy() == want_rgb).all()


def _depth(h, w, seed, holes=0.3):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.3, 2.0, (h, w)).astype(np.float32)
    d[rng.random((h, w)) < holes] = 0
    return d


def test_missing_drops_the_restatements_set():
    full = _depth(9, 13, 1, holes=0)
    one = np.zeros_like(full)
    one[4, 7] = 1.0
    holes = _depth(9, 13, 2)
    holes[0, 0], holes[0, 1] = np.nan, -2.0  # not valid: never counted, never dropped
    imgs = [np.zeros_like(full), one, one, full, full, full, full, holes, holes, full]
    frac = [0.5, 0.9, 1.0, 0.0, 0.2, 0.9, 116.5 / 117, 0.2, 0.9, 0.2]
    assert R.missing_count(frac[6], 117) == 116  # m == n_valid - 1
    depth = dev(np.stack(imgs))
    out = twice(lambda: ops.aug_depth_missing(depth, frac, SEED)).cpu().numpy()
    for b, (img, fr) in enumerate(zip(imgs, frac)):
        want, dropped = R.missing(img, fr, SEED, b)
        assert np.array_equal(out[b], want, equal_nan=True), b
        assert int(dropped.sum()) == int(fr * int((img > 0).sum()))
    assert ((out[4] == 0) != (out[9] == 0)).any()  # the same content and fraction at another index: another set
    inplace = depth.clone()
    ops.aug_depth_missing(inplace, frac, SEED, out=inplace)
    assert np.array_equal(inplace.cpu().numpy(), out, equal_nan=True)
    keep = ops.aug_depth_missing(depth, frac, SEED, [False] * 10)
    assert same(keep, depth)


def test_missing_on_a_larger_frame():
    imgs = [_depth(64, 80, 3), _depth(64, 80, 3), np.ones((64, 80), np.float32)]
    frac = [0.2, 0.9, 0.5]
    out = twice(lambda: ops.aug_depth_missing(dev(np.stack(imgs)), frac, SEED + 1)).cpu().numpy()
    for b in range(3):
        want, dropped = R.missing(imgs[b], frac[b], SEED + 1, b)
        assert np.array_equal(out[b], want) and dropped.sum() == int(frac[b] * (imgs[b] > 0).sum())


def _check(name, got, ref32, ref64):
    """4 x the restatement's own float32-vs-float64 difference on the case, floor one float32 ulp of the value."""
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(ref64)
        assert np.array_equal(np.isnan(got), np.isnan(ref64))
        yard = float(np.abs(ref32.astype(np.float64) - ref64)[finite].max())
        err = np.abs(got.astype(np.float64) - ref64)
        tol = np.maximum(4 * yard, np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64))
        print(f"{name}: yardstick {yard:.3e}, bound {4 * yard:.3e} (floor 1 ulp), device error {err[finite].max():.3e}")
        assert (err[finite] <= tol[finite]).all(), (name, float(err[finite].max()), yard)


def _with_oddities(d):
    d = d.copy()
    d[0, 0], d[0, 1], d[0, 2] = np.nan, -1.5, 0.0
    return d


@pytest.mark.parametrize("h,w", [(7, 11), (33, 65)])
def test_gaussian_noise(h, w):
    imgs = [_with_oddities(_depth(h, w, 5)), _depth(h, w, 6, holes=0), _depth(h, w, 7)]
    std, flags = [0.01, 0.02, 0.05], [True, True, False]
    depth = dev(np.stack(imgs))
    out = twice(lambda: ops.aug_depth_noise(depth, std, SEED, None, flags))
    got = out.cpu().numpy()
    for b in (0, 1):
        _check(f"gaussian noise {h}x{w} image {b}", got[b], R.gaussian_noise(imgs[b], std[b], SEED, b, np.float32),
               R.gaussian_noise(imgs[b], std[b], SEED, b))
    assert np.isnan(got[0, 0, 0]) and got[0, 0, 1] == -1.5 and got[0, 0, 2] == 0 and (got[1] != imgs[1]).all()
    assert same(out[2], depth[2])
    inplace = depth.clone()
    ops.aug_depth_noise(inplace, std, SEED, None, flags, out=inplace)
    assert same(inplace, out)


@pytest.mark.parametrize("h,w", [(20, 30), (33, 65)])
def test_correlated_noise(h, w):
    """Grids 1 x 1, 2 x 3, a zero-side grid and a larger one in one batch."""
    grids = [(1, 1), (2, 3), (0, 3), (5, 7)]
    imgs = [_with_oddities(_depth(h, w, 10 + i, holes=0.1)) for i in range(4)]
    depth = dev(np.stack(imgs))
    gh, gw = [g[0] for g in grids], [g[1] for g in grids]
    out = twice(lambda: ops.aug_depth_noise(depth, 0.01, SEED, (gh, gw)))
    got = out.cpu().numpy()
    for b, (a, c) in enumerate(grids):
        _check(f"correlated noise {h}x{w} grid {a}x{c}", got[b], R.correlated_noise(imgs[b], 0.01, a, c, SEED, b, np.float32),
               R.correlated_noise(imgs[b], 0.01, a, c, SEED, b))
        assert np.isnan(got[b, 0, 0]) and got[b, 0, 1] == -1.5 and got[b, 0, 2] == 0
    assert same(out[2], depth[2]) and not same(out[0], depth[0])
    inplace = depth.clone()
    ops.aug_depth_noise(inplace, 0.01, SEED, (gh, gw), out=inplace)
    assert same(inplace, out)


@pytest.mark.parametrize("h,w", [(7, 7), (8, 13), (33, 65)])
def test_depth_blur(h, w):
    ks = [3, 4, 7, 5]
    imgs = [_depth(h, w, 20 + i, holes=0.2) for i in range(4)]
    depth = dev(np.stack(imgs))
    out = twice(lambda: ops.aug_depth_blur(depth, ks, [True, True, True, False]))
    got = out.cpu().numpy()
    for b in range(3):
        _check(f"depth blur {h}x{w} k={ks[b]}", got[b], R.depth_blur(imgs[b], ks[b], np.float32), R.depth_blur(imgs[b], ks[b]))
    assert same(out[3], depth[3])
    with pytest.raises(ValueError):
        ops.aug_depth_blur(depth, 3, out=depth)


def test_depth_blur_side_shorter_than_k():
    depth = dev(np.ones((2, 6, 9), np.float32))
    with pytest.raises(AssertionError, match="shorter"):
        ops.aug_depth_blur(depth, [3, 7])
    torch.cuda.synchronize()  # nothing was launched: nothing to fail
    assert float(ops.aug_depth_blur(depth, [3, 6]).sum()) == pytest.approx(108)


# ellipses on 48 x 64: oblique angles, so that no pixel sits exactly on a boundary, except the rx = 0 needle at angle 0
def _ellipse_batch():
    h, w = 48, 64
    full = np.ones((h, w), np.float32)
    holes = _with_oddities(_depth(h, w, 30, holes=0.2))
    u = lambda x, y: np.float32((y * w + x + 0.5) / (h * w))  # noqa: E731  (on a frame without holes)
    t0 = [[u(20, 20), 12, 8, 30, 0.25], [u(28, 24), 10, 6, 75, -0.5], [u(40, 12), 9, 9, 10, 0.125], [u(30, 22), 3, 2, 145, 1.0],
          [0.0, 7, 5, 50, 0.375], [u(63, 47), 8, 3, 100, -0.25], [u(10, 40), 0, 3, 0, 2.0]]  # border centres (0, 0), (63, 47); rx = 0
    rng = np.random.default_rng(31)
    t1 = np.stack([rng.random(7), rng.integers(2, 12, 7), rng.integers(2, 12, 7), rng.integers(1, 89, 7) + 90 * rng.integers(0, 4, 7),
                   rng.normal(0, 0.01, 7)], axis=1)
    table = np.stack([np.asarray(t0, np.float32), t1.astype(np.float32), np.asarray(t0, np.float32), np.asarray(t0, np.float32),
                      np.asarray(t0, np.float32)])
    imgs = [full, holes, full, np.zeros_like(full), full]
    count = [7, 7, 0, 7, 9]  # count = 0, n_valid = 0, and a count beyond the table (clamped to 7)
    return imgs, table, count


def test_ellipses():
    imgs, table, count = _ellipse_batch()
    depth = dev(np.stack(imgs))
    drop = twice(lambda: ops.aug_depth_ellipses(depth, table, count, False)).cpu().numpy()
    noise = twice(lambda: ops.aug_depth_ellipses(depth, table, count, True)).cpu().numpy()
    inside = borderline = 0
    for b, img in enumerate(imgs):
        n = min(count[b], 7)
        ref, covered, q64 = R.ellipses(img, table[b], n, False)
        if not covered.any():
            assert np.array_equal(drop[b], img, equal_nan=True) and np.array_equal(noise[b], img, equal_nan=True), b
            continue
        q32 = R.ellipses(img, table[b], n, False, np.float32)[2].astype(np.float64)
        near = np.abs(q64 - 1) < 0.5
        yard = 4 * float(np.abs(q32 - q64)[near].max())
        open_ = (np.abs(q64 - 1) <= yard).any(axis=0)  # a pixel whose form is within the yardstick of 1 may fall on either side
        print(f"ellipses image {b}: form yardstick {yard / 4:.3e}, bound {yard:.3e}, {int(open_.sum())} open of {int(covered.sum())} inside")
        inside, borderline = inside + int(covered.sum()), borderline + int(open_.sum())
        with np.errstate(invalid="ignore"):
            got_covered = np.where(img != 0, drop[b] == 0, covered)  # a pixel that was 0 already shows nothing
            got_covered = np.where(np.isnan(img), ~np.isnan(drop[b]), got_covered)
        assert (got_covered == covered)[~open_].all(), b
        assert np.array_equal(drop[b][~covered & ~open_], img[~covered & ~open_], equal_nan=True)
        r32, r64 = R.ellipses(img, table[b], n, True, np.float32)[0], R.ellipses(img, table[b], n, True)[0]
        keep = ~open_
        _check(f"ellipse noise image {b}", noise[b][keep], r32[keep], r64[keep])
    assert inside > 1000 and borderline <= 0.01 * inside, (borderline, inside)  # the restatement alone stays within 1 %
    full_noise = noise[0]
    assert full_noise[20, 20] in (np.float32(1.25), np.float32(0.5), np.float32(2.0))  # covered by several: the last one wins
    ref = R.ellipses(imgs[0], table[0], 7, True)[0]
    assert ref[24, 28] == 0.5 or ref[24, 28] == 2.0  # ellipses 0 and 1 overlap there; 1 (or the later 3) wins over 0
    assert np.isnan(noise[1][0, 0]) and noise[1][0, 1] == -1.5 and noise[1][0, 2] == 0  # not valid: nothing is added
    assert np.array_equal(drop[4], drop[0]) and np.array_equal(noise[4], noise[0])
    inplace = depth.clone()
    ops.aug_depth_ellipses(inplace, table, count, True, out=inplace)
    assert np.array_equal(inplace.cpu().numpy(), noise, equal_nan=True)
    assert same(ops.aug_depth_ellipses(depth, table, count, False, [False] * 5), depth)


def test_chains_run_end_to_end():
    """The factory chains through the user-facing layer: shapes and dtypes stay, an image no augmentation applied to comes back
    bit for bit, and a seed reproduces the batch."""
    rng = np.random.default_rng(40)
    B, h, w = 6, 24, 36
    seg = rng.integers(0, 3, (B, h, w)).astype(np.int32)
    batch = A.ObservationBatch(rgb=dev(rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)), depth=dev(np.stack([_depth(h, w, i) for i in range(B)])),
                               segmentation=dev(seg), background=dev(rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)))
    chain = A.make_background_augmentations() + A.make_rgb_augmentations() + A.make_depth_augmentations(2)
    a = A.apply_augmentations(chain, batch, np.random.default_rng(7))
    b = A.apply_augmentations(chain, batch, np.random.default_rng(7))
    assert same(a.rgb, b.rgb) and same(a.depth, b.depth) and a.rgb.shape == batch.rgb.shape and a.depth.dtype == torch.float32
    assert not same(a.rgb, batch.rgb) and not same(a.depth, batch.depth)
    off = [A.SceneObservationAugmentation(c.transform, p=-1.0) for c in chain]  # random() <= p never holds
    c = A.apply_augmentations(off, batch, np.random.default_rng(7))
    assert same(c.rgb, batch.rgb) and same(c.depth, batch.depth)
