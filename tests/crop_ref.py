"""Reference of the crop-and-resize (crop.hip, crop_math.h, the fused output pass of raster.hip): torchvision's
``roi_align(aligned=False, spatial_scale=1)`` as ``TB/lib3d/cropping.py:155-197`` calls it, the RGB-D validity rule and the depth
normalisation of ``normalize_images`` (MP/models/pose_rigid.py:455-544), in numpy on the CPU.

What is float32 here belongs to the DEFINITION: the sample coordinates ``start + p*bin + (s+0.5)*bin/g`` (torchvision computes them
in float32 too) carry the discrete rules -- a sample is dropped outside ``[-1, size]``, clamped at 0, collapsed onto ``size-1``.
Everything after that is float64 in the literal order of the double loop over the samples: the weights ``l`` and ``1-l``, their
products, the sum and the division by ``g*g``.  Nothing here knows the kernels' fold; ``axis_spans`` / ``tile_paths`` derive from the
definition alone which tiles a fold over at most ``K_SPAN`` source indices can serve, and the tests use them to prove that a case
reaches the path it is named after.  The case table at the end is shared by the CPU and the GPU tests."""

import numpy as np

F = np.float32
K_SPAN = 5          # source rows / columns a separable fold holds (crop_math.h kSpan)
TILE = (32, 64)     # output rows x columns of a workgroup of the stand-alone kernel
VALID_THRESHOLD = float(F(0.99))  # ``mask >= 0.99`` on a float32 tensor compares with the float32 constant


def axis_samples(start, bin_size, n, size, g):
    """Sample placement and boundary rules along one axis for the output indices ``0..n-1``: ``(valid, lo, hi, l)`` of shape
    ``[n, g]``; coordinates float32, the upper weight ``l`` float64 (``coordinate - lo`` is exact in either format)."""
    start, bin_size = F(start), F(bin_size)
    p = np.arange(n, dtype=F)[:, None]
    s = np.arange(g, dtype=F)[None, :]
    y = (start + p * bin_size) + ((s + F(0.5)) * bin_size) / F(g)
    assert y.dtype == F
    valid = ~((y < F(-1.0)) | (y > F(size)))
    y = np.where(y <= 0, F(0), y)
    lo = y.astype(np.int64)
    top = lo >= size - 1
    lo = np.where(top, size - 1, lo)
    hi = np.where(top, size - 1, lo + 1)
    y = np.where(top, lo.astype(F), y)
    return valid, lo, hi, y.astype(np.float64) - lo


def box_bins(box, out_size):
    """``(x1, y1, bin_w, bin_h)`` in float32: the box clamp ``max(x2 - x1, 1)`` of aligned=False."""
    x1, y1, x2, y2 = [F(v) for v in box]
    rw, rh = max(x2 - x1, F(1.0)), max(y2 - y1, F(1.0))
    return x1, y1, rw / F(out_size[1]), rh / F(out_size[0])


def roi_align_ref(images, boxes, im_ids, out_size, sampling_ratio):
    """``images [Bi, C, H, W]``, ``boxes [n, 4]`` xyxy, ``im_ids [n]`` -> float64 ``[n, C, oh, ow]``."""
    images = np.asarray(images)
    _, C, H, W = images.shape
    oh, ow = out_size
    g = int(sampling_ratio)
    out = np.zeros((len(boxes), C, oh, ow), np.float64)
    for r, (box, im) in enumerate(zip(np.asarray(boxes, F), im_ids)):
        img = images[int(im)].astype(np.float64)
        x1, y1, bin_w, bin_h = box_bins(box, out_size)
        vy, ylo, yhi, ly = axis_samples(y1, bin_h, oh, H, g)
        vx, xlo, xhi, lx = axis_samples(x1, bin_w, ow, W, g)
        acc = np.zeros((C, oh, ow), np.float64)
        for iy in range(g):
            hy, ly_ = (1.0 - ly[:, iy])[:, None], ly[:, iy][:, None]
            for ix in range(g):
                hx, lx_ = (1.0 - lx[:, ix])[None, :], lx[:, ix][None, :]
                ok = vy[:, iy][:, None] & vx[:, ix][None, :]
                yl, yh, xl, xh = ylo[:, iy][:, None], yhi[:, iy][:, None], xlo[:, ix][None, :], xhi[:, ix][None, :]
                val = (hy * hx) * img[:, yl, xl] + (hy * lx_) * img[:, yl, xh] + (ly_ * hx) * img[:, yh, xl] + (ly_ * lx_) * img[:, yh, xh]
                acc += np.where(ok, val, 0.0)
        out[r] = acc / float(g * g)
    return out


def normalize_depth(d, z, mode):
    """Depth modes of ``normalize_images``: 0 none, 1 ``d / z``, 2 ``clamp(d / z, 0, 2) - 1``, 3 ``clamp(d - z, -2, 2)``."""
    if mode == 1:
        return d / z
    if mode == 2:
        return np.clip(d / z, 0.0, 2.0) - 1.0
    if mode == 3:
        return np.clip(d - z, -2.0, 2.0)
    assert mode == 0
    return d


def crop_ref(images, boxes, im_ids, out_size, sampling_ratio=4, n_channels=None, depth_norm_z=None, depth_norm_mode=0):
    """``crop_images`` on the first ``n_channels`` planes: ``(crops [n, C, oh, ow] float64, mask [n, oh, ow] float64 or None)``.
    With 4 channels the validity mask ``depth > 0`` goes through the same interpolation (``mask``), depth is zeroed where it is
    below 0.99 and then normalised with ``depth_norm_z [n]``."""
    images = np.asarray(images)
    C = images.shape[1] if n_channels is None else n_channels
    crops = roi_align_ref(images[:, :C], boxes, im_ids, out_size, sampling_ratio)
    if C < 4:
        return crops, None
    mask = roi_align_ref((images[:, 3:4] > 0).astype(np.float64), boxes, im_ids, out_size, sampling_ratio)[:, 0]
    d = np.where(mask >= VALID_THRESHOLD, crops[:, 3], 0.0)
    if depth_norm_mode:
        d = normalize_depth(d, np.asarray(depth_norm_z, np.float64)[:, None, None], depth_norm_mode)
    crops[:, 3] = d
    return crops, mask


def axis_spans(start, bin_size, n, size, g):
    """Per output index, the number of distinct source indices between the first and the last one its valid samples touch
    (0 when no sample is valid): what a fold of that output row / column has to hold."""
    valid, lo, hi, _ = axis_samples(start, bin_size, n, size, g)
    first = np.where(valid, lo, 1 << 30).min(1)
    last = np.where(valid, hi, -1).max(1)
    return np.where(last >= first, last - first + 1, 0)


def tile_paths(box, out_size, frame_size, g, tile=TILE):
    """Which path every ``tile`` (rows x columns) of output pixels of one crop must take: ``dict(separable [ty, tx] bool,
    span_y [ty], span_x [tx]: the largest span of the tile's rows / columns, live [ty, tx]: some pixel has a valid sample)``.
    A tile is separable when no row and no column of it needs more than ``K_SPAN`` source indices."""
    x1, y1, bin_w, bin_h = box_bins(box, out_size)
    sy = axis_spans(y1, bin_h, out_size[0], frame_size[0], g)
    sx = axis_spans(x1, bin_w, out_size[1], frame_size[1], g)
    span_y = np.array([sy[i:i + tile[0]].max() for i in range(0, out_size[0], tile[0])])
    span_x = np.array([sx[i:i + tile[1]].max() for i in range(0, out_size[1], tile[1])])
    return dict(separable=(span_y[:, None] <= K_SPAN) & (span_x[None, :] <= K_SPAN), span_y=span_y, span_x=span_x,
                live=(span_y[:, None] > 0) & (span_x[None, :] > 0), rows=sy, cols=sx)


# ---------------------------------------------------------------------------------------------------------------- the case table
FRAMES = {"A": (37, 53), "B": (48, 64), "wide": (24, 300)}  # H x W, two frames each
N_FRAMES = 2


def make_frames(name, seed=0):
    """``[2, 4, H, W]`` float32: colour in [0, 1), depth in [0.3, 1.3) with rectangular holes (depth = 0).  Rectangles, and
    not scattered pixels: the interpolated validity mask is then 1 or well below 0.99 almost everywhere, and both outcomes of the
    rule occur at every bin size of the table."""
    H, W = FRAMES[name]
    rs = np.random.RandomState(seed + sum(map(ord, name)))
    img = rs.rand(N_FRAMES, 4, H, W).astype(F)
    img[:, 3] += F(0.3)
    for b in range(N_FRAMES):
        for k in range(2):  # two vertical bands and a horizontal one over the left half, shifted per frame
            x0 = ((2 * k + 1) * W) // 5 + (b * W) // 11
            img[b, 3, :, x0:x0 + max(W // 12, 2)] = 0.0
        y0 = H // 3 + 2 * b
        img[b, 3, y0:y0 + max(H // 10, 2), :W // 2] = 0.0
    return img


class Case:
    """One row of the table: a box on a frame at an output size, and the mix of paths it is named for at sampling ratio 4.
    ``expect``: ``separable`` (every tile), ``slow`` (every tile), ``slow_x`` / ``slow_y`` (every tile slow because of that axis
    alone), ``mixed_empty`` (a slow tile beside a separable tile without a valid sample), ``mixed_live`` (beside a separable tile
    with valid samples), ``outside`` (no valid sample anywhere).  ``spans``: the (min, max) over live output columns that the
    case is built to reach, or None.  ``ratios``: run at sampling ratios 1-4 (cases 1-5 of the table).  ``depth_mix``: both
    outcomes of the validity rule occur on at least 5 % of the pixels each."""

    def __init__(self, name, frame, out_size, box, expect, spans=None, ratios=False, depth_mix=True, im_id=1, fused=None):
        self.name, self.frame, self.out_size, self.box = name, frame, out_size, np.array(box, F)
        self.expect, self.spans, self.ratios, self.depth_mix, self.im_id = expect, spans, ratios, depth_mix, im_id
        self.fused = fused  # the fused render + crop kernel runs the case too: what to expect of its tiles (band_tile)

    def __repr__(self):
        return self.name


def band_tile(out_size):
    """The tile of the fused kernel: a band of whole output rows of at most 3200 pixels (raster.hip kBandPixels), one decision
    between the two paths per band."""
    return (min(3200 // out_size[1], out_size[0]), out_size[1])


def check_paths(case, g=4, tile=TILE, expect=None):
    """Assert that ``case`` reaches the paths it is named for (``expect``: one name or several); returns ``tile_paths``."""
    expect = case.expect if expect is None else expect
    if not isinstance(expect, str):
        for e in expect:
            t = check_paths(case, g, tile, e)
        return t
    t = tile_paths(case.box, case.out_size, FRAMES[case.frame], g, tile)
    sep, live = t["separable"], t["live"]
    e = expect
    if e == "separable":
        assert sep.all() and live.any(), (case, t)
    elif e == "slow":
        assert not sep.any() and (t["span_y"] > K_SPAN).all() and (t["span_x"] > K_SPAN).all(), (case, t)
    elif e == "slow_x":
        assert not sep.any() and (t["span_y"] <= K_SPAN).all() and (t["span_y"] > 0).all(), (case, t)
    elif e == "slow_y":
        assert not sep.any() and (t["span_x"] <= K_SPAN).all() and (t["span_x"] > 0).all(), (case, t)
    elif e == "mixed_empty":
        assert (~sep).any() and (sep & ~live).any(), (case, t)
    elif e == "mixed_live":
        assert (~sep).any() and (sep & live).any(), (case, t)
    elif e == "outside":
        assert sep.all() and not live.any(), (case, t)
    else:
        raise AssertionError(e)
    if case.spans is not None and g == 4:
        cols = t["cols"][t["cols"] > 0]
        assert (cols.min(), cols.max()) == case.spans, (case, cols.min(), cols.max())
    return t


CASES = [
    # 1-5: the bin sizes, also run at sampling ratios 1-3 (3b: the widest fold the separable path holds)
    Case("up_bin0.2", "A", (33, 70), (10.3, 8.2, 24.3, 14.8), "separable", spans=(2, 3), ratios=True),
    Case("unit_frame", "B", (48, 64), (0, 0, 64, 48), "separable", spans=(1, 2), ratios=True),
    Case("bin2.6", "wide", (5, 70), (20.4, 2.3, 202.4, 15.3), "separable", spans=(4, 4), ratios=True, fused="separable"),
    Case("bin3.6_full_fold", "wide", (5, 70), (20.4, 2.3, 272.4, 20.3), "separable", spans=(4, 5), ratios=True),
    Case("bin4.4_alternating", "wide", (5, 64), (7.3, 1.1, 288.9, 23.1), "slow", spans=(5, 6), ratios=True, fused="slow"),
    Case("bin6.6_slow", "B", (7, 9), (2.3, 0.9, 61.7, 47.1), "slow", ratios=True, fused="slow"),
    # 6: one axis slow, the other separable
    Case("slow_x_only", "wide", (24, 32), (10.5, 3.2, 222.0, 20.0), "slow_x"),
    Case("slow_y_only", "B", (5, 3), (20.2, 3.5, 23.9, 44.5), "slow_y"),
    # 7: tiles that disagree inside one crop
    Case("mixed_empty_left", "A", (24, 80), (-300, 4.2, 53, 30.6), "mixed_empty"),
    Case("mixed_empty_top", "A", (64, 32), (8.1, -300, 40.3, 37), "mixed_empty"),
    Case("mixed_live_wide", "wide", (24, 128), (1.35, 2.0, 515.91, 21.5), "mixed_live"),
    # the same for the bands of the fused kernel (25 rows at 128 columns): band 0 separable with valid samples, band 1 slow, band 2 empty
    Case("mixed_bands", "B", (64, 128), (2.3, -92.15, 60.7, 165.13), "mixed_live", fused=("mixed_live", "mixed_empty")),
    # 8: wholly outside, one per side
    Case("outside_left", "A", (24, 32), (-40, 5, -2, 30), "outside", depth_mix=False),
    Case("outside_right", "A", (24, 32), (54.5, 5, 90, 30), "outside", depth_mix=False),
    Case("outside_top", "A", (24, 32), (5, -50, 40, -1.5), "outside", depth_mix=False),
    Case("outside_bottom", "A", (24, 32), (5, 38.5, 40, 80), "outside", depth_mix=False),
    # 9: width and height below 1: the clamp to 1 (placed across the edge of a hole)
    Case("degenerate", "A", (24, 32), (8.6, 3.0, 9.1, 3.2), "separable", im_id=0),
    # 10: first and last samples exactly on the rules (power-of-two bins: the float32 coordinates are exact).  bin = 2, g = 4:
    # samples at x1 + 0.25 + 0.5 k.  x1 = -1.25 puts the first on -1 (kept, clamped to 0), the next on -0.5, 0; 32 columns
    # end at x1 + 64 - 0.25 = 62.5.  Rows: y1 = -1.75 puts the first on -1.5 (dropped) and the second on -1 (kept).
    Case("edge_low", "B", (24, 32), (-1.25, -1.75, 62.75, 46.25), "separable"),
    # last samples on size-1 (collapse) and size (kept): 32 columns of bin 2 from x1 = 0.25: the last column samples 62.5, 63, 63.5,
    # 64 (W = 64); rows from y1 = 0.75: the last row samples 47 (H - 1), 47.5, 48 (H), 48.5 (dropped)
    Case("edge_high", "B", (24, 32), (0.25, 0.75, 64.25, 48.75), "separable"),
    # the same two upper rules on the literal path: bin 8, samples at x1 + 8 p + 1, 3, 5, 7; the last column samples 58, 60, 62 and
    # 64 (W: kept, collapsed onto W - 1), the last row 42, 44, 46 and 48 (H: kept)
    Case("edge_high_slow", "B", (5, 3), (41, 9, 65, 49), "slow", fused="slow"),
    Case("whole_tiles", "B", (64, 128), (-3.5, -2.25, 60.1, 50.3), "separable"),
]
CASE_BY_NAME = {c.name: c for c in CASES}
RATIO_CASES = [c for c in CASES if c.ratios]
DEPTH_CASES = [c for c in CASES if c.depth_mix]
FUSED_CASES = [c for c in CASES if c.fused]
# the six boxes of test_crop_vs_oracle (480 x 640) scaled by 1/10 to the 48 x 64 frame
ORACLE_BOXES = np.array([[10.03, 8.02, 42.07, 32.01], [-5, -4, 30, 22.25], [50, 40, 70, 55], [1, 1, 1.05, 1.02], [0, 0, 64, 48],
                         [30, 20, 34, 23]], F)
ORACLE_IDS = np.array([0, 1, 0, 1, 1, 0], np.int32)
