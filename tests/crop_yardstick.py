"""Yardsticks of the crop kernels' GPU tests: how far a float32 evaluation of the definition lies from the float64 reference
(tests/crop_ref.py).  Unlike the reference, this module knows the two orders in which the kernels add -- the literal
sampling_ratio^2-sample loop of ``slow_pixel`` and the fold of the separable path -- and that they do not contract a multiply and
an add (``fp contract(off)``).  Nothing here is compared with a kernel, it only sizes the bounds.  Every figure below is measured
and asserted by tests/test_crop_reference.py on the CPU; tests/test_gpu_crop_paths.py allows the kernels 4x: a kernel may
re-associate the sums, it may not lose digits."""

import numpy as np

import crop_ref as R

F = np.float32
SCALE_FLOOR = 1e-6   # floor of the scale S (the reference on |image|): pixels without a valid sample have S = 0 and error 0
Z_VALUES = np.array([0.7, 0.2, 2.8, -1.5], F)  # depth_norm_z per crop: 0.2 and -1.5 reach the clamps of mode 2 (2 and 0), -1.5 and 2.8 those of mode 3


def _axis_f32(start, bin_size, n, size, g):
    valid, lo, hi, l = R.axis_samples(start, bin_size, n, size, g)
    l = l.astype(F)  # exact: the coordinate and lo are float32
    return valid, lo, hi, l, F(1.0) - l


def literal_f32(planes, box, out_size, g):
    """``planes [C, H, W]`` float32 -> the sums of the samples ``[C, oh, ow]`` float32 in the order of ``slow_pixel``: per
    sample ``w1 v00 + w2 v01 + w3 v10 + w4 v11`` from the left, added to the accumulator, rows of samples outside, columns inside."""
    planes = np.asarray(planes, F)
    _, H, W = planes.shape
    x1, y1, bin_w, bin_h = R.box_bins(box, out_size)
    vy, ylo, yhi, ly, hy = _axis_f32(y1, bin_h, out_size[0], H, g)
    vx, xlo, xhi, lx, hx = _axis_f32(x1, bin_w, out_size[1], W, g)
    acc = np.zeros((planes.shape[0],) + tuple(out_size), F)
    for iy in range(g):
        for ix in range(g):
            yl, yh, xl, xh = ylo[:, iy][:, None], yhi[:, iy][:, None], xlo[:, ix][None, :], xhi[:, ix][None, :]
            a, b = hy[:, iy][:, None], ly[:, iy][:, None]
            c, d = hx[:, ix][None, :], lx[:, ix][None, :]
            val = (((a * c) * planes[:, yl, xl] + (a * d) * planes[:, yl, xh]) + (b * c) * planes[:, yh, xl]) + (b * d) * planes[:, yh, xh]
            assert val.dtype == F
            acc = acc + np.where(vy[:, iy][:, None] & vx[:, ix][None, :], val, F(0))
    return acc


def _fold_f32(start, bin_size, n, size, g):
    """Dense ``[n, size]`` float32 weights of one axis: per source index the weights of the valid samples added in sample order,
    lower neighbour before upper (``fold_axis``).  Adding the zeros of the other indices changes nothing."""
    valid, lo, hi, l, h = _axis_f32(start, bin_size, n, size, g)
    w = np.zeros((n, size), F)
    rows = np.arange(n)
    for s in range(g):
        np.add.at(w, (rows, lo[:, s]), np.where(valid[:, s], h[:, s], F(0)))
        np.add.at(w, (rows, hi[:, s]), np.where(valid[:, s], l[:, s], F(0)))
    return w


def folded_f32(planes, box, out_size, g):
    """The same sums in the order of the separable path: per source row the columns from the left (``racc += wx v``), then the
    rows from the top (``acc += wy racc``), all float32, no fused multiply-add."""
    planes = np.asarray(planes, F)
    _, H, W = planes.shape
    x1, y1, bin_w, bin_h = R.box_bins(box, out_size)
    wy = _fold_f32(y1, bin_h, out_size[0], H, g)   # [oh, H]
    wx = _fold_f32(x1, bin_w, out_size[1], W, g)   # [ow, W]
    racc = np.zeros((planes.shape[0], H, out_size[1]), F)
    for c in range(W):
        racc = racc + wx[None, None, :, c] * planes[:, :, c][:, :, None]
    acc = np.zeros((planes.shape[0],) + tuple(out_size), F)
    for r in range(H):
        acc = acc + wy[None, :, r][:, :, None] * racc[:, r][:, None, :]
    assert acc.dtype == F
    return acc


def crop_f32(frame, box, out_size, g, z, mode, order):
    """One crop of a 4-channel ``frame [4, H, W]`` as a float32 evaluation: ``(colour [3, oh, ow], depth [oh, ow], mask [oh, ow])``,
    depth after the validity rule and depth mode ``mode`` with ``depth_norm_z = z``."""
    frame = np.asarray(frame, F)
    planes = np.concatenate([frame, (frame[3:4] > 0).astype(F)], 0)
    sums = (literal_f32 if order == "literal" else folded_f32)(planes, box, out_size, g)
    vals = sums / F(g * g)
    mask = vals[4]
    d = np.where(mask < F(0.99), F(0), vals[3])
    z = F(z)
    if mode == 1:
        d = d / z
    elif mode == 2:
        d = np.minimum(np.maximum(d / z, F(0)), F(2)) - F(1)
    elif mode == 3:
        d = np.minimum(np.maximum(d - z, F(-2)), F(2))
    assert d.dtype == F
    return vals[:3], d, mask


def depth_scale(S, z, mode):
    """The scale of the depth channel after ``mode``, from the scale ``S`` of the interpolated depth: the normalisation divides
    by ``z`` (1, 2) and adds a term of size 1 (2) or ``|z|`` (3), whose rounding the result carries."""
    z = abs(float(z))
    return {0: S, 1: S / z, 2: S / z + 1.0, 3: S + z}[mode]


def case_inputs(case):
    """The call of one case in the CPU and the GPU tests: the case's box four times, one ``depth_norm_z`` of ``Z_VALUES`` each,
    the third crop on the other frame."""
    boxes = np.tile(case.box[None], (4, 1))
    ids = np.array([case.im_id, case.im_id, 1 - case.im_id, case.im_id], np.int32)
    return boxes, ids, Z_VALUES.copy()


def scales(frames, boxes, ids, out_size, g):
    """``S``: the reference on ``|image|`` (colour ``[n, 3, oh, ow]`` and the unmasked depth ``[n, oh, ow]``), floored."""
    s = np.maximum(R.roi_align_ref(np.abs(frames), boxes, ids, out_size, g), SCALE_FLOOR)
    return s[:, :3], s[:, 3]


def band_of_mask():
    """Half-width of the exclusion band round 0.99: depth pixels whose float64 mask lies this close to the threshold may fall on
    either side in float32 and are not compared."""
    return 4 * MEASURED_F32_ERROR["mask"]


def measure(case, g, frames=None):
    """Worst ``|f32 - f64| / S`` of both float32 evaluations on one case: ``dict(colour, depth0..depth3, mask, near)``; ``near`` =
    share of depth pixels inside the exclusion band."""
    frames = R.make_frames(case.frame) if frames is None else frames
    boxes, ids, zs = case_inputs(case)
    worst = {k: 0.0 for k in ("colour", "depth0", "depth1", "depth2", "depth3", "mask")}
    s_col, s_dep = scales(frames, boxes, ids, case.out_size, g)
    near = 0.0
    for mode in range(4):
        ref, mask = R.crop_ref(frames, boxes, ids, case.out_size, g, depth_norm_z=zs, depth_norm_mode=mode)
        keep = np.abs(mask - R.VALID_THRESHOLD) > band_of_mask()
        near = max(near, 1.0 - keep.mean())
        for order in ("literal", "folded"):
            for i in range(len(boxes)):
                col, d, m = crop_f32(frames[ids[i]], boxes[i], case.out_size, g, zs[i], mode, order)
                worst["colour"] = max(worst["colour"], float((np.abs(col - ref[i, :3]) / s_col[i]).max()))
                worst["mask"] = max(worst["mask"], float(np.abs(m - mask[i]).max()))  # S of the mask is at most 1
                e = np.abs(d - ref[i, 3]) / depth_scale(s_dep[i], zs[i], mode)
                worst[f"depth{mode}"] = max(worst[f"depth{mode}"], float(e[keep[i]].max()) if keep[i].any() else 0.0)
    worst["near"] = near
    return worst


# Worst |f32 - f64| / S over every case of crop_ref.CASES (cases with ``ratios`` at sampling ratios 1-4, the others at 4), both
# orders of summation; ``mask`` is the absolute error of the interpolated validity mask, whose scale is at most 1.
MEASURED_F32_ERROR = {"colour": 3.04e-7, "depth0": 2.72e-7, "depth1": 3.19e-7, "depth2": 1.46e-7, "depth3": 2.07e-7, "mask": 1.2e-7}
