"""The crop kernels path by path against the float64 reference (tests/crop_ref.py): the stand-alone kernel of crop.hip and the
crop of the fused render + crop kernel (raster.hip), on the case table of crop_ref -- both paths (separable fold, literal
samples), tiles that disagree inside one crop, partial tiles, sampling ratios 1-4, depth modes 0-3, every destination layout.
Needs a real MI355X: ``pytest -m gpu``.

Stated tolerances (none is a literal here):
* fp32 outputs: ``|got - ref| <= 4 x e x S`` per pixel, ``S`` the reference on |image| (for depth after a mode:
  crop_yardstick.depth_scale), ``e`` = crop_yardstick.MEASURED_F32_ERROR, the error of a float32 evaluation of the definition in the
  kernels' two orders of summation, re-measured on the CPU by tests/test_crop_reference.py;
* depth is not compared where the float64 validity mask lies within 4 x e_mask of 0.99 (either outcome of the rule is a correct
  float32 answer there): at most 0.5 % of the pixels of a case (the table has none);
* fp16 destinations: the fp32 kernel's output rounded once, bit for bit.
Every case first proves with crop_ref.tile_paths that it reaches the path it is named after."""

import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import crop_ref as R  # noqa: E402
import crop_yardstick as Y  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
WORST = {}  # (kernel, path, quantity) -> worst |got - ref| / (e x S) seen, printed by the tests


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scene_store(dev):
    from happypose_amd.ops import MeshStore
    from happypose_amd.synthetic import make_object_dataset

    return MeshStore(make_object_dataset(3, seed=1, tex_size=256), dev)


@functools.lru_cache(maxsize=None)
def _frames(name):
    f = R.make_frames(name)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _reference(name, g, tile):
    """Everything a comparison needs, computed once per (case, sampling ratio, tile shape) and left unchanged."""
    case = R.CASE_BY_NAME[name]
    frames = _frames(case.frame)
    boxes, ids, zs = Y.case_inputs(case)
    s_col, s_dep = Y.scales(frames, boxes, ids, case.out_size, g)
    refs = {m: R.crop_ref(frames, boxes, ids, case.out_size, g, depth_norm_z=zs, depth_norm_mode=m) for m in range(4)}
    mask = refs[0][1]
    keep = np.abs(mask - R.VALID_THRESHOLD) > Y.band_of_mask()
    assert 1.0 - keep.mean() <= 0.005
    t = R.tile_paths(case.box, case.out_size, R.FRAMES[case.frame], g, tile)
    oh, ow = case.out_size
    sep = np.repeat(np.repeat(t["separable"], tile[0], 0), tile[1], 1)[:oh, :ow]
    return dict(boxes=boxes, ids=ids, zs=zs, s_col=s_col, s_dep=s_dep, refs=refs, keep=keep, sep=sep, paths=t)


def _compare(kernel, got, ref, n_channels, mode, what):
    """``got [n, C, oh, ow]`` (numpy, fp32 kernel output) against the reference under the stated bounds."""
    got = got.astype(np.float64)
    want = ref["refs"][mode][0]
    e = Y.MEASURED_F32_ERROR
    ratio = np.abs(got[:, :3] - want[:, :3]) / (e["colour"] * ref["s_col"])
    checks = [("colour", ratio)]
    if n_channels == 4:
        scale = np.stack([Y.depth_scale(ref["s_dep"][i], ref["zs"][i], mode) for i in range(len(got))])
        rd = np.abs(got[:, 3] - want[:, 3]) / (e[f"depth{mode}"] * scale)
        checks.append((f"depth{mode}", np.where(ref["keep"], rd, 0.0)))
    for q, r in checks:
        for path, sel in (("separable", ref["sep"]), ("slow", ~ref["sep"])):
            if sel.any():
                key = (kernel, path, q)
                WORST[key] = max(WORST.get(key, 0.0), float(r[..., sel].max()))
        assert r.max() <= 4.0, (what, q, float(r.max()), "x the float32 yardstick; allowed 4")


def _cases_with_ratios():
    return [(c, g) for c in R.CASES for g in ((1, 2, 3, 4) if c.ratios else (4,))]


def _on(dev, ref, frames):
    return (torch.as_tensor(np.array(frames), device=dev), torch.as_tensor(ref["boxes"], device=dev),
            torch.as_tensor(ref["ids"], device=dev), torch.as_tensor(ref["zs"], device=dev))


# ------------------------------------------------------------------------------------------------------ the stand-alone kernel
@pytest.mark.parametrize("case,g", _cases_with_ratios(), ids=lambda v: repr(v))
def test_standalone_fp32_destinations(dev, case, g):
    """NCHW, NHWC records of 8 floats (plain and owned) and of 5 floats; C = 3, C = 4 and 3 channels of a 4-channel frame;
    depth modes 0-3 -- against the reference; what the crop does not own keeps the sentinel, what it owns is zero."""
    from happypose_amd import ops

    if g == 4:
        R.check_paths(case)
    ref = _reference(case.name, g, R.TILE)
    frames = _frames(case.frame)
    n, (oh, ow) = len(ref["boxes"]), case.out_size
    for C, nC in ((3, 3), (4, 3), (4, 4)):
        img, boxes, ids, zs = _on(dev, ref, frames[:, :C])
        for mode in ((0, 1, 2, 3) if nC == 4 else (0,)):
            kw = dict(sampling_ratio=g, depth_norm_z=zs if mode else None, depth_norm_mode=mode, n_channels=nC)
            what = (case.name, g, C, nC, mode)
            nchw = ops.crop_roi_align(img, boxes, ids, (oh, ow), **kw)
            assert nchw.shape == (n, nC, oh, ow)
            _compare("crop", nchw.cpu().numpy(), ref, nC, mode, what + ("nchw",))
            for rec, owns in ((8, False), (8, True), (5, False)):
                x = torch.full((n, oh, ow, rec), SENTINEL, device=dev)
                ops.crop_roi_align(img, boxes, ids, (oh, ow), out=x, owns_record=owns, **kw)
                assert torch.equal(x[..., :nC].permute(0, 3, 1, 2), nchw), what + (rec, owns)  # one kernel, one arithmetic
                assert bool((x[..., nC:] == (0.0 if owns else SENTINEL)).all()), what + (rec, owns)
    print({k: round(v, 3) for k, v in WORST.items() if k[0] == "crop"})


@pytest.mark.parametrize("case", [c for c in R.CASES if c.expect != "outside"] + [R.CASE_BY_NAME["outside_left"]], ids=repr)
def test_standalone_fp16_destinations(dev, case):
    """The sector store (16-half records, owned) and the strided store (24-half records): the fp32 kernel's values rounded once."""
    from happypose_amd import ops

    ref = _reference(case.name, 4, R.TILE)
    n, (oh, ow) = len(ref["boxes"]), case.out_size
    for C, nC, mode in ((3, 3, 0), (4, 3, 0), (4, 4, 0), (4, 4, 2), (4, 4, 3)):
        img, boxes, ids, zs = _on(dev, ref, _frames(case.frame)[:, :C])
        kw = dict(depth_norm_z=zs if mode else None, depth_norm_mode=mode, n_channels=nC)
        want = ops.crop_roi_align(img, boxes, ids, (oh, ow), **kw).permute(0, 2, 3, 1).half()
        for rec, owns in ((16, True), (16, False), (24, False), (24, True)):
            x = torch.full((n, oh, ow, rec), SENTINEL, device=dev, dtype=torch.float16)
            ops.crop_roi_align(img, boxes, ids, (oh, ow), out=x, owns_record=owns, **kw)
            assert torch.equal(x[..., :nC], want), (case.name, C, nC, mode, rec, owns)
            owned = owns and rec == 16  # a 24-half record is no whole number of sectors: the crop writes its channels only
            assert bool((x[..., nC:] == (0.0 if owned else SENTINEL)).all()), (case.name, C, nC, mode, rec, owns)


def test_standalone_bad_ids(dev):
    """Device-resident ids out of range (-1 and Bi): an all-zero crop, in every depth mode and layout; the other crops of the call
    are what they are without the bad ones; the call succeeds (``ops.check`` raises on any status but OK)."""
    from happypose_amd import ops

    frames = _frames("B")
    img = torch.as_tensor(np.array(frames), device=dev)
    host_boxes = np.array([SEPARABLE_BOX, SEPARABLE_BOX, [-40.5, -60.2, 120.3, 100.4], [-40.5, -60.2, 120.3, 100.4]], np.float32)
    assert R.tile_paths(host_boxes[0], (24, 32), R.FRAMES["B"], 4)["separable"].all()      # a fold
    assert not R.tile_paths(host_boxes[2], (24, 32), R.FRAMES["B"], 4)["separable"].any()  # and a literal crop
    boxes = torch.as_tensor(host_boxes, device=dev)
    good = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device=dev)
    bad = torch.tensor([-1, 0, R.N_FRAMES, 1], dtype=torch.int32, device=dev)
    zs = torch.as_tensor(Y.Z_VALUES, device=dev)
    with pytest.raises(IndexError):
        ops.crop_roi_align(img, boxes, bad.cpu(), (24, 32))  # host-resident ids are checked like the reference's indexing
    for mode in range(4):
        kw = dict(depth_norm_z=zs if mode else None, depth_norm_mode=mode)
        a, b = ops.crop_roi_align(img, boxes, good, (24, 32), **kw), ops.crop_roi_align(img, boxes, bad, (24, 32), **kw)
        assert float(b[0].abs().max()) == 0 and float(b[2].abs().max()) == 0
        assert torch.equal(a[[1, 3]], b[[1, 3]]) and float(a[0].abs().max()) > 0 and float(a[2].abs().max()) > 0
        for dt, rec in ((torch.float32, 8), (torch.float16, 16)):
            x = torch.full((4, 24, 32, rec), SENTINEL, device=dev, dtype=dt)
            ops.crop_roi_align(img, boxes, bad, (24, 32), out=x, owns_record=True, **kw)
            assert float(x[[0, 2]].abs().max()) == 0
            assert torch.equal(x[[1, 3]][..., :4].float(), a[[1, 3]].permute(0, 2, 3, 1).to(dt).float())


# ------------------------------------------------------------------------------------------------------------- the fused kernel
def _render_args(dev, n, out_size, V=1):
    """The smallest scene that puts an object in view: the camera looks down the axis at 0.3 m, focal length twice the longer side."""
    from happypose_amd.synthetic import random_rotations

    h, w = out_size
    rs = np.random.RandomState(7)
    T = np.tile(np.eye(4, dtype=np.float32), (n * V, 1, 1))
    T[:, :3, :3] = random_rotations(rs, n * V)
    T[:, 2, 3] = 0.3
    f = 2.0 * max(h, w)
    K = np.tile(np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], np.float32), (n * V, 1, 1))
    obj = torch.as_tensor((np.arange(n) % 3).astype(np.int32), device=dev)
    return obj, torch.as_tensor(T.reshape(n, V, 4, 4), device=dev), torch.as_tensor(K.reshape(n, V, 3, 3), device=dev)


SEPARABLE_BOX = np.array([10.3, 8.2, 24.3, 14.8], np.float32)  # inside frame B: bin 0.44 at 24 x 32


@pytest.mark.parametrize("case", R.FUSED_CASES, ids=repr)
def test_fused_crop_channels(dev, scene_store, case):
    """``hp_render_inputs``: the crop channels of the records against the reference, 3 and 4 crop channels, fp32 records and
    fp16 records (16 halves: one view owns the record; 24 halves: it does not) = the fp32 values rounded once; the rendered
    channels are there and are the same as with a separable box in place of the case's."""
    from happypose_amd import ops

    tile = R.band_tile(case.out_size)
    R.check_paths(case, 4, tile, case.fused)
    ref = _reference(case.name, 4, tile)
    n, (oh, ow) = len(ref["boxes"]), case.out_size
    sep_box = np.array([10.3, 8.2, 10.3 + 0.25 * ow, 8.2 + 0.25 * oh], np.float32)  # bin 0.25: a fold at every output size
    t_sep = R.tile_paths(sep_box, case.out_size, R.FRAMES[case.frame], 4, tile)
    assert t_sep["separable"].all() and t_sep["live"].any()
    obj, T, K = _render_args(dev, n, case.out_size)
    sep_boxes = torch.as_tensor(np.tile(sep_box[None], (n, 1)), device=dev)
    for C, nC, mode in ((3, 3, 0), (4, 3, 0), (4, 4, 0), (4, 4, 1), (4, 4, 2), (4, 4, 3)):
        img, boxes, ids, zs = _on(dev, ref, _frames(case.frame)[:, :C])
        kw = dict(images=img, im_ids=ids, n_img_channels=nC, depth_norm_z=zs if mode else None, depth_norm_mode=mode)
        out = {}
        for dt, rec in ((torch.float32, 8), (torch.float16, 16), (torch.float16, 24)):
            x = torch.full((n, oh, ow, rec), SENTINEL, device=dev, dtype=dt)
            ops.render_inputs(scene_store, x, obj, T, K, False, False, boxes=boxes, **kw)
            y = torch.full((n, oh, ow, rec), SENTINEL, device=dev, dtype=dt)
            ops.render_inputs(scene_store, y, obj, T, K, False, False, boxes=sep_boxes, **kw)
            what = (case.name, C, nC, mode, str(dt), rec)
            assert float(x[..., nC:nC + 3].abs().sum()) > 0, what
            assert torch.equal(x[..., nC:], y[..., nC:]), what  # renders and pads do not depend on the crop box or its path
            assert not torch.equal(x[..., :nC], y[..., :nC]), what
            out[(dt, rec)] = x
        x32 = out[(torch.float32, 8)]
        _compare("fused", x32[..., :nC].permute(0, 3, 1, 2).cpu().numpy(), ref, nC, mode, (case.name, C, nC, mode))
        assert bool((x32[..., nC + 3:] == SENTINEL).all())
        for rec in (16, 24):
            assert torch.equal(out[(torch.float16, rec)][..., :nC + 3], x32[..., :nC + 3].half()), (case.name, C, nC, mode, rec)
    print({k: round(v, 3) for k, v in WORST.items() if k[0] == "fused"})


@pytest.mark.parametrize("case", R.FUSED_CASES, ids=repr)
def test_fused_permuted_layout(dev, scene_store, case):
    """Two views, view 0 carries 1 crop channel (the depth plane: validity rule and mode) and view 1 two (red, green): the
    1- and 2-channel fold and their literal counterpart, fp32 and fp16 records."""
    from happypose_amd import ops

    tile = R.band_tile(case.out_size)
    R.check_paths(case, 4, tile, case.fused)
    ref = _reference(case.name, 4, tile)
    n, (oh, ow) = len(ref["boxes"]), case.out_size
    obj, T, K = _render_args(dev, n, case.out_size, V=2)
    img, boxes, ids, zs = _on(dev, ref, _frames(case.frame))
    layout = ([0, 8], [3, 11], [3, 0], [1, 2])  # view_c0, crop_c0, crop_src0, crop_n
    for mode in (0, 2):
        out = {}
        for dt in (torch.float32, torch.float16):
            x = torch.full((n, oh, ow, 16), SENTINEL, device=dev, dtype=dt)
            ops.render_inputs(scene_store, x, obj, T, K, False, False, images=img, boxes=boxes, im_ids=ids, n_img_channels=4,
                              depth_norm_z=zs if mode else None, depth_norm_mode=mode, layout=layout)
            out[dt] = x
        x = out[torch.float32]
        got = torch.stack([x[..., 11], x[..., 12], x[..., 12], x[..., 3]], 1).cpu().numpy()  # blue is not cropped: green twice
        want = dict(ref, refs={mode: (ref["refs"][mode][0][:, [0, 1, 1, 3]], None)}, s_col=ref["s_col"][:, [0, 1, 1]])
        _compare("fused", got, want, 4, mode, (case.name, "permuted", mode))
        assert float(x[..., 0:3].abs().sum()) > 0 and float(x[..., 8:11].abs().sum()) > 0
        untouched = [4, 5, 6, 7, 13, 14, 15]
        assert bool((x[..., untouched] == SENTINEL).all())
        written = [0, 1, 2, 3, 8, 9, 10, 11, 12]
        assert torch.equal(out[torch.float16][..., written], x[..., written].half())
