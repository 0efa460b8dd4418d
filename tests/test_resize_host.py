"""Host-side checks of the resize layer without a GPU: argument errors of hp_resize_* / hp_seg_boxes and of their wrappers, the
no-op path of CropResizeToAspectTransform, and batches without K or object_ids through every transform."""

import dataclasses

import numpy as np
import pytest
import torch

from happypose_amd import _ffi
from happypose_amd import augmentations as A
from happypose_amd import ops

P = 4096  # stands for a device pointer: an argument error is reported before anything is dereferenced


def _rgb(lib, B=2, ih=8, iw=8, oh=4, ow=4, d_in=P, tab=P, n_tables=1, ksx=3, band=8, ksy=3, apply=P, out=2 * P, ws=P, ws_bytes=1 << 40, xb=P, yb=P):
    return lib.hp_resize_rgb(B, ih, iw, oh, ow, d_in, n_tables, tab, xb, P, ksx, band, yb, P, ksy, apply, out, ws, ws_bytes, None)


def test_resize_rgb_argument_errors_without_gpu():
    lib = _ffi.lib()
    for kw in (dict(B=-1), dict(ih=0), dict(iw=-2), dict(oh=0), dict(ow=0), dict(B=70000), dict(ih=1 << 15, iw=1 << 15), dict(oh=70000),
               dict(d_in=None), dict(tab=None), dict(apply=None), dict(out=None), dict(out=P), dict(n_tables=0), dict(n_tables=3),
               dict(ksx=-1), dict(ksy=5000), dict(xb=None), dict(yb=None), dict(band=0), dict(band=12289), dict(ksx=0), dict(ksy=0),
               dict(ws=None), dict(ws_bytes=2 * 8 * 4 * 3 - 1)):
        assert _rgb(lib, **kw) == -1 and b"hp_resize_rgb" in lib.hp_last_error(), kw
    assert _rgb(lib, B=0, d_in=None) == 0  # B == 0: HP_OK, nothing launched, no pointer looked at
    assert lib.hp_resize_workspace_bytes(2, 8, 4) == 192 and lib.hp_resize_workspace_bytes(1, 3, 3) == 32
    for bad in ((-1, 8, 4), (2, 0, 4), (2, 8, 0), (70000, 8, 4), (1, 1 << 15, 1 << 15)):
        assert lib.hp_resize_workspace_bytes(*bad) == -1


def test_resize_nearest_and_seg_boxes_argument_errors_without_gpu():
    lib = _ffi.lib()

    def nearest(B=2, ih=8, iw=8, oh=4, ow=4, d_in=P, tab=P, n_tables=1, xi=P, yi=P, apply=P, out=2 * P):
        return lib.hp_resize_nearest(B, ih, iw, oh, ow, d_in, n_tables, tab, xi, yi, apply, out, None)

    for kw in (dict(B=-1), dict(ih=0), dict(ow=-1), dict(B=70000), dict(oh=70000), dict(d_in=None), dict(tab=None), dict(xi=None),
               dict(yi=None), dict(apply=None), dict(out=None), dict(out=P), dict(n_tables=0), dict(n_tables=3)):
        assert nearest(**kw) == -1 and b"hp_resize_nearest" in lib.hp_last_error(), kw
    assert nearest(B=0, d_in=None) == 0

    def boxes(B=2, h=8, w=8, seg=P, ids=P, count=P, max_ids=4, out=P, n_px=P):
        return lib.hp_seg_boxes(B, h, w, seg, ids, count, max_ids, out, n_px, None)

    for kw in (dict(B=-1), dict(h=0), dict(w=0), dict(B=70000), dict(h=1 << 15, w=1 << 15), dict(seg=None), dict(ids=None), dict(count=None),
               dict(out=None), dict(n_px=None), dict(max_ids=0), dict(max_ids=257)):
        assert boxes(**kw) == -1 and b"hp_seg_boxes" in lib.hp_last_error(), kw
    assert boxes(B=0, seg=None) == 0


def test_wrappers_refuse_cpu_tensors_and_wrong_types():
    rgb, depth, seg = torch.zeros(2, 4, 5, 3, dtype=torch.uint8), torch.zeros(2, 4, 5), torch.zeros(2, 4, 5, dtype=torch.int32)
    for call in (lambda: ops.resize_rgb(rgb, (2, 2)), lambda: ops.resize_nearest(depth, (2, 2)), lambda: ops.resize_nearest(seg, (2, 2)),
                 lambda: ops.seg_boxes(seg, [[1], [2]]), lambda: ops.resize_rgb(rgb.numpy(), (2, 2))):
        with pytest.raises(ValueError, match="device"):
            call()


def test_table_argument_errors():
    for kw in (dict(filter="lanczos"), dict(box=(0, 0, 6, 4)), dict(box=(2, 0, 2, 4)), dict(box=(-1, 0, 3, 4)), dict(crop=(3, 0, 3, 4)),
               dict(out_size=(0, 2))):
        with pytest.raises(ValueError):
            ops.resize_tables(**{"in_size": (4, 5), "out_size": (2, 2), **kw})
    # a box is in the pixels of the CROPPED image
    assert ops.resize_tables((4, 5), (2, 2), box=(0, 0, 7, 6), crop=(-1, -1, 6, 5))["xbounds"][0, 0] == -1
    with pytest.raises(ValueError):
        ops._resize_rects(np.zeros((3, 4)), 2, "box")
    with pytest.raises(ValueError):
        ops._resize_rects([0.5, 0, 2, 2], 1, "box")
    sets, table_of = ops._resize_sets(3, [[0, 0, 2, 2], [0, 0, 3, 3], [0, 0, 2, 2]], None, "t")
    assert sets == [((0, 0, 2, 2), None), ((0, 0, 3, 3), None)] and list(table_of) == [0, 1, 0]
    table, count = ops.seg_boxes_table([[3, 5, 9], [], [1]], 3)
    assert table.tolist() == [[3, 5, 9], [0, 0, 0], [1, 0, 0]] and count.tolist() == [3, 0, 1]
    with pytest.raises(ValueError):
        ops.seg_boxes_table([[1]], 2)
    with pytest.raises(ValueError):
        ops.seg_boxes_table([[2 ** 31]], 1)


def test_crop_resize_asserts_and_no_op():
    with pytest.raises(AssertionError):
        A.CropResizeToAspectTransform((640, 480))
    T = A.CropResizeToAspectTransform()
    assert T.resize == (480, 640) and T.aspect == 640 / 480
    # frames that already have the size: the batch comes back as it is, nothing is launched (these tensors are on the host)
    batch = A.ObservationBatch(rgb=torch.zeros(2, 24, 32, 3, dtype=torch.uint8), segmentation=torch.zeros(2, 24, 32, dtype=torch.int32),
                               K=torch.eye(3).repeat(2, 1, 1), object_ids=[[1], [2]])
    T = A.CropResizeToAspectTransform((24, 32))
    assert T(batch, np.random.default_rng(0)) is batch
    assert A.SceneObservationAugmentation(T, p=1.0)(batch, np.random.default_rng(0)) is batch
    with pytest.raises(AssertionError):
        T(A.ObservationBatch(rgb=batch.rgb), np.random.default_rng(0))  # the reference asserts a segmentation
    with pytest.raises(ValueError, match="every image"):
        T.apply(batch, {}, np.array([True, False]))
    with pytest.raises(ValueError, match="device"):  # another size: the kernels are needed, and there is no host implementation
        A.CropResizeToAspectTransform((12, 16))(batch, np.random.default_rng(0))


ALL = [A.PillowBlur, A.PillowSharpness, A.PillowContrast, A.PillowBrightness, A.PillowColor, A.DepthGaussianNoiseTransform,
       A.DepthCorrelatedGaussianNoiseTransform, A.DepthMissingTransform, A.DepthDropoutTransform, A.DepthEllipseDropoutTransform,
       A.DepthEllipseNoiseTransform, A.DepthBlurTransform, A.DepthBackgroundDropoutTransform, A.ReplaceBackgroundTransform]


def test_batches_without_K_or_object_ids_run_every_existing_transform(monkeypatch):
    """The new fields are optional and ride along: every transform of before takes a batch built the old way (four positional
    tensors), hands its kernel wrapper the same arguments as before and returns a batch whose new fields are still None."""
    fields = [f.name for f in dataclasses.fields(A.ObservationBatch)]
    assert fields[:4] == ["rgb", "depth", "segmentation", "background"] and set(fields[4:]) == {"K", "object_ids", "boxes_modal", "visible"}
    rgb, depth, seg = torch.zeros(2, 4, 5, 3, dtype=torch.uint8), torch.ones(2, 4, 5), torch.zeros(2, 4, 5, dtype=torch.int32)
    batch = A.ObservationBatch(rgb, depth, seg, rgb.clone())
    assert batch.K is None and batch.object_ids is None and batch.boxes_modal is None and batch.visible is None and batch.batch_size == 2
    called = []
    for name in ("aug_rgb_enhance", "aug_rgb_blur", "aug_replace_background", "aug_depth_noise", "aug_depth_missing", "aug_depth_ellipses",
                 "aug_depth_blur", "aug_depth_mask"):
        monkeypatch.setattr(ops, name, lambda x, *a, _n=name, **k: called.append(_n) or x)
    monkeypatch.setattr(ops, "resize_rgb", lambda *a, **k: pytest.fail("no resize was asked for"))
    for cls in ALL:
        out = cls()(batch, np.random.default_rng(0))
        assert (out.K, out.object_ids, out.boxes_modal, out.visible) == (None, None, None, None), cls.__name__
        assert out.rgb is rgb and out.depth is depth and out.segmentation is seg
    assert len(called) == len(ALL)
    assert A.ReplaceBackgroundTransform().resize_background is False and A.make_background_augmentations()[0].transform.resize_background is False
    # with K and object_ids the fields ride along unchanged
    with_k = dataclasses.replace(batch, K=torch.eye(3).repeat(2, 1, 1), object_ids=[[1], [2]])
    out = A.PillowColor()(with_k, np.random.default_rng(0))
    assert out.K is with_k.K and out.object_ids is with_k.object_ids
