"""Training-image augmentations on the device: the transforms of the reference's ``toolbox/datasets/augmentations.py`` with its
class names, arguments, defaults and order, applied to a whole batch of frames that already lives on the GPU
(``csrc/augment.hip``; every formula is in ``include/happypose_amd.h``).

A transform has two halves.  ``draw(batch_size, rng)`` runs on the host and returns the small per-image parameters (factors,
radii, ellipse tables, a 64-bit seed for the per-pixel streams) from a ``numpy.random.Generator``; ``apply(batch, params)`` runs
the kernels.  ``__call__(batch, rng)`` does both.  ``SceneObservationAugmentation(transform | list, p)`` adds the per-image
``apply`` flags: an image is transformed with probability ``p``, and only if every enclosing augmentation applied as well.

The RGB transforms equal Pillow byte for byte.  The depth transforms restate the reference's OpenCV calls (parity unpinned).
The reference's random STREAMS are not reproduced: they come from the global ``random`` / ``np.random`` state.

``CropResizeToAspectTransform`` is the one transform that changes a frame's geometry (``csrc/resize.hip``): it equals Pillow's
``crop`` and ``resize`` byte for byte, rewrites ``K`` and recomputes the modal boxes from the resized id map.  Out of scope:
loading VOC -- the background frames come with the batch (``ReplaceBackgroundTransform(resize_background=True)`` resizes them).
"""

from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops


@dataclasses.dataclass
class ObservationBatch:
    """``rgb [B, H, W, 3]`` uint8, ``depth [B, H, W]`` float32 (metres, 0 = invalid), ``segmentation [B, H, W]`` int32 (0 =
    background: ``SceneRenderer``'s ``ids + 1``), ``background [B, H, W, 3]`` uint8 (``[B, H', W', 3]`` with
    ``ReplaceBackgroundTransform(resize_background=True)``); all dense, on the device.  Optional, for
    ``CropResizeToAspectTransform``: ``K [B, 3, 3]`` (any device) and ``object_ids``, one list of unique ids per image -- the
    transform then fills ``boxes_modal [B, max_ids, 4]`` int32 ``(x1, y1, x2, y2)``, inclusive, and ``visible [B, max_ids]``
    bool, slot ``k`` of image ``b`` for ``object_ids[b][k]`` (a slot that is not visible has an unspecified box)."""

    rgb: Optional[torch.Tensor] = None
    depth: Optional[torch.Tensor] = None
    segmentation: Optional[torch.Tensor] = None
    background: Optional[torch.Tensor] = None
    K: Optional[torch.Tensor] = None
    object_ids: Optional[Sequence[Sequence[int]]] = None
    boxes_modal: Optional[torch.Tensor] = None
    visible: Optional[torch.Tensor] = None

    @property
    def batch_size(self) -> int:
        for t in (self.rgb, self.depth, self.segmentation):
            if t is not None:
                return int(t.shape[0])
        raise ValueError("ObservationBatch: empty")


Params = Dict[str, np.ndarray]


def _all(batch_size: int) -> np.ndarray:
    return np.ones(batch_size, bool)


def _seed(rng: np.random.Generator) -> np.ndarray:
    return rng.integers(0, 2 ** 64, size=1, dtype=np.uint64)


class SceneObservationTransform:
    def draw(self, batch_size: int, rng: np.random.Generator) -> Params:
        return {}

    def apply(self, batch: ObservationBatch, params: Params, apply: Optional[np.ndarray] = None) -> ObservationBatch:
        raise NotImplementedError

    def __call__(self, batch: ObservationBatch, rng: np.random.Generator) -> ObservationBatch:
        return self.apply(batch, self.draw(batch.batch_size, rng))


class SceneObservationAugmentation(SceneObservationTransform):
    """The reference's wrapper: ``transform`` (one transform, or a list of augmentations applied in order) with probability
    ``p`` per image.  ``draw`` returns ``{"apply": [B] bool, "inner": params | [params]}``; a nested augmentation's flags are
    combined (and) with those of everything around it."""

    def __init__(self, transform: Union[SceneObservationTransform, List["SceneObservationAugmentation"]], p: float = 1.0):
        self.p = p
        self.transform = transform

    def draw(self, batch_size: int, rng: np.random.Generator) -> dict:
        flags = rng.random(batch_size) <= self.p
        if isinstance(self.transform, list):
            inner = [t.draw(batch_size, rng) for t in self.transform]
        else:
            inner = self.transform.draw(batch_size, rng)
        return {"apply": flags, "inner": inner}

    def apply(self, batch: ObservationBatch, params: dict, apply: Optional[np.ndarray] = None) -> ObservationBatch:
        flags = np.asarray(params["apply"], bool)
        if apply is not None:
            flags = flags & np.asarray(apply, bool)
        if isinstance(self.transform, list):
            for t, p in zip(self.transform, params["inner"]):
                batch = t.apply(batch, p, flags)
        else:
            batch = self.transform.apply(batch, params["inner"], flags)
        return batch


# ---- RGB ----------------------------------------------------------------------------------------------------------------------------
class PillowRGBTransform(SceneObservationTransform):
    op = ""

    def __init__(self, factor_interval: Tuple[float, float]):
        self.factor_interval = factor_interval

    def draw(self, batch_size: int, rng: np.random.Generator) -> Params:
        lo, hi = self.factor_interval
        return {"factor": rng.uniform(lo, hi, size=batch_size).astype(np.float32)}

    def apply(self, batch, params, apply=None):
        assert batch.rgb is not None
        flags = _all(batch.batch_size) if apply is None else apply
        return dataclasses.replace(batch, rgb=ops.aug_rgb_enhance(batch.rgb, self.op, params["factor"], flags))


class PillowSharpness(PillowRGBTransform):
    op = "sharpness"

    def __init__(self, factor_interval: Tuple[float, float] = (0.0, 50.0)):
        super().__init__(factor_interval)


class PillowContrast(PillowRGBTransform):
    op = "contrast"

    def __init__(self, factor_interval: Tuple[float, float] = (0.2, 50.0)):
        super().__init__(factor_interval)


class PillowBrightness(PillowRGBTransform):
    op = "brightness"

    def __init__(self, factor_interval: Tuple[float, float] = (0.1, 6.0)):
        super().__init__(factor_interval)


class PillowColor(PillowRGBTransform):
    op = "color"

    def __init__(self, factor_interval: Tuple[float, float] = (0, 20.0)):
        super().__init__(factor_interval)


class PillowBlur(SceneObservationTransform):
    """``ImageFilter.GaussianBlur(k)``, ``k`` an integer of ``factor_interval`` (both ends included)."""

    def __init__(self, factor_interval: Tuple[int, int] = (1, 3)):
        self.factor_interval = factor_interval

    def draw(self, batch_size, rng):
        lo, hi = self.factor_interval
        return {"k": rng.integers(lo, hi + 1, size=batch_size).astype(np.int32)}

    def apply(self, batch, params, apply=None):
        assert batch.rgb is not None
        flags = _all(batch.batch_size) if apply is None else apply
        return dataclasses.replace(batch, rgb=ops.aug_rgb_blur(batch.rgb, params["k"], flags))


class ReplaceBackgroundTransform(SceneObservationTransform):
    """``rgb[segmentation == 0] = background[segmentation == 0]`` with ``batch.background``, already at frame size.  With
    ``resize_background=True`` a background of another size is first resized as the reference's ``PIL.Image.resize((w, h))``
    does it: with Pillow's default filter, bicubic."""

    def __init__(self, resize_background: bool = False):
        self.resize_background = resize_background

    def apply(self, batch, params, apply=None):
        assert batch.rgb is not None and batch.segmentation is not None and batch.background is not None
        flags = _all(batch.batch_size) if apply is None else apply
        background = batch.background
        if self.resize_background and background.shape[1:3] != batch.rgb.shape[1:3]:
            background = ops.resize_rgb(background, batch.rgb.shape[1:3], "bicubic")
        return dataclasses.replace(batch, rgb=ops.aug_replace_background(batch.rgb, batch.segmentation, background, flags))


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def k_crop_resize(K: np.ndarray, box: Sequence[float], crop_resize: Tuple[float, float]) -> np.ndarray:
    """The reference's ``get_K_crop_resize`` (lib3d/camera_geometry.py; ``csrc/crop_math.h`` has the same closed form) for
    ``K [B, 3, 3]`` and ONE float box ``(x1, y1, x2, y2)``, in float32: the focal lengths scale by final / crop size, the
    principal point moves with the crop's centre and is rescaled about the pixel centres."""
    f32 = np.float32
    K = np.asarray(K, f32)
    x1, y1, x2, y2 = (f32(v) for v in box)
    final_w, final_h = f32(max(crop_resize)), f32(min(crop_resize))
    crop_w, crop_h = x2 - x1, y2 - y1
    centre_x, centre_y = (crop_w - f32(1)) / f32(2), (crop_h - f32(1)) / f32(2)
    cx = K[:, 0, 2] + centre_x - (x1 + x2) / f32(2)
    cy = K[:, 1, 2] + centre_y - (y1 + y2) / f32(2)
    scale_x, scale_y = final_w / crop_w, final_h / crop_h
    new_K = K.copy()
    new_K[:, 0, 0] = scale_x * K[:, 0, 0]
    new_K[:, 1, 1] = scale_y * K[:, 1, 1]
    new_K[:, 0, 2] = (final_w - f32(1)) / f32(2) + scale_x * (cx - centre_x)
    new_K[:, 1, 2] = (final_h - f32(1)) / f32(2) + scale_y * (cy - centre_y)
    return new_K


class CropResizeToAspectTransform(SceneObservationTransform):
    """The first transform of the reference's chains: frames whose size is not ``resize = (h, w)`` are cropped about their
    centre to its aspect (``PIL.Image.crop`` of the reference's float box: every edge rounded, halves to the even integer; a
    frame that is too wide is padded with zeros, as there) and resized -- RGB with Pillow's BILINEAR, segmentation and depth with
    NEAREST.  ``K`` goes through ``get_K_crop_resize`` twice, with the float box and crop sizes the reference passes (on the
    host: it is 9 numbers per image); ``boxes_modal`` / ``visible`` are recomputed from the resized segmentation for
    ``batch.object_ids``.  ``bbox_amodal`` and ``visib_fract``, which the reference drops, are not part of the batch.  A batch
    that already has the size comes back as it is.  The transform changes the frames' size, so it cannot apply to a part of a
    batch: ``apply`` flags that are not all set raise ValueError."""

    def __init__(self, resize: Tuple[int, int] = (480, 640)):
        assert resize[1] >= resize[0]
        self.resize = (int(resize[0]), int(resize[1]))
        self.aspect = max(resize) / min(resize)

    def crop_box(self, h: int, w: int) -> Optional[Tuple[float, float, float, float]]:
        """The float box ``(x1, y1, x2, y2)`` of the centre crop; None when ``w / h`` is close to the aspect."""
        if np.isclose(w / h, self.aspect):
            return None
        crop_h = w * 1 / self.aspect
        crop_h, crop_w = min(crop_h, w), max(crop_h, w)
        x0, y0 = w / 2, h / 2
        return (x0 - crop_w / 2, y0 - crop_h / 2, x0 + crop_w / 2, y0 + crop_h / 2)

    def apply(self, batch, params, apply=None):
        assert batch.rgb is not None
        assert batch.segmentation is not None
        if apply is not None and not np.asarray(apply, bool).all():
            raise ValueError("CropResizeToAspectTransform changes the frame size: it applies to every image of a batch or to none")
        h, w = int(batch.rgb.shape[1]), int(batch.rgb.shape[2])
        if (h, w) == self.resize:
            return batch
        K = None if batch.K is None else np.asarray(batch.K.detach().cpu(), np.float32).reshape(-1, 3, 3)
        box, rect = self.crop_box(h, w), None
        if box is not None:
            rect = tuple(int(round(v)) for v in box)  # PIL.Image.crop
            if K is not None:
                K = k_crop_resize(K, box, (box[3] - box[1], box[2] - box[0]))
            h, w = rect[3] - rect[1], rect[2] - rect[0]
        out_hw = (min(self.resize), max(self.resize))
        rgb = ops.resize_rgb(batch.rgb, out_hw, "bilinear", crop=rect)
        segmentation = ops.resize_nearest(batch.segmentation, out_hw, crop=rect)
        depth = None if batch.depth is None else ops.resize_nearest(batch.depth, out_hw, crop=rect)
        new = dataclasses.replace(batch, rgb=rgb, segmentation=segmentation, depth=depth)
        if K is not None:
            K = k_crop_resize(K, (0, 0, w, h), out_hw)
            new.K = torch.from_numpy(K).to(device=batch.K.device, dtype=batch.K.dtype).reshape(batch.K.shape)
        if batch.object_ids is not None:
            boxes, n_px = ops.seg_boxes(segmentation, batch.object_ids)
            new.boxes_modal, new.visible = boxes, n_px > 0
        return new


# ---- depth --------------------------------------------------------------------------------------------------------------------------
class DepthTransform(SceneObservationTransform):
    def _transform_depth(self, batch: ObservationBatch, params: Params, flags: np.ndarray) -> torch.Tensor:
        raise NotImplementedError

    def apply(self, batch, params, apply=None):
        assert batch.depth is not None
        flags = _all(batch.batch_size) if apply is None else apply
        return dataclasses.replace(batch, depth=self._transform_depth(batch, params, flags))


class DepthGaussianNoiseTransform(DepthTransform):
    """Adds Gaussian noise of ``std_dev`` to the valid depth pixels."""

    def __init__(self, std_dev: float = 0.02):
        self.std_dev = std_dev

    def draw(self, batch_size, rng):
        return {"seed": _seed(rng)}

    def _transform_depth(self, batch, params, flags):
        return ops.aug_depth_noise(batch.depth, self.std_dev, int(params["seed"][0]), None, flags)


class DepthCorrelatedGaussianNoiseTransform(DepthTransform):
    """Gaussian noise drawn on a grid ``int(H / f) x int(W / f)``, ``f`` uniform in the rescale bounds, upsampled bicubically."""

    def __init__(self, std_dev: float = 0.01, gp_rescale_factor_min: float = 15.0, gp_rescale_factor_max: float = 40.0):
        self.std_dev = std_dev
        self.gp_rescale_factor_min = gp_rescale_factor_min
        self.gp_rescale_factor_max = gp_rescale_factor_max
        self.gp_rescale_factor_bounds = [gp_rescale_factor_min, gp_rescale_factor_max]

    def draw(self, batch_size, rng):
        return {"seed": _seed(rng), "rescale_factor": rng.uniform(self.gp_rescale_factor_min, self.gp_rescale_factor_max, size=batch_size)}

    def _transform_depth(self, batch, params, flags):
        H, W = batch.depth.shape[1:3]
        f = np.asarray(params["rescale_factor"], np.float64)
        grid = ((H / f).astype(int).astype(np.int32), (W / f).astype(int).astype(np.int32))
        return ops.aug_depth_noise(batch.depth, self.std_dev, int(params["seed"][0]), grid, flags)


class DepthMissingTransform(DepthTransform):
    """Drops a fraction, uniform in ``[0, max_missing_fraction]`` (``debug``: the maximum), of the valid depth pixels."""

    def __init__(self, max_missing_fraction: float = 0.2, debug: bool = False):
        self.max_missing_fraction = max_missing_fraction
        self.debug = debug

    def draw(self, batch_size, rng):
        fr = rng.uniform(0, self.max_missing_fraction, size=batch_size)
        if self.debug:
            fr = np.full(batch_size, float(self.max_missing_fraction))
        return {"seed": _seed(rng), "fraction": fr.astype(np.float64)}

    def _transform_depth(self, batch, params, flags):
        return ops.aug_depth_missing(batch.depth, params["fraction"], int(params["seed"][0]), flags)


class DepthDropoutTransform(DepthTransform):
    """Sets the entire depth image to zero."""

    def _transform_depth(self, batch, params, flags):
        return ops.aug_depth_mask(batch.depth, None, flags)


class DepthBackgroundDropoutTransform(DepthTransform):
    """Sets all background depth values to zero."""

    def _transform_depth(self, batch, params, flags):
        assert batch.segmentation is not None
        return ops.aug_depth_mask(batch.depth, batch.segmentation, flags)


def _draw_ellipses(noise_params: dict, std_dev: Optional[float], batch_size: int, rng: np.random.Generator) -> Params:
    """Per image: a Poisson number of ellipses, centres as a uniform ``u`` over the valid pixels, gamma radii rounded to
    integers, integer angles in 0..359 and, for the noise transform, a normal ``value``.  ``table [B, E, 5]``, ``count [B]``."""
    count = rng.poisson(noise_params["ellipse_dropout_mean"], size=batch_size).astype(np.int32)
    E = int(count.max()) if batch_size else 0
    table = np.zeros((batch_size, E, 5), np.float32)
    table[..., 0] = rng.random((batch_size, E), dtype=np.float32)
    for c in (1, 2):
        table[..., c] = np.round(rng.gamma(noise_params["ellipse_gamma_shape"], noise_params["ellipse_gamma_scale"], size=(batch_size, E)))
    table[..., 3] = rng.integers(0, 360, size=(batch_size, E))
    if std_dev is not None:
        table[..., 4] = rng.normal(0.0, std_dev, size=(batch_size, E))
    return {"table": table, "count": count}


class DepthEllipseDropoutTransform(DepthTransform):
    def __init__(self, ellipse_dropout_mean: float = 10.0, ellipse_gamma_shape: float = 5.0, ellipse_gamma_scale: float = 1.0) -> None:
        self._noise_params = {"ellipse_dropout_mean": ellipse_dropout_mean, "ellipse_gamma_scale": ellipse_gamma_scale,
                              "ellipse_gamma_shape": ellipse_gamma_shape}

    def draw(self, batch_size, rng):
        return _draw_ellipses(self._noise_params, None, batch_size, rng)

    def _transform_depth(self, batch, params, flags):
        return ops.aug_depth_ellipses(batch.depth, params["table"], params["count"], False, flags)


class DepthEllipseNoiseTransform(DepthTransform):
    def __init__(self, ellipse_dropout_mean: float = 10.0, ellipse_gamma_shape: float = 5.0, ellipse_gamma_scale: float = 1.0,
                 std_dev: float = 0.01) -> None:
        self.std_dev = std_dev
        self._noise_params = {"ellipse_dropout_mean": ellipse_dropout_mean, "ellipse_gamma_scale": ellipse_gamma_scale,
                              "ellipse_gamma_shape": ellipse_gamma_shape}

    def draw(self, batch_size, rng):
        return _draw_ellipses(self._noise_params, self.std_dev, batch_size, rng)

    def _transform_depth(self, batch, params, flags):
        return ops.aug_depth_ellipses(batch.depth, params["table"], params["count"], True, flags)


class DepthBlurTransform(DepthTransform):
    """``k x k`` box filter, ``k`` an integer of ``factor_interval`` (both ends included)."""

    def __init__(self, factor_interval: Tuple[int, int] = (3, 7)):
        self.factor_interval = factor_interval

    def draw(self, batch_size, rng):
        lo, hi = self.factor_interval
        return {"k": rng.integers(lo, hi + 1, size=batch_size).astype(np.int32)}

    def _transform_depth(self, batch, params, flags):
        return ops.aug_depth_blur(batch.depth, params["k"], flags)


# ---- the reference's chains (toolbox/datasets/pose_dataset.py), as data ----------------------------------------------------------------
RGB_CHAIN = {"p": 0.8, "members": [("PillowBlur", 0.4, {"factor_interval": (1, 3)}),
                                   ("PillowSharpness", 0.3, {"factor_interval": (0.0, 50.0)}),
                                   ("PillowContrast", 0.3, {"factor_interval": (0.2, 50.0)}),
                                   ("PillowBrightness", 0.5, {"factor_interval": (0.1, 6.0)}),
                                   ("PillowColor", 0.3, {"factor_interval": (0.0, 20.0)})]}
_ELLIPSES_MEDIUM = {"ellipse_dropout_mean": 175.0, "ellipse_gamma_shape": 5.0, "ellipse_gamma_scale": 2.0}
_DEPTH_MEDIUM = [("DepthBlurTransform", 0.3, {}),
                 ("DepthCorrelatedGaussianNoiseTransform", 0.3, {"gp_rescale_factor_min": 15.0, "gp_rescale_factor_max": 40.0, "std_dev": 0.01}),
                 ("DepthEllipseDropoutTransform", 0.5, dict(_ELLIPSES_MEDIUM)),
                 ("DepthEllipseNoiseTransform", 0.5, dict(_ELLIPSES_MEDIUM, std_dev=0.01)),
                 ("DepthGaussianNoiseTransform", 0.1, {"std_dev": 0.01}),
                 ("DepthMissingTransform", 0.3, {"max_missing_fraction": 0.9})]
DEPTH_CHAINS = {
    # level 0: the original augmentations, a flat list without an outer probability
    0: {"p": None, "members": [("DepthBlurTransform", 0.3, {}), ("DepthEllipseDropoutTransform", 0.3, {}),
                               ("DepthGaussianNoiseTransform", 0.3, {"std_dev": 0.01}),
                               ("DepthMissingTransform", 0.3, {"max_missing_fraction": 0.2})]},
    1: {"p": 0.8, "members": list(_DEPTH_MEDIUM)},
    2: {"p": 0.8, "members": list(_DEPTH_MEDIUM) + [("DepthDropoutTransform", 0.3, {}), ("DepthBackgroundDropoutTransform", 0.2, {})]},
}
BACKGROUND_P = 0.3


def _build(chain: dict) -> List[SceneObservationAugmentation]:
    members = [SceneObservationAugmentation(globals()[name](**kwargs), p=p) for name, p, kwargs in chain["members"]]
    return members if chain["p"] is None else [SceneObservationAugmentation(members, p=chain["p"])]


def make_rgb_augmentations() -> List[SceneObservationAugmentation]:
    """The reference's RGB chain: blur, sharpness, contrast, brightness, color, each with its own probability, inside p = 0.8."""
    return _build(RGB_CHAIN)


def make_depth_augmentations(level: int = 1) -> List[SceneObservationAugmentation]:
    """The reference's depth chain of ``depth_augmentation_level`` 0, 1 or 2."""
    if level not in DEPTH_CHAINS:
        raise ValueError(f"Unknown depth augmentation type {level}")
    return _build(DEPTH_CHAINS[level])


def make_background_augmentations() -> List[SceneObservationAugmentation]:
    """``ReplaceBackgroundTransform`` with the reference's p = 0.3 (the background frames come with the batch)."""
    return [SceneObservationAugmentation(ReplaceBackgroundTransform(), p=BACKGROUND_P)]


def apply_augmentations(augmentations: Sequence[SceneObservationAugmentation], batch: ObservationBatch,
                        rng: np.random.Generator) -> ObservationBatch:
    for aug in augmentations:
        batch = aug(batch, rng)
    return batch
