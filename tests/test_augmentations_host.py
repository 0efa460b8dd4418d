"""Host-side checks of the augmentations: argument errors of every hp_aug_* entry point without a GPU, the draws, the nesting of
the apply flags and the factory chains against the reference's probabilities and intervals."""

import numpy as np
import pytest
import torch

from happypose_amd import _ffi
from happypose_amd import augmentations as A
from happypose_amd import ops

P = 4096  # stands for a device pointer: an argument error is reported before anything is dereferenced


def _calls(B, h, w, null):
    """One call per entry point; ``null`` names the argument that is NULL (or None for none)."""
    def p(name):
        return None if name == null else P

    lib = _ffi.lib()
    big = 1 << 40
    return {
        "hp_aug_rgb_enhance": lambda: lib.hp_aug_rgb_enhance(B, h, w, p("in"), P, P, p("apply"), p("out"), P, big, None),
        "hp_aug_rgb_blur": lambda: lib.hp_aug_rgb_blur(B, h, w, p("in"), P, P, P, p("apply"), p("out"), 0, P, big, None),
        "hp_aug_replace_background": lambda: lib.hp_aug_replace_background(B, h, w, p("in"), P, P, p("apply"), p("out"), None),
        "hp_aug_depth_noise": lambda: lib.hp_aug_depth_noise(B, h, w, p("in"), P, 0, None, None, p("apply"), 1, p("out"), None, 0, None),
        "hp_aug_depth_missing": lambda: lib.hp_aug_depth_missing(B, h, w, p("in"), P, p("apply"), 1, p("out"), P, big, None),
        "hp_aug_depth_ellipses": lambda: lib.hp_aug_depth_ellipses(B, h, w, p("in"), P, P, 4, 0, p("apply"), p("out"), P, big, None),
        "hp_aug_depth_blur": lambda: lib.hp_aug_depth_blur(B, h, w, p("in"), P, 3, p("apply"), p("out"), None),
        "hp_aug_depth_mask": lambda: lib.hp_aug_depth_mask(B, h, w, p("in"), None, p("apply"), p("out"), None),
    }


@pytest.mark.parametrize("name", sorted(_calls(1, 1, 1, None)))
def test_argument_errors_reported_without_gpu(name):
    lib = _ffi.lib()
    for B, h, w, null in ((-1, 8, 8, None), (2, 0, 8, None), (2, 8, -3, None), (70000, 8, 8, None), (2, 1 << 15, 1 << 15, None),
                          (2, 8, 8, "in"), (2, 8, 8, "out"), (2, 8, 8, "apply")):
        rc = _calls(B, h, w, null)[name]()
        assert rc == -1 and name.encode() in lib.hp_last_error(), (name, B, h, w, null)
    assert _calls(0, 8, 8, "in")[name]() == 0  # B == 0: HP_OK, nothing launched, no pointer looked at


def test_workspace_and_aliasing_errors_without_gpu():
    lib = _ffi.lib()
    assert lib.hp_aug_workspace_bytes(2, 3, 5, 0) == 16 + 120 and lib.hp_aug_workspace_bytes(3, 3, 5, 7) == 24 + 184 + 32 * 21
    for bad in ((-1, 3, 5, 0), (2, 0, 5, 0), (2, 3, 5, -1), (70000, 3, 5, 0), (1, 1 << 15, 1 << 15, 0)):
        assert lib.hp_aug_workspace_bytes(*bad) == -1
    small = lib.hp_aug_workspace_bytes(2, 8, 8, 0) - 1
    assert lib.hp_aug_rgb_enhance(2, 8, 8, P, P, P, P, 2 * P, P, small, None) == -1 and b"workspace" in lib.hp_last_error()
    assert lib.hp_aug_depth_missing(2, 8, 8, P, P, P, 1, P, P + 4, 1 << 40, None) == -1 and b"aligned" in lib.hp_last_error()
    assert lib.hp_aug_depth_noise(2, 8, 8, P, P, 1, None, P, P, 1, P, P, 1 << 40, None) == -1  # correlated without a grid
    # the neighbourhood entry points refuse to run in place
    assert lib.hp_aug_rgb_enhance(2, 8, 8, P, P, P, P, P, P, 1 << 40, None) == -1 and b"alias" in lib.hp_last_error()
    assert lib.hp_aug_rgb_blur(2, 8, 8, P, P, P, P, P, P, 0, P, 1 << 40, None) == -1 and b"alias" in lib.hp_last_error()
    assert lib.hp_aug_depth_blur(2, 8, 8, P, P, 3, P, P, None) == -1 and b"alias" in lib.hp_last_error()
    # a side shorter than k: reflect-101 is not defined
    assert lib.hp_aug_depth_blur(2, 8, 6, P, P, 7, P, 2 * P, None) == -1 and b"shorter" in lib.hp_last_error()
    assert lib.hp_aug_depth_blur(2, 8, 8, P, P, 0, P, 2 * P, None) == -1


def test_wrappers_refuse_cpu_tensors():
    rgb, depth, seg = torch.zeros(2, 4, 5, 3, dtype=torch.uint8), torch.zeros(2, 4, 5), torch.zeros(2, 4, 5, dtype=torch.int32)
    for call in (lambda: ops.aug_rgb_enhance(rgb, "color", 1.0), lambda: ops.aug_rgb_blur(rgb, 2),
                 lambda: ops.aug_replace_background(rgb, seg, rgb), lambda: ops.aug_depth_noise(depth, 0.01, 1),
                 lambda: ops.aug_depth_missing(depth, 0.1, 1), lambda: ops.aug_depth_ellipses(depth, np.zeros((2, 1, 5)), [0, 0], False),
                 lambda: ops.aug_depth_blur(depth, 3), lambda: ops.aug_depth_mask(depth, seg)):
        with pytest.raises(ValueError):
            call()


def test_blur_parameters_of_the_wrapper():
    assert [ops.aug_blur_params(k) for k in (1, 2, 3)] == [(0, 11184811, 2796202), (1, 4473924, 1677722), (2, 2876094, 1198373)]


ALL = [A.PillowBlur, A.PillowSharpness, A.PillowContrast, A.PillowBrightness, A.PillowColor, A.DepthGaussianNoiseTransform,
       A.DepthCorrelatedGaussianNoiseTransform, A.DepthMissingTransform, A.DepthDropoutTransform, A.DepthEllipseDropoutTransform,
       A.DepthEllipseNoiseTransform, A.DepthBlurTransform, A.DepthBackgroundDropoutTransform, A.ReplaceBackgroundTransform]


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


@pytest.mark.parametrize("cls", ALL)
def test_draw_is_deterministic(cls):
    t = cls()
    a, b = t.draw(64, np.random.default_rng(5)), t.draw(64, np.random.default_rng(5))
    assert _same(a, b) and all(len(v) in (1, 64) for v in a.values())
    if a:
        assert not _same(a, t.draw(64, np.random.default_rng(6)))


def test_draw_ranges():
    rng = np.random.default_rng(0)
    n = 4000
    for cls, (lo, hi) in ((A.PillowSharpness, (0.0, 50.0)), (A.PillowContrast, (0.2, 50.0)), (A.PillowBrightness, (0.1, 6.0)),
                          (A.PillowColor, (0, 20.0))):
        f = cls().draw(n, rng)["factor"]
        assert cls().factor_interval == (lo, hi) and f.dtype == np.float32 and lo <= f.min() < lo + 0.5 and hi - 0.5 < f.max() <= hi
    assert sorted(set(A.PillowBlur().draw(n, rng)["k"])) == [1, 2, 3]
    assert sorted(set(A.DepthBlurTransform().draw(n, rng)["k"])) == [3, 4, 5, 6, 7]
    f = A.DepthCorrelatedGaussianNoiseTransform().draw(n, rng)["rescale_factor"]
    assert 15.0 <= f.min() < 15.5 and 39.5 < f.max() <= 40.0
    fr = A.DepthMissingTransform(0.9).draw(n, rng)["fraction"]
    assert fr.dtype == np.float64 and 0 <= fr.min() and 0.85 < fr.max() <= 0.9
    assert (A.DepthMissingTransform(0.4, debug=True).draw(5, rng)["fraction"] == 0.4).all()
    assert A.DepthGaussianNoiseTransform().std_dev == 0.02 and A.DepthMissingTransform().max_missing_fraction == 0.2
    e = A.DepthEllipseNoiseTransform(ellipse_dropout_mean=175.0, ellipse_gamma_scale=2.0).draw(200, rng)
    t, c = e["table"], e["count"]
    assert t.shape == (200, c.max(), 5) and t.dtype == np.float32 and abs(c.mean() - 175) < 4
    assert 0 <= t[..., 0].min() and t[..., 0].max() < 1 and (t[..., 1:3] == np.round(t[..., 1:3])).all() and abs(t[..., 1].mean() - 10) < 0.2
    assert t[..., 3].min() == 0 and t[..., 3].max() == 359 and abs(t[..., 4].std() - 0.01) < 0.001
    assert (A.DepthEllipseDropoutTransform().draw(50, rng)["table"][..., 4] == 0).all()


class _Record(A.SceneObservationTransform):
    def __init__(self, log):
        self.log = log

    def apply(self, batch, params, apply=None):
        self.log.append(np.array(apply, bool))
        return batch


def test_flags_nest_as_in_the_reference():
    log = []
    aug = A.SceneObservationAugmentation([A.SceneObservationAugmentation(_Record(log), p=0.5),
                                          A.SceneObservationAugmentation(_Record(log), p=1.0)], p=0.6)
    n = 20000
    params = aug.draw(n, np.random.default_rng(1))
    aug.apply(A.ObservationBatch(rgb=torch.zeros(n, 1, 1, 3, dtype=torch.uint8)), params)
    outer, inner = params["apply"], params["inner"][0]["apply"]
    assert np.array_equal(log[0], outer & inner) and np.array_equal(log[1], outer)  # in order, and-ed with the outer flags
    assert abs(outer.mean() - 0.6) < 0.015 and abs(log[0].mean() - 0.3) < 0.015
    assert A.SceneObservationAugmentation(_Record(log), p=0.0).draw(100, np.random.default_rng(0))["apply"].sum() == 0
    assert A.SceneObservationAugmentation(_Record(log)).draw(100, np.random.default_rng(0))["apply"].all()  # p = 1 by default


def _describe(augs):
    return [(type(a.transform).__name__, a.p) if not isinstance(a.transform, list) else ("list", a.p, _describe(a.transform)) for a in augs]


def test_factory_chains_match_the_reference():
    """The probabilities, order and intervals of toolbox/datasets/pose_dataset.py:125-215."""
    (rgb,) = A.make_rgb_augmentations()
    assert _describe([rgb]) == [("list", 0.8, [("PillowBlur", 0.4), ("PillowSharpness", 0.3), ("PillowContrast", 0.3),
                                               ("PillowBrightness", 0.5), ("PillowColor", 0.3)])]
    assert [t.transform.factor_interval for t in rgb.transform] == [(1, 3), (0.0, 50.0), (0.2, 50.0), (0.1, 6.0), (0.0, 20.0)]
    assert _describe(A.make_depth_augmentations(0)) == [("DepthBlurTransform", 0.3), ("DepthEllipseDropoutTransform", 0.3),
                                                        ("DepthGaussianNoiseTransform", 0.3), ("DepthMissingTransform", 0.3)]
    lvl0 = [a.transform for a in A.make_depth_augmentations(0)]
    assert lvl0[0].factor_interval == (3, 7) and lvl0[2].std_dev == 0.01 and lvl0[3].max_missing_fraction == 0.2
    assert lvl0[1]._noise_params == {"ellipse_dropout_mean": 10.0, "ellipse_gamma_shape": 5.0, "ellipse_gamma_scale": 1.0}
    medium = [("DepthBlurTransform", 0.3), ("DepthCorrelatedGaussianNoiseTransform", 0.3), ("DepthEllipseDropoutTransform", 0.5),
              ("DepthEllipseNoiseTransform", 0.5), ("DepthGaussianNoiseTransform", 0.1), ("DepthMissingTransform", 0.3)]
    assert _describe(A.make_depth_augmentations(1)) == [("list", 0.8, medium)]
    assert _describe(A.make_depth_augmentations(2)) == [("list", 0.8, medium + [("DepthDropoutTransform", 0.3),
                                                                               ("DepthBackgroundDropoutTransform", 0.2)])]
    m = [a.transform for a in A.make_depth_augmentations(1)[0].transform]
    assert m[1].gp_rescale_factor_bounds == [15.0, 40.0] and m[1].std_dev == 0.01 and m[4].std_dev == 0.01 and m[3].std_dev == 0.01
    for t in (m[2], m[3]):
        assert t._noise_params == {"ellipse_dropout_mean": 175.0, "ellipse_gamma_shape": 5.0, "ellipse_gamma_scale": 2.0}
    assert m[5].max_missing_fraction == 0.9
    assert _describe(A.make_background_augmentations()) == [("ReplaceBackgroundTransform", 0.3)]
    with pytest.raises(ValueError):
        A.make_depth_augmentations(3)
