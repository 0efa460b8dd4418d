"""numpy restatement of csrc/scene.hip: compose, visibility, contour, overlay.

Compose and visibility restate rules that are plain (argmin of the positive depths, pixel counts and boxes).  For CONTOUR and
OVERLAY this file is the specification: the reference's ``make_contour_overlay`` runs ``cv2.Canny`` + ``cv2.dilate`` and its
``plot_overlay`` lives in a bokeh plotter, and neither ``cv2`` nor ``bokeh`` is installed, so no golden can be generated from the
reference for them.  The contour is this repository's own definition (include/happypose_amd.h, ``hp_scene_contour``); the overlay
formula is copied from ``TB/visualization/bokeh_plotter.py:133-139``.
"""

import numpy as np


def compose(layer_off, rgb, nrm, depth):
    """Layers [L, 3, H, W] / [L, 1, H, W], sorted by camera (``layer_off`` [n_cam + 1]).  Winner of a pixel: argmin over
    ``where(d > 0, d, inf)`` (numpy's argmin returns the lowest index on a tie); nothing wins where the minimum is inf."""
    layer_off = np.asarray(layer_off)
    n_cam = len(layer_off) - 1
    h, w = depth.shape[2:]
    out = {"rgb": np.zeros((n_cam, 3, h, w), np.float32), "normals": None if nrm is None else np.zeros((n_cam, 3, h, w), np.float32),
           "depth": np.zeros((n_cam, 1, h, w), np.float32), "ids": np.full((n_cam, h, w), -1, np.int32),
           "mask": np.zeros((n_cam, 1, h, w), np.uint8)}
    for c in range(n_cam):
        a, b = int(layer_off[c]), int(layer_off[c + 1])
        if a == b:
            continue
        d = depth[a:b, 0]
        key = np.where(d > 0, d, np.inf).astype(np.float32)
        win = key.argmin(0)
        cov = np.take_along_axis(key, win[None], 0)[0] < np.inf
        out["ids"][c] = np.where(cov, win, -1)
        out["mask"][c, 0] = cov
        out["depth"][c, 0] = np.where(cov, np.take_along_axis(d, win[None], 0)[0], 0)
        for name, src in (("rgb", rgb), ("normals", nrm)):
            if src is not None:
                picked = np.take_along_axis(src[a:b], win[None, None].repeat(3, 1), 0)[0]
                out[name][c] = np.where(cov[None], picked, 0)
    return out


def _box(m):
    if not m.any():
        return [-1, -1, -1, -1]
    ys, xs = np.nonzero(m)
    return [xs.min(), ys.min(), xs.max(), ys.max()]


def visibility(layer_off, depth, ids):
    """int32 [L, 10]: px_count_all, px_count_visib, bbox_all (x_min, y_min, x_max, y_max), bbox_visib; empty box = -1."""
    layer_off = np.asarray(layer_off)
    table = np.zeros((depth.shape[0], 10), np.int32)
    for c in range(len(layer_off) - 1):
        for l in range(int(layer_off[c]), int(layer_off[c + 1])):
            m_all, m_vis = depth[l, 0] > 0, ids[c] == l - int(layer_off[c])
            table[l] = [m_all.sum(), m_vis.sum(), *_box(m_all), *_box(m_vis)]
    return table


def contour(frame, labels, color, dilate_iterations):
    """``frame`` (h, w, 3) uint8; ``labels`` (h, w) int: >= 0 inside (the object id in per-object mode, 0 for a plain mask), < 0
    outside.  edge0[p]: p inside and a 4-neighbour inside the image has another label; edge[p]: some q within Chebyshev distance
    ``dilate_iterations`` has edge0[q].  Returns (painted copy, edge map uint8 0 / 255)."""
    lab = np.where(labels >= 0, labels, -1).astype(np.int64)
    h, w = lab.shape
    inside = lab >= 0
    e0 = np.zeros((h, w), bool)
    e0[:, 1:] |= inside[:, 1:] & (lab[:, 1:] != lab[:, :-1])
    e0[:, :-1] |= inside[:, :-1] & (lab[:, :-1] != lab[:, 1:])
    e0[1:, :] |= inside[1:, :] & (lab[1:, :] != lab[:-1, :])
    e0[:-1, :] |= inside[:-1, :] & (lab[:-1, :] != lab[1:, :])
    r = int(dilate_iterations)
    pad = np.pad(e0, r)
    e = np.zeros((h, w), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            e |= pad[dy:dy + h, dx:dx + w]
    out = frame.copy()
    out[e] = np.asarray(color, np.uint8)
    return out, e.astype(np.uint8) * 255


def overlay(rgb_input, rgb_rendered, mask=None):
    """``BokehPlotter.plot_overlay`` (``TB/visualization/bokeh_plotter.py:133-139``); ``mask`` None = ``get_mask_from_rgb``."""
    assert rgb_input.dtype == np.uint8 and rgb_rendered.dtype == np.uint8
    if mask is None:
        mask = (rgb_rendered > 0).any(-1)
    mask = np.asarray(mask, bool)
    rgb_overlay = np.zeros_like(rgb_input).astype(np.float32)
    rgb_overlay[~mask] = rgb_input[~mask] * 0.6 + 255 * 0.4
    rgb_overlay[mask] = rgb_rendered[mask] * 0.8 + 255 * 0.2
    return rgb_overlay.astype(np.uint8)
