"""NumPy float64 reference of the depth refiner of ``csrc/icp.hip`` (``hp_icp_refine`` and its stage entries), written from
the definition in that file's header comment, and the analytic scene its tests use.

Everything is float64 except what the definition itself fixes in float32 and what is therefore exact on both sides: the int16
pixel table ``int16(float32(u) - cx)`` and the comparisons made on the inputs (``> 0``, ``0.2 < z < 5``,
``|zm - zr| <= thresh``).  The increment ``T`` stays float64 from iteration to iteration (the kernels keep it in float32).

A projective ICP decides per source pixel: in front of the camera, which pixel it lands on, inside the image, within the
tolerance.  A float32 evaluation may decide otherwise than this one where a quantity lies on its threshold.  ``accumulate_terms``
therefore reports the margin of every decision and marks a source pixel *fragile* when one of them is small:

* a projected coordinate within ``PX_MARGIN`` of a half-integer (the rounding boundaries; -0.5 and size - 0.5 are the image bounds),
* ``|pz| < PZ_MARGIN`` (a point well behind the camera is dropped by both sides and is not fragile),
* ``| |q - p'| - tol | < TOL_MARGIN``.

A test zeroes the rendered depth at the fragile pixels (``defragilise``): both sides then drop them, as sources and in the
threshold target set, the correspondence sets are identical and the sums can be compared tightly.
"""

from __future__ import annotations

import functools

import numpy as np

N_BLOCKS, N_ACC = 64, 32  # hp_icp_accumulate: d_partial_out [n][64][32]
PX_MARGIN, PZ_MARGIN, TOL_MARGIN = 1e-3, 1e-6, 1e-6


def ipix(n, c):
    """The int16 pixel table of getXYZ: ``int16(float32(i) - c)``, truncation toward zero (exact in float32)."""
    return (np.arange(n, dtype=np.float32) - np.float32(c)).astype(np.int16).astype(np.float64)


def _intrinsics(K):
    K = np.asarray(K, np.float32).reshape(3, 3)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def _shift(a, k, axis):
    """``out[i] = a[i + k]`` along ``axis``, zero outside."""
    out = np.zeros_like(a)
    n = a.shape[axis]
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(max(k, 0), n + min(k, 0))
    dst[axis] = slice(max(-k, 0), n + min(-k, 0))
    out[tuple(dst)] = a[tuple(src)]
    return out


def _binomial5(a):
    w = (1.0, 4.0, 6.0, 4.0, 1.0)
    rows = sum(w[k + 2] * _shift(a, k, 1) for k in range(-2, 3))
    return sum(w[k + 2] * _shift(rows, k, 0) for k in range(-2, 3))


def target_table(depth, K):
    """Points and unit normals of one measured depth map: ``[H, W, 6]`` float64, zeros where the depth is not > 0.

    Smoothed depth = binomial 5x5 average over the valid (> 0) pixels of the window inside the image; points of the smoothed
    depth at the left / right / upper / lower neighbour (the pixel itself at the border); normal = (Xr - Xl) x (Xd - Xu),
    normalised; the point of the table is the back-projection of the raw depth."""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    fx, fy, cx, cy = _intrinsics(K)
    valid = depth > 0
    d = np.where(valid, depth.astype(np.float64), 0.0)
    ws = _binomial5(valid.astype(np.float64))
    sm = np.where(ws > 0, _binomial5(d) / np.where(ws > 0, ws, 1.0), 0.0)
    xs, ys = ipix(W, cx), ipix(H, cy)
    uu, vv = np.meshgrid(np.arange(W), np.arange(H))

    def point(u, v):
        z = sm[v, u]
        return np.stack([xs[u] * z / fx, ys[v] * z / fy, z], -1), z

    Xl, zl = point(np.maximum(uu - 1, 0), vv)
    Xr, zr = point(np.minimum(uu + 1, W - 1), vv)
    Xu, zu = point(uu, np.maximum(vv - 1, 0))
    Xd, zd = point(uu, np.minimum(vv + 1, H - 1))
    nrm = np.cross(Xr - Xl, Xd - Xu)
    nn = np.linalg.norm(nrm, axis=-1)
    ok = valid & (zl > 0) & (zr > 0) & (zu > 0) & (zd > 0) & (nn > 0)
    nrm = np.where(ok[..., None], nrm / np.where(ok, nn, 1.0)[..., None], 0.0)
    pts = np.stack([xs[None, :] * d / fx, ys[:, None] * d / fy, d], -1)
    return np.concatenate([pts, nrm], -1)


def source_set(depth_rendered, depth_measured, mask, depth_delta_thresh):
    """The input-level decisions, in float32 as the kernel makes them: ``(source pixels, target set)``, both ``[H, W]`` bool."""
    dr, dm = np.asarray(depth_rendered, np.float32), np.asarray(depth_measured, np.float32)
    in_range = (dm > np.float32(0.2)) & (dm < np.float32(5))
    if mask is None:
        member = (dr > 0) & (np.abs(dm - dr) <= np.float32(depth_delta_thresh))
        return member & in_range, member & in_range
    return (dr > 0) & (mask != 0) & in_range, (mask != 0) & in_range


def accumulate_terms(mode, T, depth_rendered, depth_measured, mask, K, tgt, tolerance, depth_delta_thresh, dtype=np.float64):
    """One accumulate pass of one prediction.  ``T`` ``[3, 4]`` (ignored in mode 0), ``tgt`` ``[H, W, 6]`` of the prediction's image.

    Returns a dict: ``sums [32]`` and ``abs_sums [32]`` (sum of the absolute values of the terms of each accumulator) in the layout of
    ``hp_icp_accumulate``; ``terms [N, 32]`` and ``pixels [N]`` (flat indices) of the contributing source pixels; for mode 1 also, per
    source pixel of the start set (``src_pixels [M]``): ``pz``, ``m_u`` / ``m_v`` (distance of the projected coordinate to the
    nearest half-integer, NaN where pz <= 0), ``m_tol`` (``|q - p'| - tol`` where a valid target was reached, else NaN), the
    outcome ``state`` (0 inlier, 1 behind the camera, 2 outside the image, 3 invalid target, 4 beyond the tolerance) and
    ``fragile [H, W]`` bool.

    ``dtype=np.float32`` evaluates the same per-pixel expressions in float32 (the terms stay float32; ``sums`` adds them in
    float64): the size of a float32 evaluation's error, from which the tests derive their bounds.  Its margins mean nothing."""
    dr = np.asarray(depth_rendered, np.float32)
    dm = np.asarray(depth_measured, np.float32)
    H, W = dr.shape
    fx, fy, cx, cy = _intrinsics(K)
    src, tgt_set = source_set(dr, dm, mask, depth_delta_thresh)
    pix = np.flatnonzero(src.ravel())
    v, u = np.divmod(pix, W)
    xs, ys = ipix(W, cx).astype(dtype), ipix(H, cy).astype(dtype)
    zr = dr.ravel()[pix].astype(dtype)
    S = np.stack([xs[u] * zr / fx, ys[v] * zr / fy, zr], -1)
    out = dict(src_pixels=pix)
    if mode == 0:
        zm = dm.ravel()[pix].astype(dtype)
        terms = np.zeros((len(pix), N_ACC), dtype)
        terms[:, 0:3] = S
        terms[:, 3:6] = np.stack([xs[u] * zm / fx, ys[v] * zm / fy, zm], -1)
        terms[:, 27] = 1.0
        out.update(terms=terms, pixels=pix, sums=terms.sum(0, dtype=np.float64), abs_sums=np.abs(terms).sum(0, dtype=np.float64), fragile=np.zeros((H, W), bool))
        return out
    T = np.asarray(T, np.float64).astype(dtype).reshape(3, 4)
    tgt = np.asarray(tgt).astype(dtype).reshape(H * W, 6)
    P = S @ T[:, :3].T + T[:, 3]
    pz = P[:, 2]
    front = pz > 0
    zsafe = np.where(front, pz, dtype(1.0))
    pu, pv = fx * P[:, 0] / zsafe + cx, fy * P[:, 1] / zsafe + cy
    half = lambda c: np.abs(c - np.floor(c) - 0.5)  # noqa: E731  distance to the nearest half-integer
    m_u, m_v = np.where(front, half(pu), np.nan), np.where(front, half(pv), np.nan)
    big = 1e9  # a projection this far out is outside the image whatever the rounding
    iu = np.rint(np.clip(pu, -big, big)).astype(np.int64)
    iv = np.rint(np.clip(pv, -big, big)).astype(np.int64)
    inside = front & (iu >= 0) & (iu < W) & (iv >= 0) & (iv < H)
    q = np.where(inside, iv * W + iu, 0)
    t6 = tgt[q]
    qz32 = dm.ravel()[q]
    tvalid = inside & (qz32 > np.float32(0.2)) & (qz32 < np.float32(5)) & (t6[:, 3:] != 0).any(-1) & tgt_set.ravel()[q]
    e = t6[:, :3] - P
    dist = np.sqrt((e ** 2).sum(-1))
    m_tol = np.where(tvalid, dist - dtype(tolerance), np.nan)
    inl = tvalid & (dist <= dtype(tolerance))
    state = np.select([inl, ~front, ~inside, ~tvalid], [0, 1, 2, 3], 4)
    fragile_px = (np.abs(pz) < PZ_MARGIN) | (front & ((m_u < PX_MARGIN) | (m_v < PX_MARGIN))) | (tvalid & (np.abs(m_tol) < TOL_MARGIN))
    fragile = np.zeros(H * W, bool)
    fragile[pix[fragile_px]] = True
    Pk, nk, ek = P[inl], t6[inl, 3:], e[inl]
    r = (nk * ek).sum(-1)
    J = np.concatenate([np.cross(Pk, nk), nk], -1)
    terms = np.zeros((int(inl.sum()), N_ACC), dtype)
    o = 0
    for i in range(6):
        for j in range(i, 6):
            terms[:, o] = J[:, i] * J[:, j]
            o += 1
    terms[:, 21:27] = J * r[:, None]
    terms[:, 27] = 1.0
    terms[:, 28] = r * r
    out.update(terms=terms, pixels=pix[inl], sums=terms.sum(0, dtype=np.float64), abs_sums=np.abs(terms).sum(0, dtype=np.float64), pz=pz, m_u=m_u, m_v=m_v, m_tol=m_tol,
               state=state, fragile=fragile.reshape(H, W))
    return out


def normal_equations(sums):
    """``(A [6, 6], b [6])`` of the 32 sums, with the regularisation of the definition on the diagonal."""
    A = np.zeros((6, 6))
    o = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = sums[o]
            o += 1
    return A + (1e-9 * np.trace(A) + 1e-12) * np.eye(6), np.asarray(sums[21:27], np.float64)


def solve_increment(sums):
    """The increment ``x = (rotation vector, translation)`` of one iteration, or None where the definition gives up: fewer than 6
    correspondences, or the regularised matrix is not positive definite."""
    if sums[27] < 6:
        return None
    A, b = normal_equations(sums)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if not th > 1e-12:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def compose(T, x):
    """``dT(x) T``: ``[3, 4]``."""
    R = rodrigues(x[:3])
    return np.concatenate([R @ T[:, :3], (R @ T[:, 3] + x[3:])[:, None]], 1)


def refine(depth_rendered, depth_measured, mask, K, TCO, n_iterations, n_min_points, tolerance, depth_delta_thresh, tgt=None):
    """One prediction through the whole refinement.  Returns a dict: ``pose [4, 4]`` (``TCO`` itself where rejected), ``retval``
    (0 / -1), ``residual`` (-1 where rejected), ``reason`` (None, "start", "few", "solve", "inliers"), ``n_start``, ``n_inliers``
    of the final increment, ``T`` (the increments after the centroid start and after every iteration), ``fragile [H, W]`` (the
    union over every pass made) and ``passes`` (the ``accumulate_terms`` results of the mode-1 passes)."""
    TCO = np.asarray(TCO)
    if tgt is None:
        tgt = target_table(depth_measured, K)
    args = (depth_rendered, depth_measured, mask, K, tgt, tolerance, depth_delta_thresh)
    a0 = accumulate_terms(0, None, *args)
    n0 = int(round(a0["sums"][27]))
    out = dict(pose=TCO.copy(), retval=-1, residual=-1.0, n_start=n0, n_inliers=0, T=[], passes=[], fragile=np.zeros(np.shape(depth_rendered), bool))
    if n0 < n_min_points:
        return dict(out, reason="start")
    T = np.concatenate([np.eye(3), ((a0["sums"][3:6] - a0["sums"][0:3]) / n0)[:, None]], 1)
    out["T"].append(T)
    for _ in range(n_iterations):
        a = accumulate_terms(1, T, *args)
        out["passes"].append(a)
        out["fragile"] |= a["fragile"]
        x = solve_increment(a["sums"])
        if x is None:
            return dict(out, reason="few" if a["sums"][27] < 6 else "solve")
        T = compose(T, x)
        out["T"].append(T)
    a = accumulate_terms(1, T, *args)
    out["passes"].append(a)
    out["fragile"] |= a["fragile"]
    cnt = int(round(a["sums"][27]))
    out["n_inliers"] = cnt
    residual = float(np.sqrt(a["sums"][28] / cnt)) if cnt > 0 else -1.0
    if cnt == 0 or residual > tolerance or cnt < n_min_points:
        return dict(out, reason="inliers")
    T4 = np.concatenate([T, [[0, 0, 0, 1.0]]], 0)
    return dict(out, pose=T4 @ TCO.astype(np.float64), retval=0, residual=residual, reason=None)


def defragilise(depth_rendered, run):
    """Zero ``depth_rendered`` (a copy) at the fragile pixels of ``run(depth_rendered)`` (an ``[H, W]`` bool) until none is left.
    Returns ``(depth, number of pixels removed)``."""
    d = np.array(depth_rendered, np.float32)
    removed = 0
    for _ in range(40):
        f = run(d)
        if not f.any():
            return d, removed
        removed += int((f & (d > 0)).sum())
        d[f] = 0
    raise AssertionError("fragile pixels keep appearing")


# ---- the analytic scene ----------------------------------------------------------------------------------------------

def rot(axis, deg):
    return rodrigues(np.asarray(axis, np.float64) / np.linalg.norm(axis) * np.deg2rad(deg))


def camera(H, W, scale=1.0):
    """Intrinsics with a fractional principal point (``u - cx`` is negative and non-integer on the left half: the int16 table
    truncates toward zero there, it does not floor)."""
    f = 1.6 * H * scale
    return np.array([[f, 0, W / 2 - 0.63], [0, 1.04 * f, H / 2 + 0.19], [0, 0, 1]], np.float32)


ELLIPSOID = dict(center=np.array([0.012, -0.009, 0.80]), semi=np.array([0.20, 0.125, 0.09]), R=rot([0.3, 1.0, 0.5], 28.0))
PLANE_Z = 1.1   # the background: more than depth_delta_thresh (0.1) behind the ellipsoid, whose far side ends before 1.0
PATCH_Z = 0.75  # the fronto-parallel patch: exact in float32, so is every weighted mean of it
PATCH = 11      # its side, top left corner of the image


def ellipsoid_depth(H, W, K, motion=None):
    """Depth map ``[H, W]`` float32 (0 where the ray misses) of the tri-axial ellipsoid moved by ``motion`` ``[3, 4]``, along the
    rays of the int16 pixel table: the smaller root of ``z^2 d'Ad - 2 z d'Ac + c'Ac - 1 = 0``."""
    fx, fy, cx, cy = _intrinsics(K)
    c, R = ELLIPSOID["center"], ELLIPSOID["R"]
    if motion is not None:
        motion = np.asarray(motion, np.float64)
        c, R = motion[:, :3] @ c + motion[:, 3], motion[:, :3] @ R
    A = R @ np.diag(1.0 / ELLIPSOID["semi"] ** 2) @ R.T
    d = np.stack(np.broadcast_arrays(ipix(W, cx)[None, :] / fx, ipix(H, cy)[:, None] / fy, np.ones((H, W))), -1)
    a, b, cc = np.einsum("hwi,ij,hwj->hw", d, A, d), d @ (A @ c), float(c @ A @ c) - 1.0
    disc = b * b - a * cc
    z = (b - np.sqrt(np.maximum(disc, 0.0))) / a
    return np.where((disc > 0) & (z > 0), z, 0.0).astype(np.float32)


def true_motion(seed):
    """A rigid motion of about 1 degree and a few millimetres, ``[3, 4]``: rotation about the ellipsoid's centre."""
    rs = np.random.RandomState(1000 + seed)
    R = rodrigues(rs.normal(0, 1, 3) * np.deg2rad(0.6))
    c = ELLIPSOID["center"]
    t = rs.normal(0, 1, 3) * np.array([0.002, 0.002, 0.003])
    return np.concatenate([R, (c - R @ c + t)[:, None]], 1)


def invert(M):
    R = M[:, :3].T
    return np.concatenate([R, (-R @ M[:, 3])[:, None]], 1)


def make_image(H, W, seed, scale=1.0):
    """One measured image: ``dict(K, measured, holes, patch_interior)``.  Measured depth = the ellipsoid over the background
    plane, the patch, then the holes: about 20 % random zeros, an empty 7x7 block and a 7x7 block empty but for its centre, both
    on the ellipsoid."""
    rs = np.random.RandomState(seed)
    K = camera(H, W, scale)
    e = ellipsoid_depth(H, W, K)
    m = np.where(e > 0, e, np.float32(PLANE_Z)).astype(np.float32)
    m[:PATCH, :PATCH] = PATCH_Z
    m[rs.rand(H, W) < 0.2] = 0
    v0, u0 = H // 2 - 8, W // 2 - 9
    m[v0:v0 + 7, u0:u0 + 7] = 0
    v1, u1 = H // 2 + 2, W // 2 + 3
    keep = e[v1 + 3, u1 + 3]
    m[v1:v1 + 7, u1:u1 + 7] = 0
    m[v1 + 3, u1 + 3] = keep
    inner = np.zeros((H, W), bool)
    inner[:PATCH - 3, :PATCH - 3] = True  # every pixel within 3 of these lies in the patch or outside the image
    return dict(K=K, measured=m, empty_block=(v0, u0), lone_pixel=(v1 + 3, u1 + 3), patch_interior=inner)


def make_prediction(image, seed):
    """One prediction on ``image``: the ellipsoid rendered ``true_motion(seed)^-1`` away from where it is measured, so the
    refinement should find ``true_motion(seed)``; ``mask`` is a box around the object that also holds background."""
    H, W = image["measured"].shape
    M = true_motion(seed)
    rendered = ellipsoid_depth(H, W, image["K"], invert(M))
    vs, us = np.nonzero(rendered > 0)
    mask = np.zeros((H, W), np.uint8)
    mask[max(vs.min() - 2, 0):vs.max() + 3, max(us.min() - 2, 0):us.max() + 3] = 1
    TCO = np.eye(4, dtype=np.float32)
    TCO[:3, :3] = (invert(M)[:, :3] @ ELLIPSOID["R"]).astype(np.float32)
    TCO[:3, 3] = (invert(M)[:, :3] @ ELLIPSOID["center"] + invert(M)[:, 3]).astype(np.float32)
    return dict(rendered=rendered, motion=M, mask=mask, TCO=TCO)


def make_batch(H, W, im_ids, B):
    """``B`` images (own holes, own focal length) and one prediction per entry of ``im_ids``: ``(images, predictions)``."""
    images = [make_image(H, W, seed=b, scale=1.0 + 0.06 * b) for b in range(B)]
    return images, [make_prediction(images[b], seed=i) for i, b in enumerate(im_ids)]


def stage_increments():
    """The increments of the accumulate tests, ``(name, T [3, 4], tolerance)``: identity; about 1 degree about the ellipsoid's
    centre and 3 mm; and a quarter turn about the camera's y axis that leaves part of the points behind the camera and part of
    the rest outside the image (tolerance 1 m, so that what does land on a valid target counts)."""
    c = ELLIPSOID["center"]
    R1 = rot([1.0, 2.0, -1.0], 1.0)
    small = np.concatenate([R1, (c - R1 @ c + np.array([0.002, -0.001, 0.002]))[:, None]], 1)
    far = np.concatenate([rot([0.0, 1.0, 0.0], 88.0), np.array([[-0.75], [0.0], [0.08]])], 1)
    return [("identity", np.eye(3, 4), 0.05), ("small", small, 0.05), ("far", far, 1.0)]


# ---- the cases shared by tests/test_icp_reference.py and tests/test_gpu_icp_stages.py (computed once) ----------------------

SHAPES = ((37, 53), (64, 64), (120, 160))  # blocks past the end and idle lanes / a multiple of 64 / two trips of the strided loop
IM_IDS, N_IMAGES = (1, 0, 1), 2
DELTA_THRESH = 0.1
MAX_FRAGILE_SHARE = 0.02
# the large call of the workspace test: 5 predictions over 3 images at 120x160, 2 iterations.  Freeing 3 passes of fragile pixels
# moves the increment and makes others fragile; it ends after up to 28 rounds with 1.7 % .. 8.0 % of the source set gone
LARGE_SHAPE, LARGE_IM_IDS, LARGE_N_IMAGES, MAX_FRAGILE_SHARE_LARGE_RUN = (120, 160), (2, 0, 2, 1, 0), 3, 0.08


@functools.lru_cache(maxsize=None)
def batch(H, W, im_ids=IM_IDS, n_images=N_IMAGES):
    images, preds = make_batch(H, W, im_ids, n_images)
    tgt = np.stack([target_table(im["measured"], im["K"]) for im in images])
    return images, preds, tgt


def image_masks(preds, im_ids=IM_IDS, n_images=N_IMAGES):
    """One mask per image, as the kernels take them: the union of the boxes of the image's predictions ``[n_images, H, W]``."""
    return np.stack([np.max([np.zeros_like(preds[0]["mask"])] + [p["mask"] for p, b in zip(preds, im_ids) if b == image], 0)
                     for image in range(n_images)])


@functools.lru_cache(maxsize=None)
def accumulate_cases(H, W, masked):
    """For every increment of ``stage_increments``: the rendered depths ``[n, H, W]`` without their fragile pixels, the float64
    results per prediction on them (the table is the float64 one rounded to float32: what the kernel is given), and the largest
    share of the source set that was removed.  ``masked``: the masks are those of the images (``image_masks``)."""
    images, preds, tgt = batch(H, W)
    tgt32 = tgt.astype(np.float32)
    masks = image_masks(preds) if masked else None
    cases = []
    for name, T, tol in stage_increments():
        dr, refs, share = [], [], 0.0
        for i, b in enumerate(IM_IDS):
            im, pr = images[b], preds[i]
            args = (im["measured"], masks[b] if masked else None, im["K"], tgt32[b], tol, DELTA_THRESH)
            n_src = len(accumulate_terms(0, None, pr["rendered"], *args)["src_pixels"])
            d, removed = defragilise(pr["rendered"], lambda d: accumulate_terms(1, T, d, *args)["fragile"])
            share = max(share, removed / n_src)
            dr.append(d)
            refs.append({0: accumulate_terms(0, None, d, *args), 1: accumulate_terms(1, T, d, *args)})
        cases.append(dict(name=name, T=T, tolerance=tol, rendered=np.stack(dr), refs=refs, fragile_share=share, masks=masks))
    return cases


def plane_case(H, W):
    """The degenerate scene: the measured depth is one fronto-parallel plane (normals exactly (0, 0, 1), holes as elsewhere), the
    rendered depth a slightly tilted plane 4 mm nearer over a box."""
    rs = np.random.RandomState(77)
    measured = np.full((H, W), PATCH_Z, np.float32)
    measured[rs.rand(H, W) < 0.2] = 0
    rendered = np.zeros((H, W), np.float32)
    v, u = np.mgrid[4:H - 4, 5:W - 5]
    rendered[4:H - 4, 5:W - 5] = PATCH_Z - 0.004 + 2e-4 * (u - W / 2) - 1e-4 * (v - H / 2)
    TCO = np.eye(4, dtype=np.float32)
    TCO[2, 3] = PATCH_Z
    return dict(K=camera(H, W), measured=measured, rendered=rendered, TCO=TCO)


def starved_prediction(image, seed):
    """A prediction whose start set is large and whose inliers are few: its rendered depth is the measured surface pushed back by
    0 (40 % of the pixels), 90 mm (40 %) or 45 mm (20 %), all inside depth_delta_thresh = 0.1.  The centroid start moves it
    45 mm: with a tolerance of 20 mm only the last fifth stays within reach."""
    pr = make_prediction(image, seed)
    rs = np.random.RandomState(500 + seed)
    cls = rs.choice(3, size=pr["rendered"].shape, p=[0.4, 0.4, 0.2])
    off = np.array([0.0, 0.09, 0.045], np.float32)[cls]
    H, W = pr["rendered"].shape
    e = ellipsoid_depth(H, W, image["K"])
    return dict(pr, rendered=np.where(e > 0, e + off, 0).astype(np.float32))


@functools.lru_cache(maxsize=None)
def run_cases(H, W, masked, n_iterations, im_ids=IM_IDS, n_images=N_IMAGES, n_min_points=50, tolerance=0.05):
    """Full runs of the predictions of ``batch(H, W, im_ids, n_images)``: per prediction the rendered depth without the pixels that
    are fragile in any pass of the float64 run on it (removed until none is left), that run, and the share of the source set removed."""
    images, preds, tgt = batch(H, W, im_ids, n_images)
    masks = image_masks(preds, im_ids, n_images) if masked else None
    cases = []
    for i, b in enumerate(im_ids):
        im, mask = images[b], masks[b] if masked else None
        run = lambda d: refine(d, im["measured"], mask, im["K"], preds[i]["TCO"], n_iterations, n_min_points, tolerance, DELTA_THRESH, tgt=tgt[b])  # noqa: E731
        n_src = run(preds[i]["rendered"])["n_start"]
        d, removed = defragilise(preds[i]["rendered"], lambda d: run(d)["fragile"])
        cases.append(dict(rendered=d, mask=mask, ref=run(d), fragile_share=removed / n_src))
    return cases
