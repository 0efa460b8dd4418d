"""Float64 NumPy restatement of the training losses of ``include/happypose_amd.h`` (section "The losses the pose networks are
trained and validated on") with the analytic gradient: the yardstick of tests/test_pose_losses_reference.py (against the
reference's own float64 run and finite differences) and of tests/test_gpu_pose_losses.py (bounds, allowances).  Test
infrastructure only; rows are batched over the leading axis."""

import numpy as np

TERMS = ("orn", "xy", "z")
# the difference components that feed a gradient: every one for the symmetric loss and the orientation term; x, y of the xy term;
# z of the z term
FEEDS = {"sym": [(0, (0, 1, 2))], "refiner": [(0, (0, 1, 2)), (1, (0, 1)), (2, (2,))]}


def transform(T, p):
    """T [..., 4, 4], p [B, N, 3] -> [..., N, 3] with T's leading axes (B or B, S)."""
    T = np.asarray(T, np.float64)
    p = np.asarray(p, np.float64)
    if T.ndim == 4:
        p = p[:, None]
    return np.einsum("...ac,...nc->...na", T[..., :3, :3], p) + T[..., None, :3, 3]


def symmetric_losses(TCO_possible_gt, TCO_pred, points):
    """l [B, S] = mean over points and components of |T_pred p - T_gt,s p|."""
    d = transform(TCO_pred, points)[:, None] - transform(TCO_possible_gt, points)
    return np.abs(d).reshape(d.shape[0], d.shape[1], -1).mean(-1)


def loss_co_symmetric(TCO_possible_gt, TCO_pred, points):
    l = symmetric_losses(TCO_possible_gt, TCO_pred, points)
    sym_id = l.argmin(1)  # the first minimum
    rows = np.arange(len(l))
    return {"loss": l[rows, sym_id], "sym_id": sym_id, "TCO_assign": np.asarray(TCO_possible_gt, np.float64)[rows, sym_id], "l": l}


def _sign_sums(T_gt, T_pred, points):
    """G [B, 3, 4] = sum_j sign(d_j,a) (p_j,c | 1) / (3N) with d = T_pred p - T_gt p."""
    p = np.asarray(points, np.float64)
    s = np.sign(transform(T_pred, p) - transform(T_gt, p))
    ph = np.concatenate([p, np.ones_like(p[..., :1])], -1)
    return np.einsum("bna,bnc->bac", s, ph) / (3 * p.shape[1])


def grad_co_symmetric(TCO_possible_gt, TCO_pred, points, sym_id, upstream):
    """Gradient with respect to TCO_pred [B, 4, 4] (last row zero)."""
    gt = np.asarray(TCO_possible_gt, np.float64)[np.arange(len(sym_id)), sym_id]
    out = np.zeros((len(sym_id), 4, 4))
    out[:, :3] = _sign_sums(gt, TCO_pred, points) * np.asarray(upstream, np.float64)[:, None, None]
    return out


def ortho6d(o6):
    xr, yr = o6[:, :3], o6[:, 3:6]
    nx = np.linalg.norm(xr, axis=1, keepdims=True)
    x = xr / nx
    zu = np.cross(x, yr)
    nz = np.linalg.norm(zu, axis=1, keepdims=True)
    z = zu / nz
    y = np.cross(z, x)
    return np.stack([x, y, z], -1), (x, z, yr, nx, nz)


def refiner_poses(TCO_possible_gt, TCO_input, refiner_outputs, K_crop, tCR=None):
    """The three predicted poses P [B, 3, 4, 4] (orientation, xy, z) and what the chain rule needs."""
    gt = np.asarray(TCO_possible_gt, np.float64)[:, 0]
    Ti = np.asarray(TCO_input, np.float64)
    o = np.asarray(refiner_outputs, np.float64)
    K = np.asarray(K_crop, np.float64)
    Rg, tg, Rin, ti = gt[:, :3, :3], gt[:, :3, 3], Ti[:, :3, :3], Ti[:, :3, 3]
    fxy = np.stack([K[:, 0, 0], K[:, 1, 1]], 1)
    dR, gs = ortho6d(o[:, :6])
    if tCR is not None:
        tr = np.asarray(tCR, np.float64)
        q = np.einsum("bac,bc->ba", Rg @ Rin.transpose(0, 2, 1), ti - tr)
        vz_gt = (tg[:, 2] - q[:, 2]) / tr[:, 2]
        ztgt = vz_gt * tr[:, 2]
        txy = q[:, :2] + (o[:, 6:8] / fxy + tr[:, :2] / tr[:, 2:3]) * ztgt[:, None]
        dxy = ztgt[:, None] / fxy
        tz = q[:, 2] + o[:, 8] * tr[:, 2]
        dz = tr[:, 2]
    else:
        txy = (o[:, 6:8] / fxy + ti[:, :2] / ti[:, 2:3]) * tg[:, 2:3]
        dxy = tg[:, 2:3] / fxy
        tz = o[:, 8] * ti[:, 2]
        dz = ti[:, 2]
    P = np.repeat(gt[:, None], 3, 1).copy()
    P[:, 0, :3, :3] = dR @ Rin
    P[:, 1, :2, 3] = txy
    P[:, 2, 2, 3] = tz
    return P, {"Rin": Rin, "gs": gs, "dxy": dxy, "dz": dz}


def loss_refiner(TCO_possible_gt, TCO_input, refiner_outputs, K_crop, points, tCR=None):
    P, _ = refiner_poses(TCO_possible_gt, TCO_input, refiner_outputs, K_crop, tCR)
    l = np.stack([symmetric_losses(TCO_possible_gt, P[:, t], points) for t in range(3)], 1)  # [B, 3, S]
    sym_ids = l.argmin(2)
    parts = np.take_along_axis(l, sym_ids[..., None], 2)[..., 0]
    return {"loss": parts[:, 0] + parts[:, 1] + parts[:, 2], "parts": parts, "sym_ids": sym_ids, "l": l, "P": P}


def chain(G_orn, s_xy, s_z, c):
    """The analytic chain from the sums to the nine outputs, split by term: [B, 3, 9].  G_orn [B, 3, 3] = dL/dR_pred of the
    orientation term, s_xy [B, 2] = dL/dt_x, dL/dt_y of the xy term, s_z [B] = dL/dt_z of the z term."""
    x, z, yr, nx, nz = c["gs"]
    gd = G_orn @ c["Rin"].transpose(0, 2, 1)  # dL/d dR; dR = [x y z] as columns
    gx, gy, gz = gd[:, :, 0], gd[:, :, 1], gd[:, :, 2]
    gz = gz + np.cross(x, gy)  # y = z cross x
    gx = gx + np.cross(gy, z)
    gzu = (gz - z * (z * gz).sum(1, keepdims=True)) / nz  # z = zu / |zu|
    gx = gx + np.cross(yr, gzu)  # zu = x cross yr
    gyr = np.cross(gzu, x)
    gxr = (gx - x * (x * gx).sum(1, keepdims=True)) / nx  # x = xr / |xr|
    out = np.zeros((len(G_orn), 3, 9))
    out[:, 0, :3], out[:, 0, 3:6] = gxr, gyr
    out[:, 1, 6:8] = s_xy * c["dxy"]
    out[:, 2, 8] = s_z * c["dz"]
    return out


def grad_refiner(TCO_possible_gt, TCO_input, refiner_outputs, K_crop, points, tCR, sym_ids, upstream):
    """Gradient with respect to refiner_outputs split by term, [B, 3, 9], times the upstream gradient; the total is its sum over
    the terms."""
    P, c = refiner_poses(TCO_possible_gt, TCO_input, refiner_outputs, K_crop, tCR)
    gt = np.asarray(TCO_possible_gt, np.float64)
    rows = np.arange(len(gt))
    G = [_sign_sums(gt[rows, sym_ids[:, t]], P[:, t], points) for t in range(3)]
    return chain(G[0][:, :, :3], G[1][:, :2, 3], G[2][:, 2, 3], c) * np.asarray(upstream, np.float64)[:, None, None]


def chain_max(TCO_possible_gt, TCO_input, refiner_outputs, K_crop, tCR):
    """Largest absolute entry of each row's chain: of d(output gradient) / d(one of the twelve sums)."""
    _, c = refiner_poses(TCO_possible_gt, TCO_input, refiner_outputs, K_crop, tCR)
    b = len(c["Rin"])
    best = np.zeros(b)
    for k in range(12):
        e = np.zeros((b, 12))
        e[:, k] = 1.0
        best = np.maximum(best, np.abs(chain(e[:, :9].reshape(b, 3, 3), e[:, 9:11], e[:, 11], c)).max((1, 2)))
    return best


def feeding_differences(TCO_possible_gt, preds, points, sym_ids, kind):
    """|d| of every difference component that feeds a gradient, [B, n]: preds [B, T, 4, 4], sym_ids [B, T]."""
    gt = np.asarray(TCO_possible_gt, np.float64)
    rows = np.arange(len(gt))
    cols = []
    for t, comps in FEEDS[kind]:
        d = transform(preds[:, t], points) - transform(gt[rows, sym_ids[:, t]], points)
        cols.append(np.abs(d[:, :, list(comps)]).reshape(len(gt), -1))
    return np.concatenate(cols, 1)


def sign_flip_tau(case_inputs):
    """16 * 2^-23 * (largest coordinate magnitude of the case): the float32 rounding of two transformed points."""
    big = max(float(np.abs(transform(case_inputs["TCO_possible_gt"], case_inputs["points"])).max()),
              float(np.abs(transform(case_inputs["TCO_input"], case_inputs["points"])).max()))
    return 16 * 2.0 ** -23 * big


def allowance(k, points, chain_largest, upstream):
    """Sign-flip allowance of a row's gradient: k * 2 * max(|p|, 1) / (3N) times the largest absolute entry of the row's chain
    (times the row's upstream gradient, which scales the row)."""
    p = np.abs(np.asarray(points, np.float64)).reshape(len(points), -1).max(1)
    return k * 2 * np.maximum(p, 1.0) / (3 * np.asarray(points).shape[1]) * chain_largest * np.abs(upstream)
