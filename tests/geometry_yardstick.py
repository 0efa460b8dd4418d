"""Yardsticks of the pose geometry kernels' GPU tests: how far a float32 evaluation of each definition lies from the float64
reference (tests/geometry_ref.py), and the comparison functions the GPU tests use.  Unlike the reference this module knows the order
in which the kernels of geometry.hip operate: no multiply and add is contracted except the ``fmaf`` chains as written (``K @ TV``, the
projection, ``dR @ T``, ``R p``), and the look-at of the extra views is evaluated in double and rounded once (it is taken from the
reference: its input, the translation, is the same float32 value).  Nothing here is compared with a kernel, it only sizes the bounds:
every figure of MEASURED_F32_ERROR is measured over the whole case table and asserted by tests/test_geometry_reference.py on the CPU;
tests/test_gpu_geometry.py allows the kernels 4x, for the reasons given in tests/detect_yardstick.py (another order of association,
the device's division and ``sqrtf`` in place of NumPy's).

The scales S the errors are relative to:
* ``prep_R``, ``prep_TCV_R``, ``update_R`` -- rotation entries: 1;
* ``prep_TCV_t`` -- translations of the views: max|t| of the (normalised) pose;
* ``prep_boxes_rend``, ``prep_boxes_crop`` -- pixel boxes: max(image size, |box|) per hypothesis;
* ``prep_K_crop`` -- max(|K_crop|, s x max(|crop box|, |K|)) per view, s the larger of the crop's two scale factors: the principal
  point is ``s x (a difference of box coordinates)``, whose operands are of the second magnitude;
* ``update_t`` -- max(|t|, |tCR|, |t_out|) per hypothesis;
* ``init_t`` -- max(|t_out|, f x max|X| / (box side + 1)) per hypothesis: the depth is f x (a difference of the points' camera
  coordinates X) / the box side.
The copies (tCR, the translation and the bottom row of TCO, the bottom row of TCV_O, the rotation of the initial pose, all of TCO
without ``normalize``) are compared exactly.

Measured (worst |f32 - f64| / S over the tables): prep_R 1.21e-7, prep_TCV_R 1.74e-7, prep_TCV_t 2.07e-7, prep_boxes_rend 1.7e-7,
prep_boxes_crop 2.16e-7, prep_K_crop 1.24e-6, update_R 2.19e-7, update_t 7.59e-8, init_t 1.29e-7.  prep_K_crop is the largest because the focal length
is scaled by ``crop size / (x2 - x1)``: a difference of two box coordinates of some hundred px that is itself about a hundred px."""

import numpy as np

import geometry_ref as R

F = np.float32
D = np.float64
Z32 = F(0.1)


def fma(a, b, c):
    """``fmaf``: the product is exact in double; the double rounding of the sum differs from one rounding in rare ties only."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, D) * np.asarray(b, D) + np.asarray(c, D)).astype(F)


def _gram32(xr, yr):
    """Columns x, y, z from raw x, y ``[..., 3]`` float32 in normalize_T_dev's order."""
    def cross(a, b):
        return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                         a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)

    def norm(a):
        return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])[..., None]

    with np.errstate(all="ignore"):
        x = xr / norm(xr)
        z = cross(x, yr)
        z = z / norm(z)
        y = cross(z, x)
    assert x.dtype == F and y.dtype == F and z.dtype == F
    return x, y, z


def _normalize32(T):
    x, y, z = _gram32(T[:3, 0], T[:3, 1])
    out = np.zeros((4, 4), F)
    out[:3, 0], out[:3, 1], out[:3, 2], out[:3, 3], out[3, 3] = x, y, z, T[:3, 3], 1
    return out


def _view32(M, T):
    """view_from_cam0: ``M`` the double look-at pose, ``T [4,4]`` float32."""
    Mf = np.asarray(M, D).astype(F)
    Ri = Mf[:3, :3].T
    with np.errstate(all="ignore"):
        ti = -((Ri[:, 0] * Mf[0, 3] + Ri[:, 1] * Mf[1, 3]) + Ri[:, 2] * Mf[2, 3])
        TV = T.copy()
        TV[:3] = ((Ri[:, 0, None] * T[0] + Ri[:, 1, None] * T[1]) + Ri[:, 2, None] * T[2]) + ti[:, None] * T[3]
    assert TV.dtype == F
    return TV


def _k_crop32(K, box, crop_size):
    fw, fh = F(max(crop_size)), F(min(crop_size))
    one, two = F(1), F(2)
    with np.errstate(all="ignore"):
        cw, ch = box[2] - box[0], box[3] - box[1]
        cj, ci = (box[0] + box[2]) / two, (box[1] + box[3]) / two
        cx, cy = K[0, 2] + (cw - one) / two - cj, K[1, 2] + (ch - one) / two - ci
        ocx, ocy = cx - (cw - one) / two, cy - (ch - one) / two
        sx, sy = fw / cw, fh / ch
        out = K.copy()
        out[0, 0], out[1, 1] = sx * K[0, 0], sy * K[1, 1]
        out[0, 2], out[1, 2] = (fw - one) / two + sx * ocx, (fh - one) / two + sy * ocy
    assert out.dtype == F
    return out


def prep_f32(case, ref):
    """The outputs of hp_pose_prep(_views) in float32, in the kernel's order; hypotheses with an id outside its table are NaN."""
    b, skip = case.b, case.skip
    nvt = 1 + len(R.VIEW_OFFSETS[case.mv])
    V = nvt - skip
    o = dict(TCO=np.full((b, 4, 4), np.nan, F), tCR=np.full((b, 3), np.nan, F), TCV_O=np.full((b, V, 4, 4), np.nan, F),
             boxes_rend=np.full((b, 4), np.nan, F), boxes_crop=np.full((b, 4), np.nan, F), K_crop=np.full((b, V, 3, 3), np.nan, F),
             K_crop_main=np.full((b, 3, 3), np.nan, F))
    ids = [case.ids_main] + [case.ids_extra] * (nvt - 1)
    r = F(max(case.im_size) / min(case.im_size))
    lamb, two = F(case.lamb), F(2)
    for i in range(b):
        if R._bad(case.im_ids[i], len(case.K)) or R._bad(case.obj_ids[i], len(case.table)):
            continue
        K = case.K[case.im_ids[i]]
        T = _normalize32(case.TCO[i]) if case.normalize else np.array(case.TCO[i])
        o["TCO"][i], o["tCR"][i] = T, T[:3, 3]
        for v in range(nvt):
            TV = T if v == 0 else _view32(ref["TC0_CV"][i, v], T)
            p = case.table[case.obj_ids[i]][ids[v]]
            with np.errstate(all="ignore"):
                P = fma(K[:, 2, None], TV[2], fma(K[:, 1, None], TV[1], K[:, 0, None] * TV[0]))
                s = fma(P[:, 2], p[:, 2, None], fma(P[:, 1], p[:, 1, None], P[:, 0] * p[:, 0, None])) + P[:, 3]
                sz = np.maximum(Z32, s[:, 2])
                u, w = s[:, 0] / sz, s[:, 1] / sz
                x1, y1, x2, y2 = u.min(), w.min(), u.max(), w.max()
                cz = np.maximum(Z32, P[2, 3])
                xc, yc = P[0, 3] / cz, P[1, 3] / cz
                xdist, ydist = np.maximum(abs(x1 - xc), abs(x2 - xc)), np.maximum(abs(y1 - yc), abs(y2 - yc))
                width, height = np.maximum(xdist, ydist * r) * two * lamb, np.maximum(xdist / r, ydist) * two * lamb
                crop = np.array([xc - width / two, yc - height / two, xc + width / two, yc + height / two])
            assert crop.dtype == F and u.dtype == F
            Kn = _k_crop32(K, crop, case.crop_size)
            if v >= skip:
                o["TCV_O"][i, v - skip], o["K_crop"][i, v - skip] = TV, Kn
            if v == 0:
                o["boxes_rend"][i], o["boxes_crop"][i], o["K_crop_main"][i] = (x1, y1, x2, y2), crop, Kn
    return o


def update_f32(case):
    T, p, b = case.TCO, case.pose9, case.b
    Kc = case.K_crop.reshape(b, -1)[:, :9].reshape(b, 3, 3)
    x, y, z = _gram32(p[:, 0:3], p[:, 3:6])
    dR = np.stack([x, y, z], -1)
    tc = T[:, :3, 3]
    tr = tc if case.tCR is None else case.tCR
    zsrc = tr[:, 2]
    ztgt = p[:, 8] * zsrc
    tro = np.stack([(p[:, 6] / Kc[:, 0, 0] + tr[:, 0] / zsrc) * ztgt, (p[:, 7] / Kc[:, 1, 1] + tr[:, 1] / zsrc) * ztgt, ztgt], 1)
    d = tc - tr
    out = T.copy()
    out[:, :3, :3] = fma(dR[:, :, 2, None], T[:, 2, None, :3], fma(dR[:, :, 1, None], T[:, 1, None, :3], dR[:, :, 0, None] * T[:, 0, None, :3]))
    out[:, :3, 3] = fma(dR[:, :, 2], d[:, 2, None], fma(dR[:, :, 1], d[:, 1, None], dR[:, :, 0] * d[:, 0, None])) + tro
    assert out.dtype == F
    return out


def init_f32(case):
    n = case.n
    out = np.full((n, 4, 4), np.nan, F)
    pid = np.arange(case.table.shape[1]) if case.point_ids is None else case.point_ids
    one, two = F(1), F(2)
    for i in range(n):
        bi = i if case.box_ids is None else case.box_ids[i]
        ri = i if case.rot_ids is None else case.rot_ids[i]
        if R._bad(bi, len(case.boxes)) or R._bad(case.im_ids[i], len(case.K)) or R._bad(case.obj_ids[i], len(case.table)) or \
                (case.R is not None and R._bad(ri, len(case.R))):
            continue
        box, K = case.boxes[bi], case.K[case.im_ids[i]]
        Rm = R.ZUP.astype(F) if case.R is None else case.R[ri]
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        bcx, bcy = (box[0] + box[2]) / two, (box[1] + box[3]) / two
        tx, ty = ((bcx - cx) * one) / fx, ((bcy - cy) * one) / fy
        p = case.table[case.obj_ids[i]][pid]
        X = fma(Rm[0, 2], p[:, 2], fma(Rm[0, 1], p[:, 1], Rm[0, 0] * p[:, 0])) + tx
        Y = fma(Rm[1, 2], p[:, 2], fma(Rm[1, 1], p[:, 1], Rm[1, 0] * p[:, 0])) + ty
        bdx, bdy = (box[2] - box[0]) + one, (box[3] - box[1]) + one
        zdx, zdy = fx * (X.max() - X.min()) / bdx, fy * (Y.max() - Y.min()) / bdy
        z = (zdy + zdx) / two
        out[i] = np.eye(4, dtype=F)
        out[i, :3, :3] = Rm
        out[i, :3, 3] = (((bcx - cx) * z) / fx, ((bcy - cy) * z) / fy, z)
        assert X.dtype == F and type(z) is F
    return out


# ---------------------------------------------------------------------------------------------------------------------- scales
def _amax(a, axis):
    with np.errstate(all="ignore"):
        return np.nan_to_num(np.abs(np.asarray(a, D)), nan=0.0, posinf=0.0).max(axis)


def prep_scales(case, ref):
    skip = case.skip
    t = _amax(ref["tCR"], 1)
    size = float(max(case.im_size))
    s = _amax(ref["view_scale"], 2)
    kmax = float(np.abs(case.K).max())
    SK = np.maximum(_amax(ref["K_crop"].reshape(case.b, -1, 9), 2), (s * np.maximum(_amax(ref["view_crops"], 2), kmax))[:, skip:])
    SKm = np.maximum(_amax(ref["K_crop_main"].reshape(case.b, 9), 1), s[:, 0] * np.maximum(_amax(ref["view_crops"], 2)[:, 0], kmax))
    return dict(t=t, rend=np.maximum(size, _amax(ref["boxes_rend"], 1)), crop=np.maximum(size, _amax(ref["boxes_crop"], 1)), K=SK, K_main=SKm)


def update_scale(case, ref):
    t = [_amax(case.TCO[:, :3, 3], 1), _amax(ref[:, :3, 3], 1)] + ([] if case.tCR is None else [_amax(case.tCR, 1)])
    return np.max(t, 0)


def init_scale(case, ref):
    S = _amax(ref["TCO"][:, :3, 3], 1)
    for i, X in enumerate(ref["X"]):
        if X is not None:
            bi = i if case.box_ids is None else case.box_ids[i]
            box, K = np.asarray(case.boxes[bi], D), np.asarray(case.K[case.im_ids[i]], D)
            S[i] = max(S[i], K[0, 0] * np.abs(X[:, 0]).max() / (box[2] - box[0] + 1), K[1, 1] * np.abs(X[:, 1]).max() / (box[3] - box[1] + 1))
    return S


# ----------------------------------------------------------------------------------------------------------------- comparisons
class Worst(dict):
    """(kernel, quantity) -> worst ``|got - ref| / (e x S)`` seen."""

    def up(self, key, value):
        self[key] = max(self.get(key, 0.0), float(value))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _exact(what, got, ref):
    """Copies: the finite values equal the reference's float32 value, the others are non-finite together."""
    got, ref = np.asarray(got, D), np.asarray(ref, D)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), (what, "finiteness differs from the reference's")
    assert np.array_equal(got[fin], ref[fin]), (what, "a copied value changed")


def _bound(worst, kernel, quantity, got, ref, scale, key, factor=4.0):
    """``|got - ref| <= factor x e x scale`` where the reference is finite, and the same finiteness mask."""
    got, ref = np.asarray(got, D), np.asarray(ref, D)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), (kernel, quantity, "finiteness differs from the reference's", np.argwhere(np.isfinite(got) != fin)[:4])
    scale = np.broadcast_to(np.asarray(scale, D), ref.shape)
    with np.errstate(all="ignore"):
        ratio = np.where(fin, np.abs(got - ref) / (MEASURED_F32_ERROR[key] * scale), 0.0)
    w = float(ratio.max()) if ratio.size else 0.0
    worst.up((kernel, quantity), w)
    assert w <= factor, (kernel, quantity, w, f"x the float32 yardstick; allowed {factor}", np.unravel_index(ratio.argmax(), ratio.shape))


def check_prep(got, ref, case, worst, skip_keys=()):
    """``got``: dict of arrays as hp_pose_prep(_views) wrote them (a key in ``skip_keys`` is a null output and not looked at)."""
    S = prep_scales(case, ref)
    k = "pose_prep"
    if "TCO" not in skip_keys:
        if case.normalize:
            _bound(worst, k, "TCO rotation", got["TCO"][:, :3, :3], ref["TCO"][:, :3, :3], 1.0, "prep_R")
            _exact("TCO translation", got["TCO"][:, :3, 3], ref["TCO"][:, :3, 3])
            _exact("TCO bottom row", got["TCO"][:, 3], ref["TCO"][:, 3])
        else:
            _exact("TCO", got["TCO"], ref["TCO"])
    if "tCR" not in skip_keys:
        _exact("tCR", got["tCR"], ref["tCR"])
    if "TCV_O" not in skip_keys:
        _bound(worst, k, "TCV_O rotation", got["TCV_O"][..., :3, :3], ref["TCV_O"][..., :3, :3], 1.0, "prep_TCV_R")
        _bound(worst, k, "TCV_O translation", got["TCV_O"][..., :3, 3], ref["TCV_O"][..., :3, 3], S["t"][:, None, None], "prep_TCV_t")
        _exact("TCV_O bottom row", got["TCV_O"][..., 3, :], ref["TCV_O"][..., 3, :])
    if "boxes_rend" not in skip_keys:
        _bound(worst, k, "boxes_rend", got["boxes_rend"], ref["boxes_rend"], S["rend"][:, None], "prep_boxes_rend")
    if "boxes_crop" not in skip_keys:
        _bound(worst, k, "boxes_crop", got["boxes_crop"], ref["boxes_crop"], S["crop"][:, None], "prep_boxes_crop")
    _bound(worst, k, "K_crop", got["K_crop"], ref["K_crop"], S["K"][:, :, None, None], "prep_K_crop")
    if got.get("K_crop_main") is not None:
        _bound(worst, k, "K_crop_main", got["K_crop_main"], ref["K_crop_main"], S["K_main"][:, None, None], "prep_K_crop")


def check_update(got, ref, case, worst):
    _bound(worst, "pose_update", "rotation", got[:, :3, :3], ref[:, :3, :3], 1.0, "update_R")
    _bound(worst, "pose_update", "translation", got[:, :3, 3], ref[:, :3, 3], update_scale(case, ref)[:, None], "update_t")
    _exact("pose_update bottom row", got[:, 3], ref[:, 3])


def check_init(got, ref, case, worst):
    _exact("tco_init rotation", got[:, :3, :3], ref["TCO"][:, :3, :3])
    _exact("tco_init bottom row", got[:, 3], ref["TCO"][:, 3])
    _bound(worst, "tco_init", "translation", got[:, :3, 3], ref["TCO"][:, :3, 3], init_scale(case, ref)[:, None], "init_t")


# ----------------------------------------------------------------------------------------------------------------- measurement
def _err(w, key, got, ref, scale):
    got, ref = np.asarray(got, D), np.asarray(ref, D)
    fin = np.isfinite(ref) & np.isfinite(got)
    scale = np.broadcast_to(np.asarray(scale, D), ref.shape)
    if fin.any():
        with np.errstate(all="ignore"):
            w[key] = max(w[key], float((np.abs(got - ref)[fin] / scale[fin]).max()))


def measure():
    """Worst ``|f32 - f64| / S`` per quantity over every case of geometry_ref's tables."""
    w = {k: 0.0 for k in MEASURED_F32_ERROR}
    for name in R.PREP_CASES:
        case, ref = R.prep_case(name), R.prep_ref(name)
        got, S = prep_f32(case, ref), prep_scales(case, ref)
        _err(w, "prep_R", got["TCO"][:, :3, :3], ref["TCO"][:, :3, :3], 1.0)
        _err(w, "prep_TCV_R", got["TCV_O"][..., :3, :3], ref["TCV_O"][..., :3, :3], 1.0)
        _err(w, "prep_TCV_t", got["TCV_O"][..., :3, 3], ref["TCV_O"][..., :3, 3], S["t"][:, None, None])
        _err(w, "prep_boxes_rend", got["boxes_rend"], ref["boxes_rend"], S["rend"][:, None])
        _err(w, "prep_boxes_crop", got["boxes_crop"], ref["boxes_crop"], S["crop"][:, None])
        _err(w, "prep_K_crop", got["K_crop"], ref["K_crop"], S["K"][:, :, None, None])
        _err(w, "prep_K_crop", got["K_crop_main"], ref["K_crop_main"], S["K_main"][:, None, None])
    for name in R.UPDATE_CASES:
        case = R.update_case(name)
        ref, got = R.ref_pose_update(case), update_f32(case)
        _err(w, "update_R", got[:, :3, :3], ref[:, :3, :3], 1.0)
        _err(w, "update_t", got[:, :3, 3], ref[:, :3, 3], update_scale(case, ref)[:, None])
    for name in R.INIT_CASES:
        case = R.init_case(name)
        ref, got = R.ref_tco_init(case), init_f32(case)
        _err(w, "init_t", got[:, :3, 3], ref["TCO"][:, :3, 3], init_scale(case, ref)[:, None])
    return w


# Worst |f32 - f64| / S over the tables of geometry_ref (see the module docstring for S).
MEASURED_F32_ERROR = {"prep_R": 1.21e-7, "prep_TCV_R": 1.74e-7, "prep_TCV_t": 2.07e-7, "prep_boxes_rend": 1.7e-7, "prep_boxes_crop": 2.16e-7,
                      "prep_K_crop": 1.24e-6, "update_R": 2.19e-7, "update_t": 7.59e-8, "init_t": 1.29e-7}
