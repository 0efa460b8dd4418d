"""Reference of the pose geometry kernels (csrc/geometry.hip with csrc/look_at.h: ``hp_pose_prep``, ``hp_pose_prep_views``,
``hp_pose_update``, ``hp_tco_init_autodepth``), written from the definitions those files cite -- ``normalize_T`` (Gram-Schmidt on
the first two columns, TB/lib3d/transform_ops.py:107-120, rotations.py:22-36), the look-at views of ``make_TCO_multiview``
(TB/lib3d/multiview.py:28-92, 166-251), ``invert_transform_matrices(TC0_CV) @ TCO`` (transform_ops.py:59-67),
``project_points_robust`` (camera_geometry.py:40-56), ``deepim_boxes`` (cropping.py:27-75), ``get_K_crop_resize``
(camera_geometry.py:70-122), ortho6d + ``pose_update_with_reference_point`` (cosypose_ops.py:34-62) and ``_autodepth``
(cosypose_ops.py:184-283) -- in float64 NumPy.  Nothing here is translated from a kernel, nothing needs torch and nothing comes from
``oracle.geometry``, which rounds to float32 on the way (tests/test_geometry_reference.py cross-checks the two).

The inputs are float32 arrays and therefore exact; every operation on them is float64.  Three constants belong to the DEFINITION as
float32 values, because the reference applies Python floats to float32 tensors: the ``z_min = 0.1`` of the robust projection, the
``lamb`` of deepim_boxes and its aspect ratio ``r = max(im) / min(im)``.

Non-finite values follow IEEE arithmetic and the reference's ``min`` / ``max``, which PROPAGATE a NaN (torch's do): matrix products
add every term (``0 * NaN`` is NaN), so a non-finite entry of a pose spreads over its column of ``TCV_O`` and from there over the
boxes and the crop intrinsics.  Two rules are the project's own, not the reference's (its Panda3D look-at has none): a pose with a
non-finite entry among its 16 gets the identity as the camera of every look-at view, and an image / object / box / rotation id
outside its table makes every output of that hypothesis NaN.  The exactly degenerate look-at (reference point on camera 0's y axis)
divides 0 by 0: the look-at views of that hypothesis are NaN, as csrc/look_at.h documents.

The case tables are at the end: one per entry point, each case a named read-only record whose ``doc`` says which path it is there
for; tests/test_geometry_reference.py proves on the CPU that every case reaches that path."""

import functools

import numpy as np

from happypose_amd.mesh_store import pad_stack_points, sample_point_ids

F = np.float32
D = np.float64
Z_MIN = float(F(0.1))
VIEW_OFFSETS = {0: (), 1: ((0, 0, 0),), 3: ((0, 0, 0), (1, 0, 0), (-1, 0, 0)),
                5: ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1))}
MV_NAME = {0: "TCO", 1: "TCO+front_1view", 3: "TCO+front_3views", 5: "TCO+front_5views"}
NAN = float("nan")


def _quiet(fn):
    @functools.wraps(fn)
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    return wrapped


def mm(A, B):
    """Matrix product that adds every term in a fixed order (IEEE: a NaN or ``0 * inf`` anywhere in a row-column pair reaches the
    element), whatever the BLAS behind ``@`` does with zeros."""
    A, B = np.asarray(A, D), np.asarray(B, D)
    with np.errstate(all="ignore"):
        out = A[..., :, 0, None] * B[..., 0, None, :]
        for k in range(1, A.shape[-1]):
            out = out + A[..., :, k, None] * B[..., k, None, :]
    return out


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _norm(a):
    return np.sqrt((a * a).sum(-1, keepdims=True))


@_quiet
def ortho6d(x_raw, y_raw):
    """compute_rotation_matrix_from_ortho6d: columns (x, y, z) of ``[..., 3, 3]``."""
    x_raw, y_raw = np.asarray(x_raw, D), np.asarray(y_raw, D)
    x = x_raw / _norm(x_raw)
    z = _cross(x, y_raw)
    z = z / _norm(z)
    return np.stack([x, _cross(z, x), z], -1)


def normalize_T(T):
    T = np.asarray(T, D)
    out = np.zeros(T.shape, D)
    out[..., :3, :3] = ortho6d(T[..., :3, 0], T[..., :3, 1])
    out[..., :3, 3] = T[..., :3, 3]
    out[..., 3, 3] = 1.0
    return out


@_quiet
def look_at(pos, tgt):
    """Pose (camera -> camera 0, OpenCV axes) of a camera at ``pos`` whose +z looks at ``tgt`` with camera 0's up (0, -1, 0) as the
    hint: forward exact, right = f x up, up' = right x f; columns right, -up', forward.  Returns ``(M [4,4], |f x up|)``."""
    f = np.asarray(tgt, D) - np.asarray(pos, D)
    f = f / np.sqrt(f @ f)
    r = _cross(f, np.array([0.0, -1.0, 0.0]))
    nr = np.sqrt(r @ r)
    r = r / nr
    u = _cross(r, f)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = r, -u, f, pos
    return M, float(nr)


@_quiet
def views_TC0_CV(T, mv):
    """Cameras of the look-at views of one pose ``T [4,4]`` (float64) w.r.t. camera 0 -> ``([n,4,4], smallest |f x up| met)``; the
    offsets are in the Panda frame of camera 0 re-aimed at the reference point (x right = cv x, y forward = cv z, z up = -cv y)."""
    n = len(VIEW_OFFSETS[mv])
    tcr = T[:3, 3]
    radius = float(np.sqrt(tcr @ tcr))
    if not np.isfinite(T).all() or radius == 0.0:
        return np.tile(np.eye(4), (n, 1, 1)), NAN
    base, worst = look_at(np.zeros(3), tcr)
    out = []
    for ox, oy, oz in VIEW_OFFSETS[mv]:
        pos = radius * (ox * base[:3, 0] + oy * base[:3, 2] - oz * base[:3, 1])
        M, nr = look_at(pos, tcr)
        worst = min(worst, nr) if nr == nr else worst
        out.append(M)
    return np.array(out, D).reshape(n, 4, 4), worst


def invert_T(T):
    T = np.asarray(T, D)
    out = T.copy()
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -mm(Rt, T[..., :3, 3:4])[..., 0]
    return out


@_quiet
def project_box(P, pts):
    """``P [3,4]``, ``pts [n,3]`` -> ``(box [4], uv [n,2], raw z [n])``: z clamped to 0.1 from below, NaN kept."""
    suv = mm(pts, P[:, :3].T) + P[:, 3]
    z = np.maximum(Z_MIN, suv[:, 2])
    uv = suv[:, :2] / z[:, None]
    return np.array([uv[:, 0].min(), uv[:, 1].min(), uv[:, 0].max(), uv[:, 1].max()]), uv, suv[:, 2]


@_quiet
def deepim_box(center, box, lamb, im_size, r=None):
    xc, yc = center
    r = float(F(max(im_size) / min(im_size))) if r is None else r
    xdist = np.maximum(abs(box[0] - xc), abs(box[2] - xc))
    ydist = np.maximum(abs(box[1] - yc), abs(box[3] - yc))
    w = np.maximum(xdist, ydist * r) * 2 * float(F(lamb))
    h = np.maximum(xdist / r, ydist) * 2 * float(F(lamb))
    return np.array([xc - w / 2, yc - h / 2, xc + w / 2, yc + h / 2])


@_quiet
def K_crop_resize(K, box, crop_size):
    """get_K_crop_resize for one box -> ``(new K [3,3], (scale_x, scale_y))``."""
    fw, fh = float(max(crop_size)), float(min(crop_size))
    cw, ch = box[2] - box[0], box[3] - box[1]
    cj, ci = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2
    cx, cy = K[0, 2] + (cw - 1) / 2 - cj, K[1, 2] + (ch - 1) / 2 - ci
    ocx, ocy = cx - (cw - 1) / 2, cy - (ch - 1) / 2
    sx, sy = fw / cw, fh / ch
    out = np.array(K, D)
    out[0, 0], out[1, 1] = sx * K[0, 0], sy * K[1, 1]
    out[0, 2], out[1, 2] = (fw - 1) / 2 + sx * ocx, (fh - 1) / 2 + sy * ocy
    return out, (sx, sy)


def _bad(i, n):
    return not 0 <= int(i) < n


# ------------------------------------------------------------------------------------------------- hp_pose_prep / hp_pose_prep_views
def ref_pose_prep(case, mutate=None):
    """-> dict of float64 arrays: ``TCO [b,4,4]``, ``tCR [b,3]``, ``TCV_O [b,V,4,4]``, ``boxes_rend [b,4]``, ``boxes_crop [b,4]``, ``K_crop
    [b,V,3,3]``, ``K_crop_main [b,3,3]`` (V: the rendered views), and per EVALUATED view (the identity view first): ``TC0_CV``,
    ``view_boxes`` / ``view_crops [b,nvt,4]``, ``view_scale [b,nvt,2]``, ``uv`` (list of lists of ``[n,2]``), ``z_min`` the smallest raw
    depth of a point, ``cz`` the raw depth of the reference point, and ``cross [b]`` the smallest ``|f x up|`` of the look-ats.
    ``mutate`` names one deliberate mistake (the teeth of tests/test_geometry_reference.py)."""
    b, mv, skip = case.b, case.mv, case.skip
    nvt = 1 + len(VIEW_OFFSETS[mv])
    V = nvt - skip
    table = np.asarray(case.table, D)
    K_all = np.asarray(case.K, D)
    T_in = np.asarray(case.TCO, D)
    Tn = normalize_T(T_in) if case.normalize else T_in.copy()
    ids = [np.asarray(case.ids_main)] + [np.asarray(case.ids_extra)] * (nvt - 1)
    if mutate == "drop_last_point":
        ids[0] = ids[0][:-1]
    if mutate == "drop_wave":
        ids[0] = np.delete(ids[0], np.s_[64:128])
    r = min(case.im_size) / max(case.im_size) if mutate == "r_inverted" and case.im_size[0] > case.im_size[1] else None
    o = dict(TCO=Tn.copy(), tCR=Tn[:, :3, 3].copy(), TCV_O=np.zeros((b, V, 4, 4)), boxes_rend=np.zeros((b, 4)), boxes_crop=np.zeros((b, 4)),
             K_crop=np.zeros((b, V, 3, 3)), K_crop_main=np.zeros((b, 3, 3)), TC0_CV=np.zeros((b, nvt, 4, 4)), view_boxes=np.zeros((b, nvt, 4)),
             view_crops=np.zeros((b, nvt, 4)), view_scale=np.zeros((b, nvt, 2)), uv=[], z_min=np.zeros((b, nvt)), cz=np.zeros((b, nvt)),
             cross=np.full(b, NAN))
    for i in range(b):
        o["uv"].append([])
        if _bad(case.im_ids[i], len(K_all)) or _bad(case.obj_ids[i], len(table)):
            for k in ("TCO", "tCR", "TCV_O", "boxes_rend", "boxes_crop", "K_crop", "K_crop_main", "view_boxes", "view_crops", "z_min", "cz"):
                o[k][i] = NAN
            o["uv"][i] = [None] * nvt
            continue
        K, pts = K_all[case.im_ids[i]], table[case.obj_ids[i]]
        cams, o["cross"][i] = views_TC0_CV(Tn[i], mv)
        o["TC0_CV"][i] = np.concatenate([np.eye(4)[None], cams])
        TV = mm(invert_T(o["TC0_CV"][i]), Tn[i][None])
        Kv = np.zeros((nvt, 3, 3))
        for v in range(nvt):
            P = mm(K, TV[v, :3])
            box, uv, z = project_box(P, pts[ids[v]])
            with np.errstate(all="ignore"):
                cz = np.maximum(Z_MIN, P[2, 3])
                crop = deepim_box((P[0, 3] / cz, P[1, 3] / cz), box, case.lamb, case.im_size, r)
            Kv[v], o["view_scale"][i, v] = K_crop_resize(K, crop, case.crop_size)
            o["view_boxes"][i, v], o["view_crops"][i, v], o["z_min"][i, v], o["cz"][i, v] = box, crop, np.nanmin(z) if np.isfinite(z).any() else NAN, P[2, 3]
            o["uv"][i].append(uv)
        o["boxes_rend"][i], o["boxes_crop"][i] = o["view_boxes"][i, 0], o["view_crops"][i, 0]
        order = list(range(skip, nvt))
        if mutate == "swap_views_2_3":
            order[2 - skip], order[3 - skip] = 3, 2
        o["TCV_O"][i], o["K_crop"][i] = TV[order], Kv[order]
        o["K_crop_main"][i] = Kv[skip] if mutate == "kcrop_main_slot0" else Kv[0]
    return o


# ------------------------------------------------------------------------------------------------------------------ hp_pose_update
@_quiet
def ref_pose_update(case, mutate=None):
    """-> ``TCO_out [b,4,4]`` float64.  ``case.K_crop`` is ``[b,3,3]`` or ``[b,V,3,3]`` (view 0 is the crop's K)."""
    T, p = np.asarray(case.TCO, D), np.asarray(case.pose9, D)
    Kc = np.asarray(case.K_crop, D)
    K0 = Kc.reshape(-1)[: 9 * case.b].reshape(case.b, 3, 3) if mutate == "k_stride_9" else Kc.reshape(case.b, -1)[:, :9].reshape(case.b, 3, 3)
    dR = ortho6d(p[:, 0:3], p[:, 3:6])
    t = T[:, :3, 3]
    tCR = t if case.tCR is None else np.asarray(case.tCR, D)
    zsrc = tCR[:, 2]
    ztgt = p[:, 8] * zsrc
    t_ref = np.stack([(p[:, 6] / K0[:, 0, 0] + tCR[:, 0] / zsrc) * ztgt, (p[:, 7] / K0[:, 1, 1] + tCR[:, 1] / zsrc) * ztgt, ztgt], 1)
    out = T.copy()
    out[:, :3, :3] = mm(dR, T[:, :3, :3])
    out[:, :3, 3] = mm(dR, (t - tCR)[:, :, None])[:, :, 0] + t_ref
    return out


# ----------------------------------------------------------------------------------------------------------- hp_tco_init_autodepth
ZUP = np.array([[0, 1, 0], [0, 0, -1], [-1, 0, 0]], D)


@_quiet
def ref_tco_init(case, mutate=None):
    """-> dict(``TCO [n,4,4]``, ``X``: list of camera-frame points ``[n_points,3]`` at ``z_guess``) float64."""
    n, table = case.n, np.asarray(case.table, D)
    out, Xs = np.zeros((n, 4, 4)), []
    pid = np.arange(table.shape[1]) if case.point_ids is None else np.asarray(case.point_ids)
    for i in range(n):
        bi = i if case.box_ids is None else case.box_ids[i]
        if mutate == "box_ids_ignored":
            bi = min(i, len(case.boxes) - 1)
        ri = i if case.rot_ids is None else case.rot_ids[i]
        if _bad(bi, len(case.boxes)) or _bad(case.im_ids[i], len(case.K)) or _bad(case.obj_ids[i], len(table)) or \
                (case.R is not None and _bad(ri, len(case.R))):
            out[i] = NAN
            Xs.append(None)
            continue
        box, K = np.asarray(case.boxes[bi], D), np.asarray(case.K[case.im_ids[i]], D)
        R = ZUP if case.R is None else np.asarray(case.R[ri], D)
        fxfy, cxcy = np.array([K[0, 0], K[1, 1]]), np.array([K[0, 2], K[1, 2]])
        centre = (box[[0, 1]] + box[[2, 3]]) / 2
        t = np.array([*(((centre - cxcy) * 1.0) / fxfy), 1.0])
        X = mm(table[case.obj_ids[i]][pid], R.T) + t
        delta = X[:, :2].max(0) - X[:, :2].min(0)
        bb = (box[[2, 3]] - box[[0, 1]]) + 1
        z_from = fxfy * delta / bb
        z = (z_from[1] + z_from[0]) / 2
        out[i, :3, :3], out[i, :2, 3], out[i, 2, 3], out[i, 3, 3] = R, ((centre - cxcy) * z) / fxfy, z, 1.0
        Xs.append(X)
    return dict(TCO=out, X=Xs)


# =========================================================================================================================== cases
class Case:
    """A named, read-only record: ``name``, ``doc`` (the path the case is there for) and its inputs as read-only float32 / int32
    arrays."""

    def __init__(self, name, doc, **kw):
        for v in kw.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        object.__setattr__(self, "__dict__", dict(name=name, doc=doc, **kw))

    def __setattr__(self, *a):
        raise AttributeError("cases are read-only")

    def replace(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Case(d.pop("name"), d.pop("doc"), **d)

    def __repr__(self):
        return f"Case({self.name})"


N_PAD = 300
OBJECT_SIZES = (300, 257, 40)  # n_pad = 300 is no multiple of the 256-thread block, and two objects have padded rows


def _object(n, seed):
    rs = np.random.RandomState(seed)
    return (rs.uniform(-1, 1, size=(n, 3)) * np.array([0.09, 0.06, 0.12]) + rs.uniform(-0.01, 0.01, size=3)).astype(F)


@functools.lru_cache(None)
def base_objects():
    """The vertex lists of the three objects (what the mesh store is built from)."""
    return tuple(_object(n, 40 + k) for k, n in enumerate(OBJECT_SIZES))


def table_of(objects):
    """The store's padded point table ``[n_obj, n_pad, 3]`` float32 of a list of vertex arrays."""
    t = pad_stack_points([np.asarray(o, np.float64) for o in objects]).astype(F)
    assert t.shape[1] == N_PAD
    return t


def point_ids(n):
    return sample_point_ids(N_PAD, n).astype(np.int32)


IMAGES = {  # image size, crop size, two K rows with fx != fy and off-centre principal points
    "landscape": ((480, 640), (240, 320), [[[600.0, 0, 312.5], [0, 612.25, 251.0], [0, 0, 1]], [[550.5, 0, 333.25], [0, 540.0, 228.5], [0, 0, 1]]]),
    "portrait": ((640, 480), (320, 240), [[[600.0, 0, 231.5], [0, 612.25, 333.0], [0, 0, 1]], [[550.5, 0, 250.25], [0, 540.0, 309.5], [0, 0, 1]]]),
    "tiny": ((37, 53), (16, 24), [[[50.0, 0, 25.5], [0, 51.25, 19.0], [0, 0, 1]], [[45.5, 0, 27.25], [0, 44.0, 17.5], [0, 0, 1]]]),
}


def poses(b, seed, z=(0.5, 1.2), xy=0.15):
    """``[b,4,4]`` float32: a random rotation perturbed by 2 % (so ``normalize`` has work to do), the object in front of the camera."""
    rs = np.random.RandomState(seed)
    T = np.tile(np.eye(4), (b, 1, 1))
    for i in range(b):
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
        T[i, :3, :3] = q * np.sign(np.linalg.det(q))
    T[:, :3, :3] += 0.02 * rs.normal(size=(b, 3, 3))
    T[:, :2, 3] = rs.uniform(-xy, xy, size=(b, 2))
    T[:, 2, 3] = rs.uniform(*z, size=b)
    return T.astype(F)


def _ids(b, n_obj=3):
    """``im_ids = [1, 0, 1, ...]`` and object ids that repeat and are no identity."""
    return ((np.arange(b) + 1) % 2).astype(np.int32), np.array([(2, 0, 1, 1, 2, 0, 0)[i % 7] % n_obj for i in range(b)], np.int32)


def _prep(name, doc, b, mv, *, skip=0, normalize=1, image="landscape", lamb=1.4, n_main=300, n_extra=200, seed=0, T=None, table=None,
          obj_ids=None, odd=None, planted=(), regular=True):
    im_size, crop_size, K = IMAGES[image]
    im_ids, oid = _ids(b)
    T = poses(b, seed) if T is None else np.array(T, F)
    return Case(name, doc, b=b, mv=mv, skip=skip, normalize=normalize, im_size=im_size, crop_size=crop_size, lamb=lamb, K=np.array(K, F),
                im_ids=im_ids, obj_ids=oid if obj_ids is None else np.array(obj_ids, np.int32), TCO=T,
                table=table_of(base_objects()) if table is None else table, ids_main=point_ids(n_main), ids_extra=point_ids(n_extra),
                n_main=n_main, n_extra=n_extra, odd=odd, planted=tuple(planted), regular=regular, image=image)


PLANT_POSITIONS = (0, 63, 64, 255, 256)
MAIN_EDGES = (1, 63, 64, 65, 255, 256, 257, 300)
EXTRA_EDGES = (1, 64, 200)


def plant_positions(n):
    return sorted({j for j in PLANT_POSITIONS if j < n} | {n - 1})


def _plant_main(n, mv):
    """One hypothesis and one object (300 vertices, no padding) per planted position: the vertex at position ``pos[k]`` of the id list
    is the top-left corner of the box (x1, y1), the one at ``pos[k + 1]`` the bottom-right (x2, y2); with one position the only point
    is all four."""
    pos = plant_positions(n)
    b = len(pos)
    T = poses(b, 100 + n)
    Rn = normalize_T(T)[:, :3, :3]
    ids = point_ids(n)
    objs, planted = [], []
    for k in range(b):
        o = np.array(base_objects()[0])
        ja, jb = pos[k], pos[(k + 1) % b]
        o[ids[ja]] = (Rn[k].T @ np.array([-0.35, -0.30, 0.0])).astype(F)
        planted += [(k, 0, 0, ja), (k, 0, 1, ja)]
        if jb != ja:
            o[ids[jb]] = (Rn[k].T @ np.array([0.30, 0.35, 0.0])).astype(F)
        planted += [(k, 0, 2, jb), (k, 0, 3, jb)]
        objs.append(o)
    return _prep(f"plant_main_{n}", f"n_points_main = {n}: box corners planted at positions {pos} of the id list (lane, wave and loop-tail edges)",
                 b, mv, n_main=n, n_extra=64, T=T, table=table_of(objs), obj_ids=np.arange(b), planted=planted)


def _plant_extra(n, mv, skip):
    """As _plant_main for the 200-point list of the look-at views: hypothesis ``k`` plants one coordinate of the box of one view."""
    pos = plant_positions(n)
    b = len(pos)
    T = poses(b, 200 + n)
    Tn = normalize_T(T)
    ids = point_ids(n)
    nvt = 1 + len(VIEW_OFFSETS[mv])
    objs, planted = [], []
    for k in range(b):
        v = nvt - 1 - k % (nvt - 1)  # the last views first: 5 and 4 of the five-view type
        coord = k % 4
        cam = views_TC0_CV(Tn[k], mv)[0][v - 1]
        TV = mm(invert_T(cam), Tn[k])
        d = np.array([(-0.4, 0, 0), (0, -0.4, 0), (0.4, 0, 0), (0, 0.4, 0)][coord], D)
        o = np.array(base_objects()[0])
        o[ids[pos[k]]] = (TV[:3, :3].T @ d).astype(F)
        planted.append((k, v, coord, pos[k]))
        objs.append(o)
    return _prep(f"plant_extra_{n}", f"n_points_extra = {n} != n_points_main: one box coordinate of a look-at view planted at positions {pos}",
                 b, mv, skip=skip, n_main=300, n_extra=n, T=T, table=table_of(objs), obj_ids=np.arange(b), planted=planted)


def _odd_pose(kind, seed):
    """A batch of 3 whose hypothesis 1 is the odd one; ``plain`` is the same batch with a regular pose there."""
    T = poses(3, seed)
    plain = T.copy()
    if kind == "nan_rot":
        T[1, 1, 1] = np.nan
    elif kind == "inf_trans":
        T[1, 0, 3] = np.inf
    elif kind == "nan_bottom":
        T[1, 3, 2] = np.nan
    elif kind in ("deg_up", "deg_down"):
        T[1, :3, 3] = (0.0, -0.75 if kind == "deg_up" else 0.75, 0.0)
    return T, plain


@functools.lru_cache(None)
def _prep_table():
    c = [
        _prep("tco_b1", "single view, one hypothesis, normalize", 1, 0, seed=1),
        _prep("tco_b65_raw", "single view, 65 hypotheses, normalize = 0, lamb = 1.0, 257 points (a second pass of one lane)", 65, 0, normalize=0,
              lamb=1.0, n_main=257, seed=2),
        _prep("front1_b3", "TCO+front_1view: the re-aimed camera 0 alone", 3, 1, seed=3),
        _prep("front3_b65_portrait", "TCO+front_3views on a portrait image and crop, n_points 256 / 64", 65, 3, image="portrait", n_main=256,
              n_extra=64, seed=4),
        _prep("front5_b3_tiny", "TCO+front_5views (views 4 and 5: above, below) on a 37x53 image, n_points 255 / 1", 3, 5, image="tiny", n_main=255,
              n_extra=1, seed=5),
        _prep("front5_b65", "the largest launch: 65 hypotheses x 6 views x 300 / 200 points", 65, 5, seed=6),
        _prep("skip3_b3", "remove_TCO_rendering with 3 rendered views: slot = v - 1, K_crop_main", 3, 3, skip=1, seed=7),
        _prep("skip5_b65_raw_portrait", "remove_TCO_rendering with 5 views, normalize = 0, lamb = 1.0, portrait", 65, 5, skip=1, normalize=0, lamb=1.0,
              image="portrait", n_main=65, n_extra=64, seed=8),
        _prep("skip3_b3_tiny", "remove_TCO_rendering on the 37x53 image with its landscape 16x24 crop", 3, 3, skip=1, image="tiny", n_main=63, seed=9),
        _prep("behind_b3", "points behind the camera plane: raw depth below 0.1 is clamped", 3, 3, T=poses(3, 10, z=(0.12, 0.2), xy=0.05), seed=10),
        _prep("ref_behind_b3", "reference point with z < 0.1 (0.05, 0.02 and -0.3): cz is clamped, in the look-at views too where |tCR| < 0.1", 3, 3,
              T=_with_z(poses(3, 11, xy=0.02), (0.05, 0.02, -0.3))),
    ]
    for n in MAIN_EDGES:
        c.append(_plant_main(n, 3 if n in (64, 300) else 0))
    c += [_plant_extra(1, 3, 0), _plant_extra(64, 3, 1), _plant_extra(200, 5, 0)]
    for kind, doc, mv, skip, normalize in (
            ("nan_rot", "a NaN rotation entry, normalize = 0: identity look-at, NaN boxes where the reference's min / max propagate", 5, 0, 0),
            ("inf_trans", "an infinite translation, normalize = 1, remove_TCO_rendering", 3, 1, 1),
            ("nan_bottom", "a NaN in the bottom row, normalize = 0: non-finite only among entries 12..15", 3, 0, 0),
            ("deg_up", "exactly degenerate look-at, tCR = (0, -r, 0): the look-at views are NaN", 3, 0, 1),
            ("deg_down", "exactly degenerate look-at, tCR = (0, +r, 0), remove_TCO_rendering", 3, 1, 1)):
        T, plain = _odd_pose(kind, 20 + len(c))
        c.append(_prep(kind, doc, 3, mv, skip=skip, normalize=normalize, T=T, odd=(1, kind, plain), regular=False))
    return {k.name: k for k in c}


def _with_z(T, z):
    T = T.copy()
    T[:, 2, 3] = z
    return T


PREP_CASES = ("tco_b1", "tco_b65_raw", "front1_b3", "front3_b65_portrait", "front5_b3_tiny", "front5_b65", "skip3_b3", "skip5_b65_raw_portrait",
              "skip3_b3_tiny", "behind_b3", "ref_behind_b3") + tuple(f"plant_main_{n}" for n in MAIN_EDGES) + \
    tuple(f"plant_extra_{n}" for n in EXTRA_EDGES) + ("nan_rot", "inf_trans", "nan_bottom", "deg_up", "deg_down")
PREP_REGULAR = tuple(n for n in PREP_CASES if n not in ("nan_rot", "inf_trans", "nan_bottom", "deg_up", "deg_down"))
PREP_ODD = ("nan_rot", "inf_trans", "nan_bottom", "deg_up", "deg_down")
# device-resident ids outside their tables, (table, value): 2 K rows and 3 objects
PREP_BAD_IDS = (("im_ids", 2), ("im_ids", -1), ("obj_ids", 3), ("obj_ids", -5))


def prep_case(name):
    return _prep_table()[name]


def prep_bad_id_case(field, value):
    """``skip3_b3`` with hypothesis 1's id replaced."""
    base = prep_case("skip3_b3")
    ids = np.array(getattr(base, field))
    ids[1] = value
    return base.replace(name=f"bad_{field}_{value}", doc=f"{field}[1] = {value}: outside its table", regular=False, **{field: ids}), base


@functools.lru_cache(None)
def prep_ref(name):
    return ref_pose_prep(prep_case(name))


# ------------------------------------------------------------------------------------------------------------ pose_update cases
def _update(name, doc, b, seed, *, views=0, tcr="offset", bottom=False, collinear=False):
    rs = np.random.RandomState(seed)
    T = poses(b, seed)
    if bottom:
        T[:, 3] = rs.uniform(-0.5, 2.0, size=(b, 4)).astype(F)
    p = np.zeros((b, 9))
    p[:, :3] = rs.normal(size=(b, 3)) * rs.uniform(0.5, 4.0, size=(b, 1))  # no unit vector
    p[:, 3:6] = rs.normal(size=(b, 3)) * rs.uniform(0.5, 4.0, size=(b, 1))
    if collinear:  # y_raw 0.2 rad off x_raw: nearly collinear, away from exactly
        w = np.cross(p[:, :3], rs.normal(size=(b, 3)))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        x = p[:, :3] / np.linalg.norm(p[:, :3], axis=1, keepdims=True)
        p[:, 3:6] = 1.7 * (np.cos(0.2) * x + np.sin(0.2) * w)
    p[:, 6:8] = rs.uniform(-8, 8, size=(b, 2))
    p[:, 8] = rs.uniform(0.8, 1.25, size=b)
    Kc = np.tile(np.array([[1100.0, 0, 160.0], [0, 1080.0, 120.0], [0, 0, 1]]), (b, 1, 1))
    Kc[:, 0, 0] *= rs.uniform(0.5, 2, size=b)
    Kc[:, 1, 1] *= rs.uniform(0.5, 2, size=b)
    if views:
        full = np.full((b, views, 3, 3), 7.0)  # the other views hold a sentinel that would show if read
        full[:, 0] = Kc
        Kc = full
    t = T[:, :3, 3]
    tCR = {"null": None, "equal": t.copy(), "offset": (t + rs.uniform(-0.05, 0.05, size=(b, 3))).astype(F)}[tcr]
    return Case(name, doc, b=b, TCO=T, K_crop=Kc.astype(F), pose9=p.astype(F), tCR=tCR, views=views)


@functools.lru_cache(None)
def _update_table():
    c = [
        _update("k33_offset_b1", "K_crop [b,3,3], tCR off the translation (the d term), one hypothesis", 1, 31),
        _update("k33_null_b3", "tCR null: the translation is the reference point", 3, 32, tcr="null"),
        _update("k33_equal_b65", "tCR equal to the translation, b = 65: a second, partly idle 64-thread block", 65, 33, tcr="equal"),
        _update("k4x33_offset_b65", "K_crop as view 0 of [b,4,3,3] (k_stride 36), the other views hold 7", 65, 34, views=4),
        _update("bottom_row_b3", "a bottom row that is not 0 0 0 1: copied", 3, 35, bottom=True, views=4),
        _update("collinear_b65", "non-unit, nearly collinear 6d part (0.2 rad)", 65, 36, collinear=True, tcr="null"),
    ]
    return {k.name: k for k in c}


UPDATE_CASES = ("k33_offset_b1", "k33_null_b3", "k33_equal_b65", "k4x33_offset_b65", "bottom_row_b3", "collinear_b65")


def update_case(name):
    return _update_table()[name]


# --------------------------------------------------------------------------------------------------------------- tco_init cases
def _rotations(n, seed):
    return normalize_T(poses(n, seed))[:, :3, :3].astype(F)


def _init(name, doc, n, seed, *, R=None, n_boxes=None, box_ids=False, rot_ids=False, n_points=None, table=None, obj_ids=None, planted=()):
    rs = np.random.RandomState(seed)
    nb = n if n_boxes is None else n_boxes
    x1, y1 = rs.uniform(40, 300, size=nb), rs.uniform(30, 200, size=nb)
    boxes = np.stack([x1, y1, x1 + rs.uniform(40, 250, size=nb), y1 + rs.uniform(40, 200, size=nb)], 1).astype(F)
    im_ids, oid = _ids(n)
    Rt = None if R is None else _rotations(R, seed + 1)
    return Case(name, doc, n=n, boxes=boxes, K=np.array(IMAGES["landscape"][2], F), im_ids=im_ids,
                obj_ids=oid if obj_ids is None else np.array(obj_ids, np.int32), R=Rt,
                box_ids=(np.arange(n)[::-1] % nb).astype(np.int32) if box_ids else None,
                rot_ids=((np.arange(n) * 2 + 1) % R).astype(np.int32) if rot_ids else None,
                point_ids=None if n_points is None else point_ids(n_points), n_points=n_points,
                table=table_of(base_objects()) if table is None else table, planted=tuple(planted))


def _plant_init(n):
    """As _plant_main: the extreme camera-frame x / y of the autodepth, planted at the lane, wave and loop-tail positions."""
    pos = plant_positions(n)
    b = len(pos)
    R = _rotations(b, 300 + n + 1)
    ids = point_ids(n)
    objs, planted = [], []
    for k in range(b):
        o = np.array(base_objects()[0])
        ja, jb = pos[k], pos[(k + 1) % b]
        o[ids[ja]] = (R[k].astype(D).T @ np.array([-0.5, -0.45, 0.0])).astype(F)
        planted += [(k, 0, ja), (k, 1, ja)]
        if jb != ja:
            o[ids[jb]] = (R[k].astype(D).T @ np.array([0.45, 0.5, 0.0])).astype(F)
        planted += [(k, 2, jb), (k, 3, jb)]
        objs.append(o)
    return _init(f"plant_init_{n}", f"n_points = {n}: the extreme points planted at positions {pos} of the id list", b, 300 + n, R=b, n_points=n,
                 table=table_of(objs), obj_ids=np.arange(b), planted=planted)


@functools.lru_cache(None)
def _init_table():
    c = [
        _init("zup_b1", "R null (z-up), no id tables but the required ones, all n_pad rows (the padded ones too)", 1, 51),
        _init("R_b3", "R given, one box and one rotation per hypothesis, 257 points", 3, 52, R=3, n_points=257),
        _init("tables_b65", "2 boxes and 3 rotations feeding 65 hypotheses: box_ids and rot_ids given, tables shorter than n", 65, 53, R=3, n_boxes=2,
              box_ids=True, rot_ids=True, n_points=64),
        _init("box_ids_only_b3", "box_ids given, rot_ids null", 3, 54, R=3, n_boxes=2, box_ids=True, n_points=200),
        _init("rot_ids_only_b3", "rot_ids given, box_ids null, point_ids null", 3, 55, R=2, rot_ids=True),
        _init("zup_box_ids_b65", "R null with box_ids: 65 hypotheses share 2 boxes", 65, 56, n_boxes=2, box_ids=True),
    ] + [_plant_init(n) for n in MAIN_EDGES]
    return {k.name: k for k in c}


INIT_CASES = ("zup_b1", "R_b3", "tables_b65", "box_ids_only_b3", "rot_ids_only_b3", "zup_box_ids_b65") + tuple(f"plant_init_{n}" for n in MAIN_EDGES)
# (table, value) of hypothesis 1 of ``tables_b65``: 2 boxes, 2 K rows, 3 rotations, 3 objects
INIT_BAD_IDS = (("box_ids", 2), ("box_ids", -1), ("im_ids", 2), ("im_ids", -7), ("rot_ids", 3), ("rot_ids", -1), ("obj_ids", 3), ("obj_ids", -2))


def init_case(name):
    return _init_table()[name]


def init_bad_id_case(field, value):
    base = init_case("tables_b65")
    ids = np.array(getattr(base, field))
    ids[1] = value
    return base.replace(name=f"bad_{field}_{value}", doc=f"{field}[1] = {value}: outside its table", **{field: ids}), base
