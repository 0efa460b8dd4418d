"""NumPy restatement of CosyPose's multi-view candidate matching, in float64 (or any dtype): test infrastructure, the
independent check of ``happypose_amd/csrc/multiview.hip``.  Nothing here is imported by the product.

Reference lines (CP/ = happypose/pose_estimators/cosypose/cosypose/):
  symmetric_distance        CP/lib3d/symmetric_distances.py:36-55   (symmetric_distance_batched_fast)
  reprojected_distance      CP/lib3d/symmetric_distances.py:92-122, CP/lib3d/camera_geometry.py:4-18
  estimate_camera_poses     CP/multiview/ransac.py:23-50, scatter_argmin CP/csrc/cosypose_cext.cpp:220-247
  score_matches             CP/multiview/ransac.py:78-99
  find_inliers              CP/csrc/cosypose_cext.cpp:109-218
Seeds and tentative matches are NOT restated (they depend on the C++ standard library's shuffle): the tests take them from
the golden file, and tests/test_multiview_host.py pins the library's own against it.
"""

import numpy as np

# Largest deviation of the REFERENCE's own float32 run (tests/golden/g11_multiview.npz) from this restatement in float64, over
# scenes A - D; measured and asserted by tests/test_multiview_reference.py::test_reference_float32_error_is_the_recorded_one.
# The GPU kernels (float32, FMA, other summation order) are allowed 4x that (tests/test_gpu_multiview.py).
REF_F32_ERR_DISTS = 3.4573e-07  # metres (scene C; A/B 2.84e-07, D 1.35e-07)
REF_F32_ERR_TC1C2_T = 2.2740e-07  # metres, translation column of TC1C2
REF_F32_ERR_TC1C2_R = 1.1408e-07  # rotation entries of TC1C2
GPU_FACTOR = 4.0
DIST_THRESHOLD = 0.02
N_MIN_INLIERS = 3
SCENES = ("A", "B", "C", "D")
SEED_COLUMNS = ("view1", "view2", "match1_cand1", "match1_cand2", "match2_cand1", "match2_cand2")


def invert(T):
    """TB/lib3d/transform_ops.py:59-67."""
    R, t = T[..., :3, :3], T[..., :3, 3:]
    out = T.copy()
    out[..., :3, :3] = np.swapaxes(R, -1, -2)
    out[..., :3, 3:] = -np.swapaxes(R, -1, -2) @ t
    return out


def transform_pts(T, pts):
    """T [..., 4, 4], pts [..., n, 3] -> [..., n, 3]."""
    return pts @ np.swapaxes(T[..., :3, :3], -1, -2) + T[..., None, :3, 3]


def symmetric_distance(T1, T2, obj, points, symmetries, n_sym=None):
    """(dists [b], sym_ids [b]): argmin over ALL rows of the padded table by mean squared distance (first minimum), value =
    mean of the roots."""
    T1S = T1[:, None] @ symmetries[obj]  # [b, S, 4, 4]
    p = points[obj]
    d2 = ((transform_pts(T1S, p[:, None]) - transform_pts(T2, p)[:, None]) ** 2).sum(-1)  # [b, S, n]
    best = d2.mean(-1).argmin(1)
    ar = np.arange(len(T1))
    return np.sqrt(d2[ar, best]).mean(-1), best


def project(K, T, pts):
    suv = transform_pts(T, pts) @ np.swapaxes(K, -1, -2)
    return suv[..., :2] / suv[..., 2:]


def reprojected_distance(T1, T2, K, obj, points, symmetries, n_sym):
    """symmetric_distance_reprojected: over the object's OWN n_sym symmetries, first strict minimum of the mean pixel distance."""
    dists, ids = np.empty(len(T1), T1.dtype), np.empty(len(T1), np.int64)
    for i in range(len(T1)):
        o = obj[i]
        S = symmetries[o, :n_sym[o]]
        uv1 = project(K[i], T1[i] @ S, points[o][None])
        uv2 = project(K[i], T2[i], points[o])
        d = np.linalg.norm(uv1 - uv2[None], axis=-1).mean(-1)
        ids[i] = d.argmin()
        dists[i] = d[ids[i]]
    return dists, ids


def estimate_camera_poses(poses, obj, seeds, points, symmetries, n_sym):
    """TC1C2 [n_seeds, 4, 4] and the chosen symmetry of object a."""
    a, b, g, d = (seeds[k] for k in SEED_COLUMNS[2:])
    out, chosen = np.empty((len(a), 4, 4), poses.dtype), np.empty(len(a), np.int64)
    TObC2 = invert(poses)
    for n in range(len(a)):
        S = symmetries[obj[a[n]], :n_sym[obj[a[n]]]]
        T2 = ((poses[a[n]] @ S) @ TObC2[b[n]]) @ poses[d[n]]
        ns = len(S)
        dists, _ = symmetric_distance(np.repeat(poses[g[n]][None], ns, 0), T2, np.repeat(obj[g[n]], ns), points, symmetries)
        chosen[n] = dists.argmin()  # first minimum == scatter_argmin's first strict minimum
        out[n] = poses[a[n]] @ S[chosen[n]] @ TObC2[b[n]]
    return out, chosen


def score_matches(poses, obj, tmatches, TC1C2, points, symmetries):
    h, c1, c2 = tmatches
    return symmetric_distance(poses[c1], TC1C2[h] @ poses[c2], obj[c1], points, symmetries)[0]


def find_inliers(view1, view2, tmatches, dists, dist_threshold=DIST_THRESHOLD, n_min_inliers=N_MIN_INLIERS, details=False):
    """-> (inlier_cand1, inlier_cand2, best_hypotheses[, per-hypothesis (n_inliers, dists_sum)])."""
    h, c1, c2 = tmatches
    dists = np.asarray(dists, np.float32)
    n_hyp = len(view1)
    rows = [[] for _ in range(n_hyp)]
    for n in range(len(h)):
        if dists[n] <= np.float32(dist_threshold):
            rows[h[n]].append(n)
    uniq, stats = [], []
    for hyp in range(n_hyp):
        r = sorted(rows[hyp], key=lambda n: dists[n])  # stable
        u1, u2, keep, total = set(), set(), [], np.float32(0)
        for n in r:
            if c1[n] not in u1 and c2[n] not in u2:
                u1.add(c1[n]); u2.add(c2[n]); keep.append(n)
                total = np.float32(total + dists[n])
        uniq.append(keep)
        stats.append((len(keep), float(total)))
    pairs = sorted(set(zip(view1.tolist(), view2.tolist())))
    in1, in2, best_all = [], [], []
    for pair in pairs:
        best, best_n, best_sum = -1, 0, np.finfo(np.float32).max
        for hyp in range(n_hyp):
            if (view1[hyp], view2[hyp]) != pair:
                continue
            n_in, s = stats[hyp]
            if n_in >= n_min_inliers and (n_in > best_n or (n_in == best_n and s < best_sum)):
                best, best_n, best_sum = hyp, n_in, s
        if best > 0:  # the reference's quirk
            best_all.append(best)
            in1 += [c1[n] for n in uniq[best]]
            in2 += [c2[n] for n in uniq[best]]
    res = (np.asarray(in1, np.int32), np.asarray(in2, np.int32), np.asarray(best_all, np.int32))
    return res + (stats,) if details else res


def partition(ids, members=None):
    """A labelling as a set of frozensets of members (label numbers do not matter)."""
    members = np.arange(len(ids)) if members is None else members
    groups = {}
    for m, i in zip(np.asarray(members).tolist(), np.asarray(ids).tolist()):
        groups.setdefault(i, set()).add(m)
    return {frozenset(v) for v in groups.values()}


def load_scene(g, name):
    """Arrays of scene ``name`` of the golden file ``g`` plus the mesh tables, in float64."""
    sc = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(name + "/")}
    sc["seeds"] = dict(zip(SEED_COLUMNS, sc["seeds"]))
    sc["points"], sc["symmetries"], sc["n_sym"] = g["points"], g["symmetries"], g["n_sym"]
    return sc


def restate(sc, dtype=np.float64):
    """The matching of one golden scene restated in ``dtype`` from the golden's seeds: (TC1C2, dists)."""
    poses, pts, sym = sc["poses"].astype(dtype), sc["points"].astype(dtype), sc["symmetries"].astype(dtype)
    if "cameras_TWC" in sc:
        TWC = sc["cameras_TWC"].astype(dtype)
        TC1C2 = invert(TWC[sc["seeds"]["view1"]]) @ TWC[sc["seeds"]["view2"]]
    else:
        TC1C2, _ = estimate_camera_poses(poses, sc["label_id"], sc["seeds"], pts, sym, sc["n_sym"])
    return TC1C2, score_matches(poses, sc["label_id"], sc["tmatches"], TC1C2, pts, sym)


# ---- bundle adjustment (CP/multiview/bundle_adjustment.py:208-350) restated with torch on the CPU; the Jacobian is AUTOGRAD's ----
# (the independent check of the analytic one in hp_mv_ba_linearize)
import torch  # noqa: E402


def pose9d_to_T(p):
    """CP/lib3d/transform_ops.py:57-67, TB/lib3d/rotations.py:22-36."""
    x = p[..., 0:3] / torch.norm(p[..., 0:3], dim=-1, keepdim=True)
    z = torch.cross(x, p[..., 3:6], dim=-1)
    z = z / torch.norm(z, dim=-1, keepdim=True)
    y = torch.cross(z, x, dim=-1)
    top = torch.cat((torch.stack((x, y, z), -1), p[..., 6:, None]), -1)
    bottom = torch.zeros_like(top[..., :1, :])
    bottom[..., 0, 3] = 1
    return torch.cat((top, bottom), -2)


def T_to_pose9d(T):
    return torch.cat((T[..., :3, :2].transpose(-1, -2).flatten(-2, -1), T[..., :3, -1]), dim=-1)


def project_t(K, T, pts):
    suv = (pts @ T[..., :3, :3].transpose(-1, -2) + T[..., None, :3, 3]) @ K.transpose(-1, -2)
    return suv[..., :2] / suv[..., 2:]


class BAProblem:
    """The BA of one golden scene: matched candidates of G11, the object / view order the reference's run used."""

    def __init__(self, sc, dtype=torch.float64):
        self.dtype = dtype
        npd = np.float64 if dtype == torch.float64 else np.float32
        cid = sc["matched_cand_id"]
        obj_pos = {o: n for n, o in enumerate(sc["ba_obj_id"].tolist())}
        view_pos = {v: n for n, v in enumerate(sc["ba_view_id"].tolist())}
        self.cand_obj = np.array([obj_pos[o] for o in sc["matched_obj_id"].tolist()])
        self.cand_view = np.array([view_pos[v] for v in sc["view_id"][cid].tolist()])
        self.cand_mesh = sc["label_id"][cid]
        self.obj_mesh = sc["ba_obj_label_id"]
        self.cand_TCO = sc["poses"][cid].astype(npd)
        self.K = sc["cameras_K"][sc["ba_view_id"]].astype(npd)
        self.points, self.symmetries, self.n_sym = sc["points"].astype(npd), sc["symmetries"].astype(npd), sc["n_sym"]
        self.n_obj, self.n_views = len(obj_pos), len(view_pos)
        self.TWO_9d0 = T_to_pose9d(torch.as_tensor(sc["ba_init_TWO"].astype(npd)))
        self.TCW_9d0 = T_to_pose9d(torch.as_tensor(invert(sc["ba_init_TWC"].astype(npd))))

    def align(self, TWO_9d, TCW_9d):
        TWO, TCW = pose9d_to_T(TWO_9d).numpy(), pose9d_to_T(TCW_9d).numpy()
        TCO = TCW[self.cand_view] @ TWO[self.cand_obj]
        dists, ids = reprojected_distance(self.cand_TCO, TCO, self.K[self.cand_view], self.cand_mesh, self.points, self.symmetries,
                                          self.n_sym)
        return dists, self.cand_TCO @ self.symmetries[self.cand_mesh, ids]

    def forward_jacobian(self, TWO_9d, TCW_9d, threshold=25.0):
        """-> errors [n_cand, n_pts, 2], loss, J [n_res, P] (autograd)."""
        _, aligned = self.align(TWO_9d.detach(), TCW_9d.detach())
        pts = torch.as_tensor(self.points[self.obj_mesh][self.cand_obj])
        K = torch.as_tensor(self.K[self.cand_view])
        y = project_t(K, torch.as_tensor(aligned), pts)
        n_two = TWO_9d.numel()

        def yhat_fn(theta):
            TWO, TCW = pose9d_to_T(theta[:n_two].view(-1, 9)), pose9d_to_T(theta[n_two:].view(-1, 9))
            return project_t(K, TCW[self.cand_view] @ TWO[self.cand_obj], pts).reshape(-1)

        theta = torch.cat((TWO_9d.reshape(-1), TCW_9d.reshape(-1))).detach()
        J = torch.autograd.functional.jacobian(yhat_fn, theta)
        errors = y - yhat_fn(theta).view(y.shape)
        loss = torch.clamp(errors ** 2, max=threshold).mean()
        return errors, loss, J

    def optimize_lm(self, optimize_cameras=True, n_iterations=100, threshold=25.0, lambd0=1e-3, L_down=9, L_up=11, eps=1e-5):
        TWO_9d, TCW_9d = self.TWO_9d0, self.TCW_9d0
        n_two = TWO_9d.numel()
        prev, lambd, done, hist = False, lambd0, False, {"loss": [], "lambda": [], "TWO_9d": [], "TCW_9d": []}
        for n in range(n_iterations):
            if not prev:
                errors, loss, J = self.forward_jacobian(TWO_9d, TCW_9d, threshold)
            for k, v in (("loss", float(loss)), ("lambda", lambd), ("TWO_9d", TWO_9d), ("TCW_9d", TCW_9d)):
                hist[k].append(v)
            if done:
                break
            A = (J.T @ J).double().numpy() + lambd * np.eye(J.shape[1])
            h = torch.as_tensor(np.linalg.pinv(A) @ (J.T @ errors.reshape(-1)).double().numpy()).to(self.dtype)
            TWO_u = TWO_9d + h[:n_two].view(-1, 9)
            TCW_u = TCW_9d + h[n_two:].view(-1, 9) if optimize_cameras else TCW_9d
            errors, next_loss, J = self.forward_jacobian(TWO_u, TCW_u, threshold)
            rho = float(loss - next_loss)
            if abs(rho) < eps:
                done = True
            elif rho > eps:
                TWO_9d, TCW_9d, loss, lambd, prev = TWO_u, TCW_u, next_loss, max(lambd / L_down, 1e-7), True
            else:
                lambd, prev = min(lambd * L_up, 1e7), False
        return TWO_9d, TCW_9d, hist

    def relative_poses(self, TWO_9d, TCW_9d):
        """Gauge-invariant TCO [n_obj, n_views, 4, 4] = T(TCW[v]) T(TWO[o]) (= inv(TWC[v]) TWO[o])."""
        TWO, TCW = pose9d_to_T(TWO_9d).numpy(), pose9d_to_T(TCW_9d).numpy()
        return TCW[None] @ TWO[:, None]


def golden_relative_poses(sc):
    """ba_output of G11 as [n_obj, n_views, 4, 4] in the BA's object / view order (reproject_scene: object-major)."""
    return sc["ba_output_poses"].astype(np.float64).reshape(len(sc["ba_obj_id"]), len(sc["ba_view_id"]), 4, 4)


def pose_deviation(A, B, obj_mesh, points, symmetries):
    """Largest symmetric distance (m, on the object's points) and rotation geodesic (rad, modulo the symmetries) between two
    [n_obj, n_views, 4, 4] pose sets."""
    n_obj, n_views = A.shape[:2]
    a, b = A.reshape(-1, 4, 4), B.reshape(-1, 4, 4)
    mesh = np.repeat(obj_mesh, n_views)
    d, ids = symmetric_distance(a, b, mesh, points.astype(np.float64), symmetries.astype(np.float64))
    aS = a @ symmetries.astype(np.float64)[mesh, ids]
    cos = (np.trace(np.swapaxes(aS[:, :3, :3], 1, 2) @ b[:, :3, :3], axis1=1, axis2=2) - 1) / 2
    return d.max(), np.arccos(np.clip(cos, -1, 1)).max()


# Measured by tests/test_multiview_reference.py::test_ba_reference_float32_error_is_the_recorded_one: the reference's float32 LM
# run (G11 ba_output) against this restatement in float64, largest over scenes A - D, and the float32 autograd
# J^T J / J^T e at the initialisation against float64, relative to the largest entry.
REF_F32_ERR_BA_SYMDIST = 2.5163e-05  # metres (scene C; A 5.9e-06, B 4.8e-06, D 1.9e-05)
REF_F32_ERR_BA_GEODESIC = 5.2736e-04  # rad (scene A)
REF_F32_ERR_JTJ_REL = 2.894e-07  # scene A
REF_F32_ERR_BA_ERRORS_PX = 1.293e-04  # residuals y - yhat, pixels (scene D)
REF_F32_ERR_JTE_REL = 1.428e-04  # scene D
