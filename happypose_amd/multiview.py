"""Multi-view candidate matching: the per-view pose candidates of several cameras -> objects of one scene and the relative
camera poses (CosyPose, "consistent multi-view multi-object pose estimation", stage 2).

Same names, arguments and outputs as the reference's ``CP/multiview/ransac.py`` (``multiview_candidate_matching``,
``scene_level_matching``, ``make_obj_infos``, ``get_best_viewpair_pose_est``) and ``make_view_groups`` of
``CP/multiview/bundle_adjustment.py:30-43``.  The camera-pose hypotheses and the scoring of the tentative matches are one
kernel launch each (``csrc/multiview.hip``); seeds and the inlier search are host C++ of the library.

Deviation: strongly connected components come from a routine of this module (no scipy) and are numbered by their smallest
member; the reference inherits scipy's label order.  Object ids and view groups therefore agree with the reference's as
PARTITIONS, not necessarily number by number.
"""

from __future__ import annotations

import time

import numpy as np
import pandas as pd
import torch

from . import ops
from .tensor_collection import PandasTensorCollection


def strongly_connected_components(n: int, src, dst) -> np.ndarray:
    """Label ``[n]`` of the strongly connected component of every node of the directed graph with edges ``src[i] -> dst[i]``
    (Tarjan, iterative).  Components are numbered 0, 1, ... in the order of their smallest member."""
    adj = [[] for _ in range(n)]
    for a, b in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        adj[a].append(b)
    index, low, comp = [-1] * n, [0] * n, [-1] * n
    on_stack, stack, counter, n_comp = [False] * n, [], 0, 0
    for root in range(n):
        if index[root] != -1:
            continue
        work = [(root, 0)]
        while work:
            v, i = work.pop()
            if i == 0:
                index[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on_stack[v] = True
            descended = False
            while i < len(adj[v]):
                w = adj[v][i]
                i += 1
                if index[w] == -1:
                    work.append((v, i))
                    work.append((w, 0))
                    descended = True
                    break
                if on_stack[w]:
                    low[v] = min(low[v], index[w])
            if descended:
                continue
            if low[v] == index[v]:
                while True:
                    w = stack.pop()
                    on_stack[w] = False
                    comp[w] = n_comp
                    if w == v:
                        break
                n_comp += 1
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
    comp = np.asarray(comp, dtype=np.int64).reshape(n)
    # renumber by smallest member
    _, first = np.unique(comp, return_index=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[comp[np.sort(first)]] = np.arange(len(first))
    return rank[comp] if n else comp


def scene_level_matching(candidates, inliers):
    """``CP/multiview/ransac.py:102-129``: candidates linked by mutual inlier matches are one object; an object needs
    two candidates."""
    n_cand = len(candidates)
    ids = strongly_connected_components(n_cand, inliers["inlier_matches_cand1"], inliers["inlier_matches_cand2"])
    obj_n_cand = np.bincount(ids, minlength=1)[ids] if n_cand else np.zeros(0, dtype=int)
    cand_infos = candidates.infos.copy()
    cand_infos["component_id"] = ids
    cand_infos = cand_infos[obj_n_cand >= 2].reset_index(drop=True)
    for n, (_comp_id, group) in enumerate(cand_infos.groupby("component_id")):
        cand_infos.loc[group.index, "component_id"] = n
    cand_infos = cand_infos.rename(columns={"component_id": "obj_id"})
    return PandasTensorCollection(infos=cand_infos, poses=candidates.poses[cand_infos["cand_id"].values])


def make_obj_infos(matched_candidates):
    """``CP/multiview/ransac.py:132-138``."""
    scene_infos = matched_candidates.infos.loc[:, ["obj_id", "score", "label"]].copy()
    gb = scene_infos.groupby("obj_id")
    scene_infos["n_cand"] = gb["score"].transform(len).astype(int)
    scene_infos["score"] = gb["score"].transform("sum")
    scene_infos = gb.first().reset_index(drop=False)
    return scene_infos


def get_best_viewpair_pose_est(TC1C2, seeds, inliers):
    """``CP/multiview/ransac.py:141-147``."""
    best_hypotheses = inliers["best_hypotheses"]
    infos = pd.DataFrame({"view1": seeds["view1"][best_hypotheses], "view2": seeds["view2"][best_hypotheses]})
    return PandasTensorCollection(infos=infos, TC1C2=TC1C2[torch.as_tensor(best_hypotheses, dtype=torch.long, device=TC1C2.device)])


def make_view_groups(pairs_TC1C2):
    """``CP/multiview/bundle_adjustment.py:30-43``: views linked (in both directions) by an accepted view pair form a group."""
    views = np.unique(pairs_TC1C2.infos.loc[:, ["view1", "view2"]].values.reshape(-1))
    local = {v: n for n, v in enumerate(views.tolist())}
    view1 = [local[v] for v in pairs_TC1C2.infos["view1"].tolist()]
    view2 = [local[v] for v in pairs_TC1C2.infos["view2"].tolist()]
    ids = strongly_connected_components(len(views), view1, view2)
    return pd.DataFrame({"view_id": views, "view_group": ids})


def multiview_candidate_matching(candidates, mesh_db, model_bsz=1e3, score_bsz=1e5, dist_threshold=0.02, cameras=None,
                                 n_ransac_iter=20, n_min_inliers=3):
    """``CP/multiview/ransac.py:150-222``.  ``candidates``: ``infos`` with ``view_id``, ``label``, ``score`` and ``poses
    [n, 4, 4]`` (TCO); ``mesh_db``: ``MeshDataBase.batched(aabb=True, n_sym=...).to(device)``; ``cameras`` (``infos.view_id``,
    ``TWC``): use these camera poses instead of estimating them.  ``model_bsz`` / ``score_bsz`` are accepted for the
    reference's signature; nothing is chunked here.  A scene without a single tentative match cannot be matched (the reference
    fails in ``torch.cat`` of an empty list): ``ValueError``."""
    t_models = t_score = t_misc = 0.0
    known_poses = cameras is not None
    if known_poses:
        n_ransac_iter = 1

    t0 = time.perf_counter()
    candidates.infos["cand_id"] = np.arange(len(candidates))
    labels = candidates.infos["label"].values
    label_ids = mesh_db.ids_of(labels) if len(labels) else np.zeros(0, np.int32)
    t_misc += time.perf_counter() - t0

    t0 = time.perf_counter()
    seeds, tmatches = ops.ransac_make_infos(candidates.infos["view_id"].values, label_ids, n_ransac_iter, 0)
    if len(seeds["view1"]) == 0:
        raise ValueError("multiview_candidate_matching: no two views share a label, there is nothing to match "
                         f"({len(candidates)} candidates)")
    dev = mesh_db.device_tables["points"].device if mesh_db.device_tables else candidates.poses.device
    poses = candidates.poses.to(dev)
    if not known_poses:
        TC1C2 = ops.mv_estimate_camera_poses(poses, label_ids, seeds, mesh_db)
    else:
        idx = pd.Series(np.arange(len(cameras)), index=cameras.infos["view_id"].values)
        TWC = cameras.TWC.to(dev).to(torch.float32)
        TWC1, TWC2 = TWC[idx.loc[seeds["view1"]].values], TWC[idx.loc[seeds["view2"]].values]
        TC1W = TWC1.clone()
        TC1W[:, :3, :3] = TWC1[:, :3, :3].transpose(1, 2)
        TC1W[:, :3, 3:] = -TC1W[:, :3, :3] @ TWC1[:, :3, 3:]
        TC1C2 = TC1W @ TWC2
    t_models += time.perf_counter() - t0

    t0 = time.perf_counter()
    dists = ops.mv_score_seed_matches(seeds, tmatches, TC1C2, poses, label_ids, mesh_db)  # 4 B per row on the device
    inliers = ops.ransac_find_inliers(seeds["view1"], seeds["view2"], tmatches["hypothesis_id"], tmatches["cand1"],
                                      tmatches["cand2"], dists.cpu().numpy(), dist_threshold, n_min_inliers)
    t_score += time.perf_counter() - t0

    t0 = time.perf_counter()
    pairs_TC1C2 = get_best_viewpair_pose_est(TC1C2, seeds, inliers)
    filtered_candidates = scene_level_matching(candidates, inliers)
    scene_infos = make_obj_infos(filtered_candidates)
    t_misc += time.perf_counter() - t0
    return {"filtered_candidates": filtered_candidates, "scene_infos": scene_infos, "pairs_TC1C2": pairs_TC1C2,
            "time_models": t_models, "time_score": t_score, "time_misc": t_misc}


# ---- bundle adjustment (CP/multiview/bundle_adjustment.py) and the scene predictor (CP/integrated/multiview_predictor.py) -------
from collections import defaultdict  # noqa: E402

from .tensor_collection import concatenate  # noqa: E402


class SamplerError(Exception):
    pass


def invert_transform_matrices(T: torch.Tensor) -> torch.Tensor:
    """``TB/lib3d/transform_ops.py:59-67``."""
    R_inv = T[..., :3, :3].transpose(-2, -1)
    out = T.clone()
    out[..., :3, :3] = R_inv
    out[..., :3, 3:] = -R_inv @ T[..., :3, 3:]
    return out


def compute_transform_from_pose9d(pose9d: torch.Tensor) -> torch.Tensor:
    """``CP/lib3d/transform_ops.py:57-67`` (Gram-Schmidt of ``TB/lib3d/rotations.py:22-36``)."""
    x_raw, y_raw = pose9d[..., 0:3], pose9d[..., 3:6]
    x = x_raw / torch.norm(x_raw, p=2, dim=-1, keepdim=True)
    z = torch.cross(x, y_raw, dim=-1)
    z = z / torch.norm(z, p=2, dim=-1, keepdim=True)
    y = torch.cross(z, x, dim=-1)
    T = torch.zeros(*pose9d.shape[:-1], 4, 4, dtype=pose9d.dtype, device=pose9d.device)
    T[..., :3, :3] = torch.stack((x, y, z), -1)
    T[..., :3, 3] = pose9d[..., 6:]
    T[..., 3, 3] = 1
    return T


class MultiviewRefinement:
    """``CP/multiview/bundle_adjustment.py:50-428``: object poses ``TWO`` and camera poses ``TCW`` that minimise the reprojection
    error of the objects' points against the matched candidates, by Levenberg-Marquardt.  Residuals, loss terms and the
    per-candidate blocks of ``J^T J`` / ``J^T e`` come from ``hp_mv_ba_linearize`` (analytic Jacobian); the blocks are added into
    the ``P x P`` system in candidate order and the damped system is solved on the host in float64 (the reference: ``pinverse``
    on the CPU).  Two runs are bit-identical."""

    def __init__(self, candidates, cameras, pairs_TC1C2, mesh_db):
        self.device, self.dtype = candidates.device, candidates.poses.dtype
        self.mesh_db = mesh_db
        cameras = cameras.to(self.device).to(self.dtype)
        pairs_TC1C2 = pairs_TC1C2.to(self.device).to(self.dtype)
        view_ids = np.unique(candidates.infos["view_id"])
        keep = np.logical_and(np.isin(pairs_TC1C2.infos["view1"], view_ids), np.isin(pairs_TC1C2.infos["view2"], view_ids))
        pairs_TC1C2 = pairs_TC1C2[np.where(keep)[0]]
        cameras = cameras[np.where(np.isin(cameras.infos["view_id"], view_ids))[0]]
        self.cam_infos = cameras.infos
        self.view_to_id = {view_id: n for n, view_id in enumerate(self.cam_infos["view_id"])}
        self.K = cameras.K
        self.n_views = len(self.cam_infos)
        self.obj_infos = make_obj_infos(candidates)
        self.obj_to_id = {obj_id: n for n, obj_id in enumerate(self.obj_infos["obj_id"])}
        self.obj_mesh_ids = mesh_db.ids_of(self.obj_infos["label"].values)
        self.obj_points = mesh_db.device_tables["points"][torch.as_tensor(self.obj_mesh_ids, dtype=torch.long, device=self.device)]
        self.n_points = self.obj_points.shape[1]
        self.n_objects = len(self.obj_infos)
        self.cand = candidates
        self.cand_TCO = candidates.poses
        self.cand_labels = candidates.infos["label"]
        self.cand_mesh_ids = mesh_db.ids_of(self.cand_labels.values)
        self.cand_view_ids = [self.view_to_id[v] for v in candidates.infos["view_id"]]
        self.cand_obj_ids = [self.obj_to_id[o] for o in candidates.infos["obj_id"]]
        self.n_candidates = len(self.cand_TCO)
        self.visibility_matrix = np.zeros((self.n_objects, self.n_views), dtype=int)
        self.visibility_matrix[self.cand_obj_ids, self.cand_view_ids] = 1
        self.v2v1_TC2C1_map = {
            (self.view_to_id[v2], self.view_to_id[v1]): invert_transform_matrices(TC1C2)
            for (v1, v2, TC1C2) in zip(pairs_TC1C2.infos["view1"], pairs_TC1C2.infos["view2"], pairs_TC1C2.TC1C2)}
        self.ov_TCO_cand_map = {(o, v): TCO for (o, v, TCO) in zip(self.cand_obj_ids, self.cand_view_ids, self.cand_TCO)}

    def sample_initial_TWO_TWC(self, seed):
        """``:140-198``: a spanning order of the views through the accepted view pairs, drawn with ``np.random.RandomState(seed)``."""
        nan = float("nan")
        TWO = torch.full((self.n_objects, 4, 4), nan, dtype=self.dtype, device=self.device)
        TWC = torch.full((self.n_views, 4, 4), nan, dtype=self.dtype, device=self.device)
        object_to_views = defaultdict(set)
        for v in range(self.n_views):
            for o in range(self.n_objects):
                if self.visibility_matrix[o, v]:
                    object_to_views[o].add(v)
        np_random = np.random.RandomState(seed)
        views_ordered = np_random.permutation(np.arange(self.n_views))
        objects_ordered = np_random.permutation(np.arange(self.n_objects))
        w = views_ordered[0]
        TWC[w] = torch.eye(4, 4, device=self.device, dtype=self.dtype)
        views_initialized = {w}
        views_to_initialize = set(np.arange(self.n_views)) - views_initialized
        n_pass, n = 20, 0
        while len(views_to_initialize) > 0:
            for v1 in views_ordered:
                if v1 in views_to_initialize:
                    for v2 in views_ordered:
                        if v2 not in views_initialized:
                            continue
                        if (v2, v1) in self.v2v1_TC2C1_map:
                            TWC[v1] = TWC[v2] @ self.v2v1_TC2C1_map[(v2, v1)]
                            views_to_initialize.remove(v1)
                            views_initialized.add(v1)
                            break
            n += 1
            if n >= n_pass:
                raise SamplerError("Cannot find an initialization")
        for o in objects_ordered:
            for v in views_ordered:
                if v in object_to_views[o]:
                    TWO[o] = TWC[v] @ self.ov_TCO_cand_map[(o, v)]
                    break
        return TWO, TWC

    @staticmethod
    def extract_pose9d(T):
        return torch.cat((T[..., :3, :2].transpose(-1, -2).flatten(-2, -1), T[..., :3, -1]), dim=-1)

    def align_TCO_cand(self, TWO_9d, TCW_9d):
        """``:208-221``: every candidate's pose times the symmetry that brings its reprojection closest to the current estimate
        (``hp_mv_score_matches``, reprojected mode: view = hypothesis, object = second pose table)."""
        TWO = compute_transform_from_pose9d(TWO_9d).to(self.dtype)
        TCW = compute_transform_from_pose9d(TCW_9d).to(self.dtype)
        dists, sym_ids = ops.mv_score_matches(self.cand_view_ids, np.arange(self.n_candidates), self.cand_obj_ids, TCW, self.cand_TCO,
                                              self.cand_mesh_ids, TWO, self.mesh_db, K=self.K, return_sym_ids=True)
        mesh_ids = torch.as_tensor(self.cand_mesh_ids, dtype=torch.long, device=self.device)
        sym = self.mesh_db.device_tables["symmetries"][mesh_ids, sym_ids.long().clamp_(min=0)]
        return dists, self.cand_TCO @ sym

    def forward_jacobian(self, TWO_9d, TCW_9d, residuals_threshold):
        """``:223-270`` -> ``(errors [n_cand, n_pts, 2], loss, JtJ [P, P] float64, Jte [P] float64)``, ``P = 9 (n_objects +
        n_views)``, objects first.  The candidate blocks are added in candidate order on the host."""
        _, TCO_cand_aligned = self.align_TCO_cand(TWO_9d, TCW_9d)
        errors, clipped, JtJ_c, Jte_c = ops.mv_ba_linearize(TWO_9d, TCW_9d, self.cand_obj_ids, self.cand_view_ids, TCO_cand_aligned,
                                                            self.K, self.obj_points, residuals_threshold)
        loss = clipped.mean()
        JtJ_c, Jte_c = JtJ_c.cpu().numpy(), Jte_c.cpu().numpy()
        P = 9 * (self.n_objects + self.n_views)
        JtJ, Jte = np.zeros((P, P)), np.zeros(P)
        for c, (o, v) in enumerate(zip(self.cand_obj_ids, self.cand_view_ids)):
            idx = np.r_[9 * o:9 * o + 9, 9 * (self.n_objects + v):9 * (self.n_objects + v) + 9]
            JtJ[np.ix_(idx, idx)] += JtJ_c[c]
            Jte[idx] += Jte_c[c]
        return errors, loss, JtJ, Jte

    @staticmethod
    def compute_lm_step(JtJ, Jte, lambd):
        """``:272-279``: ``pinv(J^T J + lambda I) J^T e``, float64 on the host."""
        return np.linalg.pinv(JtJ + lambd * np.eye(len(JtJ))) @ Jte

    def optimize_lm(self, TWO_9d, TCW_9d, optimize_cameras=True, n_iterations=50, residuals_threshold=25, lambd0=1e-3, L_down=9,
                    L_up=11, eps=1e-5):
        """``:281-350``, the same schedule; the step uses the unclipped errors, only the loss is clipped.  The parameters are
        carried in float64 between iterations (the history holds them so); poses leave in the candidates' dtype."""
        TWO_9d, TCW_9d = TWO_9d.double(), TCW_9d.double()
        n_params_TWO = TWO_9d.numel()
        prev_iter_is_update = False
        lambd = lambd0
        done = False
        history = defaultdict(list)
        for n in range(n_iterations):
            if not prev_iter_is_update:
                errors, loss, JtJ, Jte = self.forward_jacobian(TWO_9d, TCW_9d, residuals_threshold)
            history["TWO_9d"].append(TWO_9d)
            history["TCW_9d"].append(TCW_9d)
            history["loss"].append(loss)
            history["lambda"].append(lambd)
            history["iteration"].append(n)
            if done:
                break
            h = torch.as_tensor(self.compute_lm_step(JtJ, Jte, lambd), dtype=TWO_9d.dtype, device=self.device)
            TWO_9d_updated = TWO_9d + h[:n_params_TWO].view(self.n_objects, 9)
            TCW_9d_updated = TCW_9d + h[n_params_TWO:].view(self.n_views, 9) if optimize_cameras else TCW_9d
            errors, next_loss, JtJ, Jte = self.forward_jacobian(TWO_9d_updated, TCW_9d_updated, residuals_threshold)
            rho = loss - next_loss
            if rho.abs() < eps:
                done = True
            elif rho > eps:
                TWO_9d, TCW_9d, loss = TWO_9d_updated, TCW_9d_updated, next_loss
                lambd = max(lambd / L_down, 1e-7)
                prev_iter_is_update = True
            else:
                lambd = min(lambd * L_up, 1e7)
                prev_iter_is_update = False
        return TWO_9d, TCW_9d, history

    def robust_initialization_TWO_TCW(self, n_init=1):
        TWO_9d_init, TCW_9d_init, dists = [], [], []
        for n in range(n_init):
            TWO, TWC = self.sample_initial_TWO_TWC(n)
            TWO_9d, TCW_9d = self.extract_pose9d(TWO), self.extract_pose9d(invert_transform_matrices(TWC))
            dists_, _ = self.align_TCO_cand(TWO_9d, TCW_9d)
            TWO_9d_init.append(TWO_9d)
            TCW_9d_init.append(TCW_9d)
            dists.append(dists_.mean())
        best_iter = int(torch.tensor(dists).argmin())
        return TWO_9d_init[best_iter], TCW_9d_init[best_iter]

    def make_scene_infos(self, TWO_9d, TCW_9d):
        TWO = compute_transform_from_pose9d(TWO_9d).to(self.dtype)
        TWC = invert_transform_matrices(compute_transform_from_pose9d(TCW_9d)).to(self.dtype)
        return (PandasTensorCollection(infos=self.obj_infos.copy(), TWO=TWO),
                PandasTensorCollection(infos=self.cam_infos.copy(), TWC=TWC, K=self.K))

    def convert_history(self, history):
        history["objects"], history["cameras"] = [], []
        for TWO_9d, TCW_9d in zip(history["TWO_9d"], history["TCW_9d"]):
            objects, cameras = self.make_scene_infos(TWO_9d, TCW_9d)
            history["objects"].append(objects)
            history["cameras"].append(cameras)
        return history

    def solve(self, sample_n_init=1, **lm_kwargs):
        t0 = time.perf_counter()
        TWO_9d_init, TCW_9d_init = self.robust_initialization_TWO_TCW(n_init=sample_n_init)
        t1 = time.perf_counter()
        TWO_9d_opt, TCW_9d_opt, history = self.optimize_lm(TWO_9d_init, TCW_9d_init, **lm_kwargs)
        t2 = time.perf_counter()
        objects, cameras = self.make_scene_infos(TWO_9d_opt, TCW_9d_opt)
        objects_init, cameras_init = self.make_scene_infos(TWO_9d_init, TCW_9d_init)
        history = self.convert_history(history)
        return {"objects_init": objects_init, "cameras_init": cameras_init, "objects": objects, "cameras": cameras,
                "history": history, "time_init": t1 - t0, "time_opt": t2 - t1, "time_misc": time.perf_counter() - t2}


class MultiviewScenePredictor:
    """``CP/integrated/multiview_predictor.py:21-152``."""

    def __init__(self, mesh_db, n_sym=64, ba_aabb=True, ba_n_points=None, device="cuda"):
        self.device = torch.device(device)
        self.mesh_db_ransac = mesh_db.batched(n_sym=n_sym, aabb=True).to(self.device).float()
        self.mesh_db_ba = mesh_db.batched(aabb=ba_aabb, resample_n_points=ba_n_points, n_sym=n_sym).to(self.device).float()

    def reproject_scene(self, objects, cameras):
        TCO_data = []
        for o in range(len(objects)):
            for v in range(len(cameras)):
                obj, cam = objects[[o]], cameras[[v]]
                infos = {"scene_id": cam.infos["scene_id"].values, "view_id": cam.infos["view_id"].values,
                         "score": obj.infos["score"].values + 1.0, "view_group": obj.infos["view_group"].values,
                         "label": obj.infos["label"].values, "batch_im_id": cam.infos["batch_im_id"].values,
                         "obj_id": obj.infos["obj_id"].values, "from_ba": [True]}
                TCO_data.append(PandasTensorCollection(infos=pd.DataFrame(infos), poses=invert_transform_matrices(cam.TWC) @ obj.TWO))
        return concatenate(TCO_data)

    def predict_scene_state(self, candidates, cameras, score_th=0.3, use_known_camera_poses=False, ransac_n_iter=2000,
                            ransac_dist_threshold=0.02, ba_n_iter=100):
        """Candidates (``infos``: scene_id, group_id, view_id, label, score, batch_im_id; ``poses``) and cameras (``infos``:
        scene_id, view_id, batch_im_id; ``K``, and ``TWC`` for known poses) -> the reference's prediction keys.  A scene in which
        nothing can be matched (no candidate above ``score_th``, a single view, no view pair with enough inliers) has no scene
        state; the reference fails there in a concatenate of nothing: ``ValueError`` with the reason."""
        predictions = {}
        cand_inputs = candidates
        assert len(np.unique(candidates.infos["scene_id"])) == 1
        scene_id = np.unique(candidates.infos["scene_id"]).item()
        group_id = np.unique(candidates.infos["group_id"]).item()
        candidates = candidates[np.where(candidates.infos["score"] >= score_th)[0]]
        predictions["cand_inputs"] = candidates
        if len(candidates) == 0:
            raise ValueError(f"predict_scene_state: no candidate has score >= {score_th}")
        matching_outputs = multiview_candidate_matching(candidates=candidates, mesh_db=self.mesh_db_ransac, n_ransac_iter=ransac_n_iter,
                                                        dist_threshold=ransac_dist_threshold,
                                                        cameras=cameras if use_known_camera_poses else None)
        pairs_TC1C2 = matching_outputs["pairs_TC1C2"]
        candidates = matching_outputs["filtered_candidates"]
        predictions["cand_matched"] = candidates
        if len(candidates) == 0 or len(pairs_TC1C2) == 0:
            raise ValueError("predict_scene_state: no view pair has enough inlier matches, there is no scene to reconstruct")
        group_infos = make_view_groups(pairs_TC1C2)
        candidates = candidates.merge_df(group_infos, on="view_id").to(self.device)
        pred_objects, pred_cameras, pred_reproj, pred_reproj_init = [], [], [], []
        for view_group, candidate_ids in candidates.infos.groupby("view_group").groups.items():
            problem = MultiviewRefinement(candidates=candidates[list(candidate_ids)], cameras=cameras, pairs_TC1C2=pairs_TC1C2,
                                          mesh_db=self.mesh_db_ba)
            ba_outputs = problem.solve(n_iterations=ba_n_iter, optimize_cameras=not use_known_camera_poses)
            for key, dst_obj, dst_cam, dst_reproj in (("", pred_objects, pred_cameras, pred_reproj),
                                                      ("_init", None, None, pred_reproj_init)):
                objs, cams = ba_outputs["objects" + key], ba_outputs["cameras" + key]
                for x in (objs, cams):
                    x.infos["view_group"] = view_group
                    x.infos["group_id"] = group_id
                    x.infos["scene_id"] = scene_id
                dst_reproj.append(self.reproject_scene(objs, cams))
                if dst_obj is not None:
                    dst_obj.append(objs)
                    dst_cam.append(cams)
        predictions["scene/objects"] = concatenate(pred_objects)
        predictions["scene/cameras"] = concatenate(pred_cameras)
        predictions["ba_output"] = concatenate(pred_reproj)
        predictions["ba_input"] = concatenate(pred_reproj_init)
        cand_inputs = PandasTensorCollection(infos=cand_inputs.infos, poses=cand_inputs.poses.to(self.device))
        predictions["ba_output+all_cand"] = concatenate([predictions["ba_output"], cand_inputs])
        return predictions
