#!/usr/bin/env python3
"""Generate ``tests/golden/g12_pose_errors.npz`` by running THE REFERENCE's pose-error functions in float32 on seeded inputs.

Runs only in the build container.  ``TB/lib3d/distances.py``, ``CP/lib3d/symmetric_distances.py`` and
``CP/evaluation/meters/utils.py`` are imported from where they lie through the namespace shim of ``tools/gen_golden.py``
(``symmetric_distances`` imports the reference's C++ extension: built into a temporary directory outside the repository, as in
``tools/gen_golden_multiview.py``).  The file holds arrays only.

Metrics (rows of ``ops.pose_errors``):
  ``cloud_small`` (~900 points) / ``cloud_large`` (~2 000): ``synthetic.make_mesh`` vertices with exact duplicates removed.
  ``<c>/TXO_gt``, ``<c>/TXO_pred`` [6, 4, 4]: ground truth 0.5 - 1.2 m from the camera, predictions off by 0.02 - 0.3 rad and about
  1 cm; the LAST row has pred == gt.  ``<c>/add_*`` and ``<c>/adds_*``: ``norm_avg`` / ``xyz_avg`` / ``norm_max`` of ``dists_add`` /
  ``dists_add_symmetric``; ``K`` and ``small/pixel_dists`` [6, P]: ``reprojected_dist`` of every single point (pixels);
  ``small/adds_dists`` [6, P, 3] and ``small/adds_assign`` [6, P]: the reference's per-point differences and the neighbour each one used (recovered here from the reference's float32 point sets and checked to reproduce ``dists`` bit for bit).
  ``sym/*``: the tables of ``synthetic.make_multiview_objects`` (mesh vertices, 64 rotations per continuous axis), rows
  ``sym/obj_id``, ``sym/TXO_gt``, ``sym/TXO_pred`` and ``dists_add_symmetries`` on them: ``sym/norm_avg``, ``sym/xyz_avg``,
  ``sym/norm_max``, ``sym/sym_id`` (the candidate whose differences the reference returned); ``sym/chamfer``: ``chamfer_dist`` of the same rows.
  ``short/*``: 24 rows of ADD and ADD-S on the first 63 points of ``cloud_small`` (``TXO_gt``, ``TXO_pred``, ``add_*``, ``adds_*``,
  ``adds_assign``): the means of few terms.
Host logic: a seeded table of predictions (``pred/scene_id``, ``view_id``, ``label_id``, ``score``) and ground truth
  (``gt/...``, ``visib_fract``) with several scenes, views and labels, repeated instances and score ties, ``targets/*``, and what
  each of ``add_inst_num``, ``get_top_n_ids``, ``add_valid_gt``, ``get_candidate_matches``, ``match_poses`` and
  ``compute_auc_posecnn`` returns for it (``host/*``).

Usage:  python tools/gen_golden_pose_errors.py
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

import gen_golden as gg  # noqa: E402
import gen_golden_multiview as ggm  # noqa: E402

CP = "happypose.pose_estimators.cosypose.cosypose"
N_ROWS = 6
N_SHORT = 63  # points of the short cloud: the smallest row of several points that the GPU tests launch


def dedup_cloud(seed: int, n_lat: int, n_lon: int) -> np.ndarray:
    from happypose_amd.synthetic import make_mesh

    v = make_mesh(seed, n_lat=n_lat, n_lon=n_lon, diameter=0.15, tex_size=16).vertices.astype(np.float32)
    _, first = np.unique(v, axis=0, return_index=True)
    return v[np.sort(first)]


def make_poses(rs: np.random.RandomState, n: int):
    """Ground truth 0.5 - 1.2 m in front of the camera; predictions rotated by 0.02 - 0.3 rad about a random axis and shifted by
    about 1 cm; the last prediction IS the ground truth."""
    from happypose_amd.synthetic import random_rotations

    def rodrigues(axis, angle):
        axis = axis / np.linalg.norm(axis)
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx

    gt, pred = np.tile(np.eye(4), (n, 1, 1)), np.tile(np.eye(4), (n, 1, 1))
    gt[:, :3, :3] = random_rotations(rs, n)
    gt[:, :3, 3] = np.stack([rs.uniform(-0.15, 0.15, n), rs.uniform(-0.1, 0.1, n), rs.uniform(0.5, 1.2, n)], -1)
    for i in range(n):
        pred[i, :3, :3] = rodrigues(rs.normal(size=3), rs.uniform(0.02, 0.3)) @ gt[i, :3, :3]
        pred[i, :3, 3] = gt[i, :3, 3] + rs.normal(scale=0.006, size=3)
    pred[-1] = gt[-1]
    return gt.astype(np.float32), pred.astype(np.float32)


def host_tables(rs: np.random.RandomState):
    """Predictions and ground truth over 2 scenes x 3 views x 4 labels with repeated instances, score ties and a view without
    ground truth; targets for a part of the groups."""
    pred, gt = [], []
    for scene in (3, 7):
        for view in (0, 1, 4):
            for label in range(4):
                for _ in range(rs.randint(0, 4)):
                    gt.append((scene, view, label, rs.choice([0.05, 0.3, 0.3, 0.8, 1.0])))
                for _ in range(rs.randint(0, 5)):
                    pred.append((scene, view, label, rs.choice([0.2, 0.5, 0.5, 0.9, rs.uniform()])))
    pred += [(7, 9, 1, 0.7), (7, 9, 2, 0.4)]  # a view the ground truth does not know
    pred, gt = np.array(pred), np.array(gt)
    pred, gt = pred[rs.permutation(len(pred))], gt[rs.permutation(len(gt))]
    groups = np.unique(gt[:, :3], axis=0)
    groups = groups[rs.rand(len(groups)) < 0.7]
    targets = np.concatenate([groups, rs.randint(1, 3, size=(len(groups), 1))], 1)
    return pred, gt, targets


def main():
    import pandas as pd
    import torch

    from happypose_amd.mesh_store import MeshDataBase
    from happypose_amd.synthetic import make_multiview_objects

    gg._shim()
    ggm.build_reference_extension()
    D = gg.imp("happypose.toolbox.lib3d.distances")
    tops = gg.imp("happypose.toolbox.lib3d.transform_ops")
    SD = gg.imp(f"{CP}.lib3d.symmetric_distances")
    U = gg.imp(f"{CP}.evaluation.meters.utils")
    rmd = gg.imp(f"{CP}.lib3d.rigid_mesh_database")
    out = {}
    t = torch.as_tensor

    # ---- ADD and ADD-S on the two clouds ----------------------------------------------------------------------------------------
    rs = np.random.RandomState(12)
    for name, (seed, n_lat, n_lon) in {"small": (1201, 24, 40), "large": (1202, 36, 56)}.items():
        cloud = dedup_cloud(seed, n_lat, n_lon)
        gt, pred = make_poses(rs, N_ROWS)
        pts = t(cloud)[None].repeat(N_ROWS, 1, 1)
        out[f"cloud_{name}"], out[f"{name}/TXO_gt"], out[f"{name}/TXO_pred"] = cloud, gt, pred
        for key, fn in (("add", D.dists_add), ("adds", D.dists_add_symmetric)):
            dists = fn(t(pred), t(gt), pts)
            out[f"{name}/{key}_norm_avg"] = torch.norm(dists, dim=-1, p=2).mean(-1).numpy()
            out[f"{name}/{key}_xyz_avg"] = dists.abs().mean(dim=-2).numpy()
            out[f"{name}/{key}_norm_max"] = torch.norm(dists, dim=-1, p=2).max(-1).values.numpy()
        if name == "small":
            gt_pts, pred_pts = tops.transform_pts(t(gt), pts), tops.transform_pts(t(pred), pts)
            assign = torch.stack([((gt_pts[b][:, None] - pred_pts[b][None]) ** 2).sum(-1).argmin(1) for b in range(N_ROWS)])
            again = gt_pts - torch.gather(pred_pts, 1, assign[..., None].expand(-1, -1, 3))
            assert torch.equal(again, dists), "the recovered neighbours do not reproduce the reference's dists"
            out["small/adds_dists"], out["small/adds_assign"] = dists.numpy(), assign.numpy().astype(np.int32)
            # per-point pixel distances in the reference's arithmetic: reprojected_dist on batches of ONE point each
            n = cloud.shape[0]
            rep = lambda a: t(a)[:, None].repeat(1, n, 1, 1).reshape(N_ROWS * n, *a.shape[1:])  # noqa: E731
            out["K"] = np.array([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]], np.float32)
            pix = SD.reprojected_dist(rep(gt), rep(pred), t(out["K"])[None].repeat(N_ROWS * n, 1, 1), pts.reshape(-1, 1, 3))
            out["small/pixel_dists"] = pix.reshape(N_ROWS, n).numpy()
        print(name, cloud.shape, "ADD", out[f"{name}/add_norm_avg"], "ADD-S", out[f"{name}/adds_norm_avg"])

    # ---- ADD-SYM and chamfer_dist on the multi-view objects ------------------------------------------------------------------------
    mine = MeshDataBase.from_object_ds(make_multiview_objects()).batched(n_sym=64)
    mesh_db = rmd.BatchedMeshes(mine.infos, mine.labels, t(mine.points), t(mine.symmetries)).float()
    obj_id = np.array([0, 0, 1, 1, 2, 3, 1, 0], np.int32)
    gt, pred = make_poses(rs, len(obj_id))
    # symmetric objects seen under another symmetry than the identity: the prediction of rows 1 and 3 is near T_gt S
    pred[1] = gt[1] @ mine.symmetries[0, 1] @ np.linalg.inv(gt[1]).astype(np.float32) @ pred[1]
    pred[3] = gt[3] @ mine.symmetries[1, 23] @ np.linalg.inv(gt[3]).astype(np.float32) @ pred[3]
    norm_avg, xyz_avg, norm_max, sym_id = [], [], [], []
    for r, o in enumerate(obj_id):
        n_pts, n_sym = mine.infos[mine.labels[o]]["n_points"], mine.n_sym[o]
        pts = t(mine.points[o, :n_pts])[None]
        possible = t(gt[r])[None, None] @ t(mine.symmetries[o, :n_sym])[None]
        dists = D.dists_add_symmetries(t(pred[r])[None], possible, pts)
        same = [s for s in range(n_sym) if torch.equal(D.dists_add(t(pred[r])[None], possible[:, s], pts), dists)]
        norm_avg.append(torch.norm(dists, dim=-1, p=2).mean(-1).numpy()[0])
        norm_max.append(torch.norm(dists, dim=-1, p=2).max(-1).values.numpy()[0])
        xyz_avg.append(dists.abs().mean(dim=-2).numpy()[0])
        sym_id.append(same[0])
    labels = mine.labels[obj_id]
    chamfer, _ = SD.chamfer_dist(t(gt), t(pred), labels, mesh_db)
    out.update({"sym/points": mine.points, "sym/symmetries": mine.symmetries, "sym/n_sym": mine.n_sym,
                "sym/n_points": np.array([mine.infos[label]["n_points"] for label in mine.labels], np.int32), "sym/obj_id": obj_id,
                "sym/TXO_gt": gt, "sym/TXO_pred": pred, "sym/norm_avg": np.array(norm_avg, np.float32), "sym/norm_max": np.array(norm_max, np.float32),
                "sym/xyz_avg": np.array(xyz_avg, np.float32), "sym/sym_id": np.array(sym_id, np.int32), "sym/chamfer": chamfer.numpy()})
    print("ADD-SYM", out["sym/norm_avg"], out["sym/sym_id"], "chamfer", out["sym/chamfer"])

    # ---- a short cloud: how far the means are off when only 63 terms average the rounding away -------------------------------------
    cloud = out["cloud_small"][:N_SHORT]
    gt, pred = make_poses(np.random.RandomState(16), 4 * N_ROWS)
    pts = t(cloud)[None].repeat(len(gt), 1, 1)
    out["short/TXO_gt"], out["short/TXO_pred"] = gt, pred
    for key, fn in (("add", D.dists_add), ("adds", D.dists_add_symmetric)):
        dists = fn(t(pred), t(gt), pts)
        out[f"short/{key}_norm_avg"] = torch.norm(dists, dim=-1, p=2).mean(-1).numpy()
        out[f"short/{key}_xyz_avg"] = dists.abs().mean(dim=-2).numpy()
        out[f"short/{key}_norm_max"] = torch.norm(dists, dim=-1, p=2).max(-1).values.numpy()
    gt_pts, pred_pts = tops.transform_pts(t(gt), pts), tops.transform_pts(t(pred), pts)
    assign = ((gt_pts[:, :, None] - pred_pts[:, None]) ** 2).sum(-1).argmin(2)
    assert torch.equal(gt_pts - torch.gather(pred_pts, 1, assign[..., None].expand(-1, -1, 3)), dists)
    out["short/adds_assign"] = assign.numpy().astype(np.int32)
    print("short", cloud.shape, len(gt), "rows")

    # ---- host logic ---------------------------------------------------------------------------------------------------------------
    pred, gt, targets = host_tables(np.random.RandomState(13))
    label = lambda ids: np.array([f"obj_{int(i):06d}" for i in ids])  # noqa: E731
    frame = lambda a, last: pd.DataFrame({"scene_id": a[:, 0].astype(int), "view_id": a[:, 1].astype(int), "label": label(a[:, 2]),  # noqa: E731
                                          last: a[:, 3]})
    keys = ["scene_id", "view_id", "label"]
    pred_df, gt_df, targets_df = frame(pred, "score"), frame(gt, "visib_fract"), frame(targets, "inst_count")
    targets_df["inst_count"] = targets_df["inst_count"].astype(int)
    for k, a in (("pred", pred), ("gt", gt), ("targets", targets)):
        out[f"{k}/scene_id"], out[f"{k}/view_id"], out[f"{k}/label_id"] = (a[:, i].astype(np.int64) for i in range(3))
    out["pred/score"], out["gt/visib_fract"], out["targets/inst_count"] = pred[:, 3], gt[:, 3], targets[:, 3].astype(np.int64)

    out["host/pred_inst_id"] = U.add_inst_num(pred_df.copy(), key="pred_inst_id", group_keys=keys)["pred_inst_id"].to_numpy()
    out["host/gt_inst_id"] = U.add_inst_num(gt_df.copy(), key="gt_inst_id", group_keys=keys)["gt_inst_id"].to_numpy()
    out["host/top_all"] = np.asarray(U.get_top_n_ids(pred_df.copy(), group_keys=keys, top_key="score"), np.int64)
    out["host/top_2"] = np.asarray(U.get_top_n_ids(pred_df.copy(), group_keys=keys, top_key="score", n_top=2), np.int64)
    out["host/top_targets"] = np.asarray(U.get_top_n_ids(pred_df.copy(), group_keys=keys, top_key="score", targets=targets_df), np.int64)
    out["host/valid_all"] = U.add_valid_gt(gt_df.copy(), group_keys=keys)["valid"].to_numpy(dtype=bool)
    out["host/valid_visib"] = U.add_valid_gt(gt_df.copy(), group_keys=keys, visib_gt_min=0.1)["valid"].to_numpy(dtype=bool)
    out["host/valid_visib_targets"] = U.add_valid_gt(gt_df.copy(), group_keys=keys, visib_gt_min=0.1,
                                                     targets=targets_df)["valid"].to_numpy(dtype=bool)
    gt_valid = U.add_valid_gt(gt_df.copy(), group_keys=keys, targets=targets_df)
    out["host/valid_targets"] = gt_valid["valid"].to_numpy(dtype=bool)
    for tag, only in (("cand", True), ("cand_all", False)):
        cands = U.get_candidate_matches(pred_df.copy(), gt_valid.copy(), group_keys=keys, only_valids=only)
        out[f"host/{tag}_pred_id"], out[f"host/{tag}_gt_id"] = cands["pred_id"].to_numpy(np.int64), cands["gt_id"].to_numpy(np.int64)
    cands = U.get_candidate_matches(pred_df.copy(), gt_valid.copy(), group_keys=keys, only_valids=True)
    err = np.random.RandomState(14).choice([0.002, 0.004, 0.004, 0.01, 0.03], size=len(cands)) + 0.0
    err[::11] = np.inf
    cands["error"] = err
    matches = U.match_poses(cands.copy(), group_keys=keys)
    out["host/cand_error"] = err
    out["host/match_cand_id"] = matches["cand_id"].to_numpy().astype(np.int64)
    out["host/match_pred_id"] = matches["pred_id"].to_numpy().astype(np.int64)
    out["host/match_gt_id"] = matches["gt_id"].to_numpy().astype(np.int64)
    rs = np.random.RandomState(15)
    auc_in = np.stack([rs.uniform(0, 0.15, 40), rs.uniform(0, 0.02, 40), np.r_[rs.uniform(0, 0.12, 30), np.full(10, np.inf)],
                       np.round(rs.uniform(0, 0.12, 40), 2)])
    out["host/auc_errors"], out["host/auc"] = auc_in, np.array([U.compute_auc_posecnn(e) for e in auc_in])
    out["host/auc_none"] = np.array(U.compute_auc_posecnn(np.full(5, 0.2)))
    print(f"host: {len(pred_df)} preds, {len(gt_df)} gt, {len(targets_df)} targets, {len(cands)} candidates, {len(matches)} matches, "
          f"auc {out['host/auc']}")

    path = gg.OUT / "g12_pose_errors.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
