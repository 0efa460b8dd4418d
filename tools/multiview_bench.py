#!/usr/bin/env python3
"""Time the multi-view candidate matching and the bundle adjustment on seeded synthetic scenes of 4 x 10, 6 x 24 and 8 x 40
(views x candidates per view) at the reference's defaults (``ransac_n_iter=2000``, ``n_sym=64``, box-corner points), beside the
same steps written with plain torch ops on the device (a restatement kept in this tool: the reference's batched formulation --
``[rows, S, 4, 4]`` temporaries chunked at ``score_bsz``, dense autograd Jacobian -- NOT the reference itself, whose extension
and mesh loader are not dependencies).  Information, not a threshold.

Usage:  python tools/multiview_bench.py [--sizes 4x10,6x24,8x40] [--repeats 3] [--ba-iterations 10]
Prints one JSON line per size: milliseconds per step, median of the repeats, after one warm-up run.
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from happypose_amd import multiview as mv, ops  # noqa: E402
from happypose_amd.mesh_store import MeshDataBase  # noqa: E402
from happypose_amd.synthetic import make_multiview_objects, make_multiview_scene  # noqa: E402
from happypose_amd.tensor_collection import PandasTensorCollection  # noqa: E402


def timed(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), res


def torch_symmetric_distance(T1, T2, obj, pts, sym, bsz):
    """symmetric_distance_batched_fast, chunked (CP/lib3d/symmetric_distances.py:36-55)."""
    out = []
    for i in range(0, len(T1), bsz):
        t1, t2, o = T1[i:i + bsz], T2[i:i + bsz], obj[i:i + bsz]
        p = pts[o]
        M = t1.unsqueeze(1) @ sym[o]
        a = p.unsqueeze(1) @ M[..., :3, :3].transpose(-1, -2) + M[..., None, :3, 3]
        b = (p @ t2[:, :3, :3].transpose(-1, -2) + t2[:, None, :3, 3]).unsqueeze(1)
        d2 = ((a - b) ** 2).sum(-1)
        best = d2.mean(-1).argmin(1)
        out.append(torch.sqrt(d2[torch.arange(len(t1), device=t1.device), best]).mean(-1))
    return torch.cat(out)


def torch_matching(poses, obj, seeds, tm, pts, sym, n_sym, model_bsz=1000, score_bsz=100000):
    """estimate_camera_poses_batch + score_tmaches_batch (CP/multiview/ransac.py:23-99) with torch ops on the device."""
    dev = poses.device
    a, b, g, d = (torch.as_tensor(seeds[k], dtype=torch.long, device=dev) for k in ops._SEED_COLUMNS[2:])
    inv = mv.invert_transform_matrices(poses)
    TC1C2 = []
    for i in range(0, len(a), model_bsz):
        ai, bi, gi, di = a[i:i + model_bsz], b[i:i + model_bsz], g[i:i + model_bsz], d[i:i + model_bsz]
        S = sym[obj[ai]]  # [n, S_max, 4, 4]; rows past n_sym are identity: duplicates of index 0, which wins the tie
        n, s_max = S.shape[:2]
        T2 = (poses[ai].unsqueeze(1) @ S @ inv[bi].unsqueeze(1)) @ poses[di].unsqueeze(1)
        dist = torch_symmetric_distance(poses[gi].repeat_interleave(s_max, 0), T2.reshape(-1, 4, 4), obj[gi].repeat_interleave(s_max),
                                        pts, sym, score_bsz).view(n, s_max)
        best = dist.argmin(1)
        TC1C2.append(poses[ai] @ S[torch.arange(n, device=dev), best] @ inv[bi])
    TC1C2 = torch.cat(TC1C2)
    h, c1, c2 = (torch.as_tensor(tm[k], dtype=torch.long, device=dev) for k in ("hypothesis_id", "cand1", "cand2"))
    out = []
    for i in range(0, len(h), score_bsz):  # gathers chunked as well: [rows, 4, 4] of the whole table is itself large
        hi, c1i, c2i = h[i:i + score_bsz], c1[i:i + score_bsz], c2[i:i + score_bsz]
        out.append(torch_symmetric_distance(poses[c1i], TC1C2[hi] @ poses[c2i], obj[c1i], pts, sym, score_bsz))
    return TC1C2, torch.cat(out)


def torch_ba_linearize(problem, TWO_9d, TCW_9d, aligned):
    """forward_jacobian with torch autograd on the device (CP/multiview/bundle_adjustment.py:223-270): dense J, J^T J, J^T e."""
    dev = TWO_9d.device
    co = torch.as_tensor(problem.cand_obj_ids, device=dev)
    cv = torch.as_tensor(problem.cand_view_ids, device=dev)
    pts, K = problem.obj_points[co], problem.K[cv]
    n_two = TWO_9d.numel()

    def project(T):
        suv = (pts @ T[:, :3, :3].transpose(-1, -2) + T[:, None, :3, 3]) @ K.transpose(-1, -2)
        return suv[..., :2] / suv[..., 2:]

    def yhat(theta):
        TWO = mv.compute_transform_from_pose9d(theta[:n_two].view(-1, 9))
        TCW = mv.compute_transform_from_pose9d(theta[n_two:].view(-1, 9))
        return project(TCW[cv] @ TWO[co]).reshape(-1)

    theta = torch.cat((TWO_9d.reshape(-1), TCW_9d.reshape(-1))).float()
    J = torch.autograd.functional.jacobian(yhat, theta)
    e = project(aligned).reshape(-1) - yhat(theta)
    return J.T @ J, J.T @ e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4x10,6x24,8x40")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ba-iterations", type=int, default=10)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    db = MeshDataBase.from_object_ds(make_multiview_objects())
    mesh_db = db.batched(aabb=True, n_sym=64).to(dev)
    t = mesh_db.device_tables
    for size in args.sizes.split(","):
        n_views, n_per_view = (int(x) for x in size.split("x"))
        sc = make_multiview_scene("scale", n_views=n_views, n_objects=n_per_view)
        infos = pd.DataFrame({"view_id": sc["view_id"], "label": [f"mv_{i}" for i in sc["label_id"]], "score": sc["score"]})
        cand = PandasTensorCollection(infos=infos, poses=torch.as_tensor(sc["poses"], device=dev))
        cams = PandasTensorCollection(infos=pd.DataFrame({"view_id": np.arange(n_views)}), K=torch.as_tensor(sc["K"], dtype=torch.float32))
        seeds, tm = ops.ransac_make_infos(sc["view_id"], sc["label_id"], 2000, 0)
        line = {"size": size, "candidates": len(cand), "seeds": len(seeds["view1"]), "rows": len(tm["cand1"])}
        obj = torch.as_tensor(sc["label_id"], device=dev)
        line["hip_estimate_ms"], TC1C2 = timed(lambda: ops.mv_estimate_camera_poses(cand.poses, sc["label_id"], seeds, mesh_db), args.repeats)
        line["hip_score_ms"], _ = timed(lambda: ops.mv_score_seed_matches(seeds, tm, TC1C2, cand.poses, sc["label_id"], mesh_db), args.repeats)
        line["matching_total_ms"], out = timed(lambda: mv.multiview_candidate_matching(cand, mesh_db, n_ransac_iter=2000), args.repeats)
        if not args.skip_torch:
            line["torch_estimate_and_score_ms"], _ = timed(
                lambda: torch_matching(cand.poses, obj, seeds, tm, t["points"], t["symmetries"], t["n_sym"]), args.repeats)
        groups = mv.make_view_groups(out["pairs_TC1C2"])
        matched = out["filtered_candidates"].merge_df(groups, on="view_id").to(dev)
        problem = mv.MultiviewRefinement(matched[np.where(matched.infos["view_group"] == 0)[0]], cams, out["pairs_TC1C2"], mesh_db)
        TWO_9d, TCW_9d = problem.robust_initialization_TWO_TCW()
        line["ba_objects"], line["ba_views"], line["ba_candidates"] = problem.n_objects, problem.n_views, problem.n_candidates
        line["hip_ba_linearize_ms"], _ = timed(lambda: problem.forward_jacobian(TWO_9d, TCW_9d, 25.0), args.repeats)
        line["ba_lm_ms"], _ = timed(lambda: problem.optimize_lm(TWO_9d, TCW_9d, n_iterations=args.ba_iterations), args.repeats)
        line["ba_lm_iterations"] = args.ba_iterations
        if not args.skip_torch:
            _, aligned = problem.align_TCO_cand(TWO_9d, TCW_9d)
            line["torch_ba_linearize_ms"], _ = timed(lambda: torch_ba_linearize(problem, TWO_9d, TCW_9d, aligned), args.repeats)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in line.items()}), flush=True)


if __name__ == "__main__":
    main()
