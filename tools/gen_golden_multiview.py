#!/usr/bin/env python3
"""Generate ``tests/golden/g11_multiview.npz`` by running THE REFERENCE's multi-view candidate matching on seeded synthetic
scenes (``happypose_amd.synthetic.make_multiview_scene``: A, B, C, D of ``MULTIVIEW_SCENES``).

Runs only in the build container.  The reference's ``CP/multiview/ransac.py`` and ``CP/multiview/bundle_adjustment.py`` are
imported from where they lie through the namespace shim of ``tools/gen_golden.py``; the reference's C++ extension
(``CP/csrc/cosypose_cext.cpp``) is compiled with pybind11 into a temporary directory OUTSIDE the repository -- nothing compiled
is kept.  The reference's ``MeshDataBase.batched`` needs trimesh and pinocchio, so its own ``BatchedMeshes(infos, labels,
points, symmetries)`` is handed this repository's tables (``mesh_store.MeshDataBase.batched(aabb=True, n_sym=64)``: symmetry
table parity unpinned).

Stored per scene ``<s>`` (arrays only): the candidates after the score filter (``<s>/view_id``, ``label_id``, ``score``,
``poses``), ``<s>/cameras_TWC`` (D), the reference's seeds ``<s>/seeds`` [6, n] and tentative matches ``<s>/tmatches`` [3, n],
``<s>/TC1C2``, ``<s>/dists``, ``<s>/inlier_cand1`` / ``inlier_cand2`` / ``best_hypotheses``, the matched candidates
``<s>/matched_cand_id`` / ``matched_obj_id``, ``<s>/pairs_view1`` / ``pairs_view2`` / ``pairs_TC1C2`` and the view groups
``<s>/group_view_id`` / ``group_view_group``; from the reference's ``MultiviewScenePredictor.predict_scene_state`` on the same
scene (all candidates, score filter inside): ``<s>/cameras_K``, the bundle adjustment's object / view order (``ba_obj_id``,
``ba_obj_label_id``, ``ba_view_id``), its initialisation (``ba_init_TWO`` / ``ba_init_TWC`` = ``sample_initial_TWO_TWC(0)``,
``ba_init_reproj_dists`` = ``symmetric_distance_reprojected`` there), the history (``ba_loss``, ``ba_lambda``, ``ba_TWO_9d``,
``ba_TCW_9d``; an accepted step is a change of the 9d rows), the result (``ba_TWO``, ``ba_TWC``) and ``ba_output`` (poses,
obj_id, view_id); plus the mesh tables ``points`` / ``symmetries`` / ``n_sym``.

Usage:  python tools/gen_golden_multiview.py
"""

from __future__ import annotations

import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

import gen_golden as gg  # noqa: E402

CP = "happypose.pose_estimators.cosypose.cosypose"
SEED_COLUMNS = ("view1", "view2", "match1_cand1", "match1_cand2", "match2_cand1", "match2_cand2")
SCORE_TH, DIST_THRESHOLD, N_MIN_INLIERS = 0.3, 0.02, 3  # the reference's defaults


def build_reference_extension() -> None:
    import pybind11

    tmp = Path(tempfile.mkdtemp(prefix="cosypose_cext_"))
    suffix = subprocess.check_output([sys.executable, "-c", "import sysconfig; print(sysconfig.get_config_var('EXT_SUFFIX'))"],
                                     text=True).strip()
    import sysconfig

    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", f"-I{pybind11.get_include()}",
                           f"-I{sysconfig.get_paths()['include']}",
                           str(gg.REF / "happypose/pose_estimators/cosypose/cosypose/csrc/cosypose_cext.cpp"),
                           "-o", str(tmp / f"cosypose_cext{suffix}")])
    sys.path.insert(0, str(tmp))


def main():
    import pandas as pd
    import torch

    from happypose_amd.mesh_store import MeshDataBase
    from happypose_amd.synthetic import MULTIVIEW_SCENES, make_multiview_objects, make_multiview_scene

    gg._shim()
    build_reference_extension()
    ransac = gg.imp(f"{CP}.multiview.ransac")
    ba = gg.imp(f"{CP}.multiview.bundle_adjustment")
    rmd = gg.imp(f"{CP}.lib3d.rigid_mesh_database")
    tc = gg.imp(f"{CP}.utils.tensor_collection")

    ds = make_multiview_objects()
    mine = MeshDataBase.from_object_ds(ds).batched(aabb=True, n_sym=64)
    mesh_db = rmd.BatchedMeshes(mine.infos, mine.labels, torch.as_tensor(mine.points), torch.as_tensor(mine.symmetries)).float()
    out = {"points": mine.points, "symmetries": mine.symmetries, "n_sym": mine.n_sym}

    captured = {}
    make_infos, find_inliers = ransac.cosypose_cext.make_ransac_infos, ransac.cosypose_cext.find_ransac_inliers
    est, score = ransac.estimate_camera_poses_batch, ransac.score_tmaches_batch

    class Ext:  # records what passes between the reference's own stages; computes nothing
        scatter_argmin = staticmethod(ransac.cosypose_cext.scatter_argmin)
        expand_ids_for_symmetry = staticmethod(ransac.cosypose_cext.expand_ids_for_symmetry)

        @staticmethod
        def make_ransac_infos(*a):
            captured["seeds"], captured["tmatches"] = make_infos(*a)
            return captured["seeds"], captured["tmatches"]

        @staticmethod
        def find_ransac_inliers(*a):
            captured["inliers"] = find_inliers(*a)
            return captured["inliers"]

    def score_rec(candidates, tmatches, TC1C2, mesh_db, bsz=4096):
        captured["TC1C2"] = TC1C2
        captured["dists"] = score(candidates, tmatches, TC1C2, mesh_db, bsz=bsz)
        return captured["dists"]

    ransac.cosypose_cext = Ext
    ransac.score_tmaches_batch = score_rec

    for name, (n_iter, known) in MULTIVIEW_SCENES.items():
        sc = make_multiview_scene(name)
        keep = np.where(sc["score"] >= SCORE_TH)[0]
        infos = pd.DataFrame({"view_id": sc["view_id"][keep], "label": mine.labels[sc["label_id"][keep]], "score": sc["score"][keep]})
        candidates = tc.PandasTensorCollection(infos=infos, poses=torch.as_tensor(sc["poses"][keep]))
        cameras = None
        if known:
            cameras = tc.PandasTensorCollection(infos=pd.DataFrame({"view_id": np.arange(len(sc["TWC"]))}),
                                                TWC=torch.as_tensor(sc["TWC"], dtype=torch.float32))
            out[f"{name}/cameras_TWC"] = cameras.TWC.numpy()
        captured.clear()
        res = ransac.multiview_candidate_matching(candidates, mesh_db, dist_threshold=DIST_THRESHOLD, cameras=cameras,
                                                  n_ransac_iter=n_iter, n_min_inliers=N_MIN_INLIERS)
        groups = ba.make_view_groups(res["pairs_TC1C2"])
        out.update({
            f"{name}/view_id": sc["view_id"][keep], f"{name}/label_id": sc["label_id"][keep], f"{name}/score": sc["score"][keep],
            f"{name}/poses": sc["poses"][keep], f"{name}/n_ransac_iter": np.int64(n_iter),
            f"{name}/seeds": np.stack([captured["seeds"][k] for k in SEED_COLUMNS]).astype(np.int32),
            f"{name}/tmatches": np.stack([captured["tmatches"][k] for k in ("hypothesis_id", "cand1", "cand2")]).astype(np.int32),
            f"{name}/TC1C2": captured["TC1C2"].numpy(), f"{name}/dists": captured["dists"].numpy(),
            f"{name}/inlier_cand1": captured["inliers"]["inlier_matches_cand1"].astype(np.int32),
            f"{name}/inlier_cand2": captured["inliers"]["inlier_matches_cand2"].astype(np.int32),
            f"{name}/best_hypotheses": captured["inliers"]["best_hypotheses"].astype(np.int32),
            f"{name}/matched_cand_id": res["filtered_candidates"].infos["cand_id"].values.astype(np.int64),
            f"{name}/matched_obj_id": res["filtered_candidates"].infos["obj_id"].values.astype(np.int64),
            f"{name}/pairs_view1": res["pairs_TC1C2"].infos["view1"].values.astype(np.int64),
            f"{name}/pairs_view2": res["pairs_TC1C2"].infos["view2"].values.astype(np.int64),
            f"{name}/pairs_TC1C2": res["pairs_TC1C2"].TC1C2.numpy(),
            f"{name}/group_view_id": groups["view_id"].values.astype(np.int64),
            f"{name}/group_view_group": groups["view_group"].values.astype(np.int64),
        })
        print(f"scene {name}: {len(keep)} candidates, {out[f'{name}/seeds'].shape[1]} seeds, {out[f'{name}/tmatches'].shape[1]} rows, "
              f"{len(out[f'{name}/best_hypotheses'])} view pairs, {len(out[f'{name}/matched_cand_id'])} matched, "
              f"groups {out[f'{name}/group_view_group'].tolist()}, dists {np.sort(out[f'{name}/dists'])[[0, -1]]}")
    # ---- the bundle adjustment: the reference's MultiviewScenePredictor.predict_scene_state on the same scenes ----------------
    mvp = gg.imp(f"{CP}.integrated.multiview_predictor")
    predictor = object.__new__(mvp.MultiviewScenePredictor)  # its __init__ only builds the two mesh tables (trimesh)
    predictor.mesh_db_ransac = predictor.mesh_db_ba = mesh_db
    solved = []
    solve = ba.MultiviewRefinement.solve

    def solve_rec(self, *a, **k):
        res = solve(self, *a, **k)
        TWO_9d0, TCW_9d0 = res["history"]["TWO_9d"][0], res["history"]["TCW_9d"][0]
        with torch.no_grad():
            init_dists, _ = self.align_TCO_cand(TWO_9d0, TCW_9d0)
        solved.append((self, res, init_dists))
        return res

    ba.MultiviewRefinement.solve = solve_rec
    for name, (n_iter, known) in MULTIVIEW_SCENES.items():
        sc = make_multiview_scene(name)
        n = len(sc["view_id"])
        infos = pd.DataFrame({"scene_id": np.zeros(n, int), "group_id": np.zeros(n, int), "view_id": sc["view_id"],
                              "label": mine.labels[sc["label_id"]], "score": sc["score"], "batch_im_id": sc["view_id"]})
        candidates = tc.PandasTensorCollection(infos=infos, poses=torch.as_tensor(sc["poses"]))
        n_views = len(sc["TWC"])
        cameras = tc.PandasTensorCollection(infos=pd.DataFrame({"scene_id": np.zeros(n_views, int), "view_id": np.arange(n_views),
                                                                "batch_im_id": np.arange(n_views)}),
                                            K=torch.as_tensor(sc["K"], dtype=torch.float32),
                                            TWC=torch.as_tensor(sc["TWC"], dtype=torch.float32))
        out[f"{name}/cameras_K"] = cameras.K.numpy()
        solved.clear()
        pred = predictor.predict_scene_state(candidates, cameras, score_th=SCORE_TH, use_known_camera_poses=known,
                                             ransac_n_iter=n_iter, ransac_dist_threshold=DIST_THRESHOLD)
        assert len(solved) == 1  # one view group in every scene
        problem, res, init_dists = solved[0]
        hist = res["history"]
        out.update({
            f"{name}/ba_obj_id": problem.obj_infos["obj_id"].values.astype(np.int64),
            f"{name}/ba_obj_label_id": mine.ids_of(problem.obj_infos["label"].values).astype(np.int64),
            f"{name}/ba_view_id": problem.cam_infos["view_id"].values.astype(np.int64),
            f"{name}/ba_init_TWO": res["objects_init"].TWO.numpy(), f"{name}/ba_init_TWC": res["cameras_init"].TWC.numpy(),
            f"{name}/ba_init_reproj_dists": init_dists.numpy(),
            f"{name}/ba_loss": np.array([float(x) for x in hist["loss"]], np.float32),
            f"{name}/ba_lambda": np.array(hist["lambda"], np.float64),
            f"{name}/ba_TWO_9d": torch.stack(hist["TWO_9d"]).detach().numpy(),
            f"{name}/ba_TCW_9d": torch.stack(hist["TCW_9d"]).detach().numpy(),
            f"{name}/ba_TWO": res["objects"].TWO.detach().numpy(), f"{name}/ba_TWC": res["cameras"].TWC.detach().numpy(),
            f"{name}/ba_output_poses": pred["ba_output"].poses.detach().numpy(),
            f"{name}/ba_output_obj_id": pred["ba_output"].infos["obj_id"].values.astype(np.int64),
            f"{name}/ba_output_view_id": pred["ba_output"].infos["view_id"].values.astype(np.int64),
        })
        print(f"scene {name}: BA {len(hist['loss'])} iterations, loss {out[f'{name}/ba_loss'][0]:.5f} -> {out[f'{name}/ba_loss'][-1]:.5f}, "
              f"lambda {hist['lambda'][-1]:.2e}, keys {sorted(pred)}")
    path = gg.OUT / "g11_multiview.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
