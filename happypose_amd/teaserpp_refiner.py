"""The second depth refiner of the reference (``InferenceConfig.depth_refiner = "teaserpp"``).

Mirrors ``TeaserppRefiner`` (``MP/inference/teaserpp_refiner.py:167-294``): render the depth of every prediction at full
image resolution, take the pixels where both the rendered and the measured depth are valid as 3D-3D correspondences, reduce
them by farthest-point sampling, solve a robust registration, replace the pose when enough correspondences are inliers of
the solution.  The per-prediction Python loop of the reference (pytorch3d sampling, ``teaserpp_python`` solver on the CPU)
is one batched call of ``hp_teaser_refine`` here.  The solver and the sampler are third-party code that is absent here and
are restated from their published definitions, with a deterministic greedy clique in place of the library's exact maximum
clique: parity with the library is unpinned (see ``csrc/teaser.hip`` for the definition and ``tests/teaserpp_ref.py`` for its
CPU restatement).

Differences from the reference that a caller can see:
  * ``use_farthest_point_sampling=False`` takes the evenly spaced correspondences ``floor(k N / M)``; the reference draws
    unseeded random indices there, which no test could pin;
  * ``n_points`` is limited to 1024 (the reference's default is 1000);
  * ``extra_data`` holds the status, inlier count and clique size of EVERY prediction and the rendered depth, not the
    solver's debug output of the last one.
As in the reference, ``masks`` is accepted and not used.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from ._ffi import check, lib, ptr, stream_ptr
from .icp_refiner import DepthRefiner
from .renderer import BatchRenderer, Panda3dLightData

MAX_POINTS = 1024
MASK_TYPES = ("simple", "threshold")


class TeaserppRefiner(DepthRefiner):
    """``TeaserppRefiner(mesh_db, renderer, ...)`` with the reference's constructor.  ``retval`` per prediction: 0 accepted,
    -1 fewer than ``n_min_points`` masked pixels, -2 consistency clique smaller than 3, -3 fewer than ``min_num_inliers``
    inliers; the pose is unchanged unless it is 0."""

    def __init__(self, mesh_db, renderer: BatchRenderer, mask_type: str = "simple", depth_delta_thresh: float = 0.1,
                 n_min_points: int = 100, n_points: int = 1000, noise_bound: float = 0.01, min_num_inliers: int = 50,
                 use_farthest_point_sampling: bool = True) -> None:
        if mask_type not in MASK_TYPES:
            raise ValueError(f"Unknown mask type {mask_type}")  # the reference raises it from compute_masks
        if not 1 <= n_points <= MAX_POINTS:
            raise ValueError(f"n_points must be in 1 .. {MAX_POINTS}, got {n_points}")
        self.mesh_db = mesh_db
        self.renderer = renderer
        self.mask_type = mask_type
        self.depth_delta_thresh = depth_delta_thresh
        self.n_min_points = n_min_points
        self.n_points = n_points
        self.noise_bound = noise_bound
        self.min_num_inliers = min_num_inliers
        self.use_farthest_point_sampling = use_farthest_point_sampling
        self.light_datas = [Panda3dLightData("ambient")]

    def refine_poses(self, predictions, masks: Optional[torch.Tensor] = None, depth: Optional[torch.Tensor] = None,
                     K: Optional[torch.Tensor] = None):
        assert depth is not None
        assert K is not None
        dev = self.renderer.device
        refined = predictions.clone()
        N = len(predictions)
        if N == 0:
            return refined, {}
        depth = depth.to(dev, torch.float32)
        if depth.dim() == 4:
            depth = depth[:, 0]
        depth = depth.contiguous()
        B, H, W = depth.shape
        df = predictions.infos
        labels = df.label.tolist()
        im_ids_h = np.ascontiguousarray(df.batch_im_id.to_numpy(), dtype=np.int32)
        im_ids = torch.as_tensor(im_ids_h, device=dev)
        TCO = predictions.poses.to(dev, torch.float32).contiguous()
        K_ = K.to(dev, torch.float32)[im_ids.long()].contiguous()
        render = self.renderer.render(labels, TCO=TCO, K=K_, light_datas=[self.light_datas] * N, resolution=(H, W),
                                      render_depth=True)
        depth_rendered = render.depths.reshape(N, H, W).contiguous()
        out = torch.empty_like(TCO)
        retval = torch.empty(N, dtype=torch.int32, device=dev)
        num_inliers = torch.empty(N, dtype=torch.int32, device=dev)
        clique_size = torch.empty(N, dtype=torch.int32, device=dev)
        ws_bytes = lib().hp_teaser_workspace_bytes(N, H, W, self.n_points)
        assert ws_bytes >= 0, "hp_teaser_workspace_bytes: sizes out of range"
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib().hp_teaser_refine(N, B, H, W, ptr(depth_rendered), ptr(depth), ptr(im_ids),
                                         im_ids_h.ctypes.data_as(C.c_void_p), ptr(K_), ptr(TCO),
                                         int(self.mask_type == "threshold"), self.depth_delta_thresh, self.n_min_points,
                                         self.n_points, int(self.use_farthest_point_sampling), self.noise_bound,
                                         self.min_num_inliers, ptr(out), ptr(retval), ptr(num_inliers), ptr(clique_size),
                                         ptr(workspace), ws_bytes, stream_ptr(dev)), "hp_teaser_refine")
        # MP/inference/teaserpp_refiner.py:285: poses_input = the poses before refinement
        refined.register_tensor("poses_input", predictions.poses.clone())
        refined.register_tensor("poses", out.to(predictions.poses.device))
        return refined, {"retval": retval, "num_inliers": num_inliers, "clique_size": clique_size,
                         "depth_rendered": depth_rendered}
