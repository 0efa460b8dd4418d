"""Multi-object scenes: the reference's scene renderer and the visualisations built on it.

``SceneRenderer.render_scene`` has the signature and return type of ``Panda3dSceneRenderer.render_scene``
(``TB/renderer/panda3d_scene_renderer.py:320-390``); ``CameraRenderingData`` / ``Panda3dObjectData`` / ``Panda3dCameraData`` mirror
``TB/renderer/types.py:76-99,153-161``; ``make_contour_overlay`` mirrors ``TB/visualization/utils.py:54-82``, ``make_overlay`` is
``BokehPlotter.plot_overlay`` (``TB/visualization/bokeh_plotter.py:116-141``), ``render_prediction_wrt_camera`` is
``CP/visualization/singleview.py:24-38`` and ``make_poses_visualization`` is ``TB/inference/example_inference_utils.py:123-175``.

The rasteriser draws one object per view, so a scene is rendered as LAYERS -- one view per (camera, object) pair, sorted by
camera -- that ``csrc/scene.hip`` merges per pixel (``ops.scene_compose``); instance ids, the BOP gt-info quantities
(``scene_visibility``), outlines and overlays come from the same file.  Limitation: every layer is resolved on its
own, 4x multisampled against black, so where a nearer silhouette crosses a farther object the edge pixels blend with black in a
band at most one pixel wide; depth, ids, mask and visibility are exact, and with ``msaa=False`` so is the colour.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from .mesh_store import RigidObjectDataset
from .renderer import BatchRenderer, LightNodeProxy, Panda3dLightData, SceneRootProxy

RgbaColor = Tuple[float, float, float, float]
Resolution = Tuple[int, int]  # (h, w)
DEFAULT_LAYER_BUDGET_BYTES = 512 << 20  # layer buffers alive at once (30 objects x 8 cameras at 480 x 640 would be 2 GB)


def _as_matrix(T) -> np.ndarray:
    """4 x 4 float64 of whatever the reference's callers pass as a pose: an array / tensor, a ``Transform``-like object
    (``toHomogeneousMatrix()``) or a ``(quaternion xyzw, translation)`` pair."""
    if hasattr(T, "toHomogeneousMatrix"):
        T = T.toHomogeneousMatrix()
    if isinstance(T, torch.Tensor):
        T = T.detach().cpu().numpy()
    if isinstance(T, (tuple, list)) and len(T) == 2 and len(T[0]) == 4 and len(T[1]) == 3:
        x, y, z, w = (float(v) for v in T[0])
        M = np.eye(4)
        M[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        M[:3, 3] = T[1]
        return M
    M = np.asarray(T, dtype=np.float64)
    assert M.shape == (4, 4), f"a pose is a 4 x 4 matrix, got shape {M.shape}"
    return M


@dataclass
class CameraRenderingData:
    """``TB/renderer/types.py:76-88``: rgb (h, w, 3) uint8; normals (h, w, 3) uint8; depth (h, w, 1) float32; binary_mask
    (h, w, 1) bool."""

    rgb: np.ndarray
    normals: Optional[np.ndarray] = None
    depth: Optional[np.ndarray] = None
    binary_mask: Optional[np.ndarray] = None


@dataclass
class Panda3dObjectData:
    """``TB/renderer/types.py:153-161``."""

    label: str
    TWO: Any = field(default_factory=lambda: np.eye(4))
    color: Optional[RgbaColor] = None
    material: Any = None
    remove_mesh_material: bool = False
    scale: float = 1
    positioning_function: Optional[Callable] = None

    def __post_init__(self):
        self.TWO = _as_matrix(self.TWO)


@dataclass
class Panda3dCameraData:
    """``TB/renderer/types.py:91-99``; ``resolution`` is (h, w)."""

    K: np.ndarray
    resolution: Resolution
    TWC: Any = field(default_factory=lambda: np.eye(4))
    z_near: float = 0.1
    z_far: float = 10
    node_name: str = "camera"
    positioning_function: Optional[Callable] = None

    def __post_init__(self):
        self.TWC = _as_matrix(self.TWC)


def _object_data(o) -> Panda3dObjectData:
    """An object as the callers pass it: the dataclass, anything with ``label`` / ``TWO`` (``ObjectData``), or the plain dict of
    ``render_prediction_wrt_camera`` (``name``, ``TWO``, ``color``)."""
    if isinstance(o, Panda3dObjectData):
        return o
    if isinstance(o, dict):
        known = {"name", "label", "TWO", "color", "material", "remove_mesh_material", "scale", "positioning_function"}
        assert set(o) <= known, f"unknown object keys {sorted(set(o) - known)}"
        label = o["label"] if "label" in o else o["name"]
        return Panda3dObjectData(label=label, **{k: v for k, v in o.items() if k not in ("name", "label")})
    return Panda3dObjectData(label=o.label, TWO=o.TWO, **{k: getattr(o, k) for k in ("color", "material", "scale", "positioning_function") if hasattr(o, k)})


def _camera_data(c) -> Panda3dCameraData:
    if isinstance(c, Panda3dCameraData):
        return c
    if isinstance(c, dict):
        return Panda3dCameraData(K=c["K"], resolution=tuple(c["resolution"]), TWC=c.get("TWC", np.eye(4)),
                                 **{k: c[k] for k in ("z_near", "z_far", "positioning_function") if k in c})
    return Panda3dCameraData(K=c.K, resolution=tuple(c.resolution), TWC=c.TWC if getattr(c, "TWC", None) is not None else np.eye(4),
                             **{k: getattr(c, k) for k in ("z_near", "z_far", "positioning_function") if hasattr(c, k)})


def _check_supported(objects: Sequence[Panda3dObjectData], cameras: Sequence[Panda3dCameraData]) -> None:
    """What the layer renderer does not draw is refused, never approximated."""
    for o in objects:
        if o.scale != 1:
            raise NotImplementedError(f"object {o.label!r}: scale = {o.scale} (only 1: the mesh store holds the objects at their own size)")
        if o.material is not None:
            raise NotImplementedError(f"object {o.label!r}: a Panda3D material")
        if o.color is not None and tuple(float(v) for v in o.color) != (1.0, 1.0, 1.0, 1.0):
            raise NotImplementedError(f"object {o.label!r}: color = {tuple(o.color)} (only None or (1, 1, 1, 1): objects keep their texture)")
        if o.positioning_function is not None:
            raise NotImplementedError(f"object {o.label!r}: a positioning_function needs a scene graph; pass TWO")
    for i, c in enumerate(cameras):
        if float(c.z_near) != 0.1 or float(c.z_far) != 10.0:
            raise NotImplementedError(f"camera {i}: z_near / z_far = {c.z_near} / {c.z_far} (the rasteriser's clip range is [0.1, 10] m)")
        if c.positioning_function is not None:
            raise NotImplementedError(f"camera {i}: a positioning_function needs a scene graph; pass TWC")


@dataclass
class LayerGroup:
    """The layers of the cameras that share one resolution, sorted by camera: layer ``layer_off[i] + j`` is object ``j`` seen
    by camera ``cameras[i]`` (indices into the caller's lists)."""

    resolution: Resolution
    cameras: List[int]
    layer_off: np.ndarray     # [len(cameras) + 1] int32
    layer_camera: np.ndarray  # [L] int32: index into the caller's camera list
    layer_object: np.ndarray  # [L] int32: index into the caller's object list
    TCO: np.ndarray           # [L, 4, 4] float32 = inv(TWC) @ TWO
    K: np.ndarray             # [L, 3, 3] float32


def plan_layers(object_datas: Sequence, camera_datas: Sequence) -> List[LayerGroup]:
    """Group the cameras by resolution (first appearance orders the groups, the caller's order the cameras inside one) and
    lay out one layer per (camera, object) with ``TCO = inv(TWC) @ TWO`` (float64 product, stored as float32)."""
    objects = [_object_data(o) for o in object_datas]
    cameras = [_camera_data(c) for c in camera_datas]
    groups: Dict[Resolution, List[int]] = {}
    for i, c in enumerate(cameras):
        res = (int(c.resolution[0]), int(c.resolution[1]))
        groups.setdefault(res, []).append(i)
    n_obj = len(objects)
    out = []
    for res, cams in groups.items():
        L = len(cams) * n_obj
        TCO, K = np.zeros((L, 4, 4), np.float32), np.zeros((L, 3, 3), np.float32)
        for i, ci in enumerate(cams):
            TCW = np.linalg.inv(_as_matrix(cameras[ci].TWC))
            for j, o in enumerate(objects):
                TCO[i * n_obj + j] = TCW @ _as_matrix(o.TWO)
                K[i * n_obj + j] = np.asarray(cameras[ci].K, dtype=np.float64).reshape(3, 3)
        out.append(LayerGroup(res, list(cams), (np.arange(len(cams) + 1) * n_obj).astype(np.int32),
                              np.repeat(np.asarray(cams, np.int32), n_obj), np.tile(np.arange(n_obj, dtype=np.int32), len(cams)), TCO, K))
    return out


def scene_bounds(centers: np.ndarray, radii: np.ndarray, TWO: Sequence[np.ndarray]) -> Tuple[np.ndarray, float]:
    """Bounding sphere of the scene root: the union of the objects' bounding spheres moved into the world frame, merged in
    object order (the smallest sphere around two spheres at each step).  An empty scene is a point at the origin."""
    c, r = np.zeros(3), 0.0
    for i, T in enumerate(TWO):
        ci = T[:3, :3] @ np.asarray(centers[i], np.float64) + T[:3, 3]
        ri = float(radii[i])
        if i == 0:
            c, r = ci, ri
            continue
        d = float(np.linalg.norm(ci - c))
        if d + ri <= r:
            continue
        if d + r <= ri:
            c, r = ci, ri
            continue
        nr = (d + r + ri) / 2
        c = c + (ci - c) * ((nr - r) / d)
        r = nr
    return c, r


def light_positions_in_object_frames(pos_world: np.ndarray, TWO: Sequence[np.ndarray]) -> np.ndarray:
    """World positions [n_lights, 3] -> [n_objects, n_lights, 3] in every object's own frame (``inv(TWO) @ p``): the rasteriser
    takes a layer's lights there."""
    pos_world = np.asarray(pos_world, np.float64).reshape(-1, 3)
    out = np.zeros((len(TWO), len(pos_world), 3), np.float32)
    for i, T in enumerate(TWO):
        TOW = np.linalg.inv(T)
        out[i] = pos_world @ TOW[:3, :3].T + TOW[:3, 3]
    return out


def scene_lights(light_datas: Sequence[Panda3dLightData], center: np.ndarray, radius: float):
    """``setup_lights`` (``TB/renderer/panda3d_scene_renderer.py:294-318``) on the scene root's proxy: ``(ambient [3], world
    positions [n, 3], colours [n, 3])``."""
    amb, pos, col = np.zeros(3, np.float32), [], []
    for l in light_datas:
        if l.light_type == "ambient":
            amb += np.asarray(l.color[:3], np.float32)
        elif l.light_type == "point":
            if l.positioning_function is not None:
                node = LightNodeProxy()
                l.positioning_function(SceneRootProxy(center, radius), node)
                pos.append(np.asarray(node.pos, np.float64))
            elif getattr(l, "direction", None) is not None:
                pos.append(np.asarray(l.direction, np.float64) * radius * l.radius_factor)
            else:
                raise AssertionError("a point light needs a positioning_function")
            col.append(np.asarray(l.color[:3], np.float32))
        else:
            raise NotImplementedError(l.light_type)
    return amb, np.asarray(pos, np.float64).reshape(-1, 3), np.asarray(col, np.float32).reshape(-1, 3)


def overlay_tables() -> Tuple[np.ndarray, np.ndarray]:
    """``(lut_render, lut_input)``: the two branches of ``BokehPlotter.plot_overlay`` for every byte value, evaluated by the
    reference's own numpy expression (uint8 array times Python float, stored to float32, truncated to uint8)."""
    v = np.arange(256, dtype=np.uint8)
    lut_render, lut_input = np.zeros(256, np.float32), np.zeros(256, np.float32)
    lut_render[:] = v * 0.8 + 255 * 0.2
    lut_input[:] = v * 0.6 + 255 * 0.4
    return lut_render.astype(np.uint8), lut_input.astype(np.uint8)


def _to_u8_hwc(x: torch.Tensor) -> torch.Tensor:
    """[n, 3, h, w] float in [0, 1] on the 8-bit grid -> [n, h, w, 3] uint8."""
    return (x * 255.0 + 0.5).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


class SceneRenderer:
    """``Panda3dSceneRenderer`` replacement.  Pass ``renderer=`` (a ``BatchRenderer``) or ``store=`` to share the device-resident
    meshes; the render state defaults to the reference's like ``BatchRenderer``'s (``msaa=True``, ``aniso=True``).
    ``layer_budget_bytes`` bounds the layer buffers alive at once."""

    def __init__(self, asset_dataset: Optional[RigidObjectDataset] = None, preload_labels=None, debug: bool = False, verbose: bool = False,
                 device="cuda", renderer: Optional[BatchRenderer] = None, store: Optional[ops.MeshStore] = None, msaa: Optional[bool] = None,
                 aniso: Optional[bool] = None, layer_budget_bytes: int = DEFAULT_LAYER_BUDGET_BYTES):
        if renderer is not None:
            store = renderer.store
            msaa = renderer.msaa if msaa is None else msaa
            aniso = renderer.aniso if aniso is None else aniso
        assert store is not None or asset_dataset is not None, "SceneRenderer needs an object dataset, a BatchRenderer or a MeshStore"
        self.store = store if store is not None else ops.MeshStore(asset_dataset, device)
        self.device = self.store.device
        self.msaa = True if msaa is None else bool(msaa)
        self.aniso = True if aniso is None else bool(aniso)
        self.layer_budget_bytes = int(layer_budget_bytes)
        self._luts = None

    # ------------------------------------------------------------------------------------------------------------- rendering
    def _layer_lights(self, objects, light_datas):
        """Per OBJECT: ambient [n_obj, 3], positions [n_obj, n_pts, 3] in the object's frame, colours [n_obj, n_pts, 3]."""
        packed = self.store.packed
        oid = [self.store.label_to_id[o.label] for o in objects]
        TWO = [o.TWO for o in objects]
        center, radius = scene_bounds(packed.bounds_center[oid], packed.bounds_radius[oid], TWO)
        amb, pos_w, col = scene_lights(light_datas, center, radius)
        n = len(objects)
        amb = np.tile(amb[None], (n, 1))
        if len(pos_w) == 0:
            return amb, None, None
        return amb, light_positions_in_object_frames(pos_w, TWO), np.tile(col[None], (n, 1, 1))

    def _rasterize(self, group: LayerGroup, sl: slice, obj_ids, lights, render_normals: bool):
        amb, pos, col = lights
        o = group.layer_object[sl]
        t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a[o]), device=self.device)  # noqa: E731
        rgb, nrm, dep, _ = ops.rasterize(self.store, obj_ids[sl], torch.as_tensor(group.TCO[sl]), torch.as_tensor(group.K[sl]), group.resolution,
                                         render_normals=render_normals, render_depth=True, ambient=t(amb), light_pos=t(pos), light_col=t(col),
                                         msaa=self.msaa, aniso=self.aniso)
        return rgb, nrm, dep

    def _render_group(self, group: LayerGroup, objects, lights, render_normals: bool, keep_layer_depth: bool) -> Dict[str, Any]:
        h, w = group.resolution
        n_obj, n_cam = len(objects), len(group.cameras)
        dev = self.device
        obj_ids = torch.as_tensor([self.store.label_to_id[objects[j].label] for j in group.layer_object], dtype=torch.int32).reshape(-1)
        layer_bytes = h * w * 4 * (4 + (3 if render_normals else 0))
        max_layers = max(1, self.layer_budget_bytes // layer_bytes)
        parts: List[Dict[str, torch.Tensor]] = []
        depths: List[torch.Tensor] = []
        if n_obj <= max_layers:  # whole cameras per chunk, one compose call each
            step = max(1, max_layers // max(n_obj, 1))
            for c0 in range(0, n_cam, step):
                c1 = min(n_cam, c0 + step)
                sl = slice(c0 * n_obj, c1 * n_obj)
                if n_obj:
                    rgb, nrm, dep = self._rasterize(group, sl, obj_ids, lights, render_normals)
                else:
                    rgb = torch.empty((0, 3, h, w), device=dev)
                    nrm = torch.empty((0, 3, h, w), device=dev) if render_normals else None
                    dep = torch.empty((0, 1, h, w), device=dev)
                parts.append(ops.scene_compose(np.arange(c1 - c0 + 1, dtype=np.int32) * n_obj, rgb, nrm, dep))
                if keep_layer_depth:
                    depths.append(dep)
        else:  # a camera's layers do not fit: merge them chunk by chunk, the composite so far going first (it wins ties)
            for c in range(n_cam):
                comp = None
                for o0 in range(0, n_obj, max_layers):
                    o1 = min(n_obj, o0 + max_layers)
                    rgb, nrm, dep = self._rasterize(group, slice(c * n_obj + o0, c * n_obj + o1), obj_ids, lights, render_normals)
                    if keep_layer_depth:
                        depths.append(dep)
                    if comp is None:
                        comp = ops.scene_compose([0, o1 - o0], rgb, nrm, dep)
                        continue
                    new = ops.scene_compose([0, o1 - o0 + 1], torch.cat([comp["rgb"], rgb]), torch.cat([comp["normals"], nrm]) if render_normals else None,
                                            torch.cat([comp["depth"], dep]))
                    k = new["ids"]  # 0: the composite so far (keeps its id), j > 0: object o0 + j - 1; index bookkeeping only
                    new["ids"] = torch.where(k == 0, comp["ids"], torch.where(k > 0, k + (o0 - 1), k))
                    comp = new
                parts.append(comp)
        out: Dict[str, Any] = {k: (torch.cat([p[k] for p in parts]) if parts[0][k] is not None else None) for k in ("rgb", "normals", "depth", "ids", "mask")}
        out["layer_camera"] = torch.as_tensor(group.layer_camera, device=dev)
        out["layer_object"] = torch.as_tensor(group.layer_object, device=dev)
        out["layer_off"] = group.layer_off
        out["cameras"] = list(group.cameras)
        out["resolution"] = group.resolution
        if keep_layer_depth:
            out["layer_depth"] = torch.cat(depths) if depths else torch.empty((0, 1, h, w), device=dev)
        return out

    def render_scene_tensors(self, object_datas, camera_datas, light_datas, render_normals: bool = False, render_depth: bool = False,
                             render_binary_mask: bool = False, copy_arrays: bool = True, clear: bool = True,
                             keep_layer_depth: bool = False) -> List[Dict[str, Any]]:
        """``render_scene`` without leaving the device.  One dict per group of cameras that share a resolution (``cameras``:
        their indices in ``camera_datas``): ``rgb`` [n, 3, h, w], ``normals`` (or None), ``depth`` [n, 1, h, w], ``ids``
        [n, h, w] int32 (index into ``object_datas``, -1 = background), ``mask`` [n, 1, h, w] uint8, and the ``layer_camera`` /
        ``layer_object`` index tensors of the layers that were drawn.  Depth, ids and mask are always there (the merge needs them);
        the three ``render_*`` flags are checked like the reference's."""
        if render_binary_mask:
            assert render_depth, "Binary mask can only be rendered if depth is rendered"
        objects = [_object_data(o) for o in object_datas]
        cameras = [_camera_data(c) for c in camera_datas]
        _check_supported(objects, cameras)
        for o in objects:
            assert o.label in self.store.label_to_id, f"unknown object label {o.label!r}"
        lights = self._layer_lights(objects, light_datas)
        return [self._render_group(g, objects, lights, render_normals, keep_layer_depth) for g in plan_layers(objects, cameras)]

    def render_scene(self, object_datas, camera_datas, light_datas, render_normals: bool = False, render_depth: bool = False,
                     render_binary_mask: bool = False, copy_arrays: bool = True, clear: bool = True) -> List[CameraRenderingData]:
        """``Panda3dSceneRenderer.render_scene``: one ``CameraRenderingData`` per camera, in the caller's order."""
        groups = self.render_scene_tensors(object_datas, camera_datas, light_datas, render_normals, render_depth, render_binary_mask)
        out: List[Optional[CameraRenderingData]] = [None] * len(camera_datas)
        for g in groups:
            rgb = _to_u8_hwc(g["rgb"]).cpu().numpy()
            nrm = _to_u8_hwc(g["normals"]).cpu().numpy() if render_normals else None
            dep = g["depth"].permute(0, 2, 3, 1).cpu().numpy() if render_depth else None
            msk = g["mask"].permute(0, 2, 3, 1).cpu().numpy().astype(bool) if render_binary_mask else None
            for i, ci in enumerate(g["cameras"]):
                out[ci] = CameraRenderingData(rgb[i], None if nrm is None else nrm[i], None if dep is None else dep[i],
                                              None if msk is None else msk[i])
        return out  # type: ignore[return-value]

    def scene_visibility(self, object_datas, camera_datas):
        """BOP gt-info of a scene (``MP/scripts/bop_calc_gt_info.py``): a DataFrame with one row per (camera, object) --
        ``cam_id``, ``obj_id`` (indices into the two lists), ``label``, ``px_count_all``, ``px_count_visib``, ``visib_fract``,
        ``bbox_obj`` and ``bbox_visib`` as BOP's ``(x, y, width, height)``, ``(-1, -1, -1, -1)`` for an empty box."""
        import pandas as pd

        objects = [_object_data(o) for o in object_datas]
        rows = []
        for g in self.render_scene_tensors(objects, camera_datas, [], render_depth=True, keep_layer_depth=True):
            table = ops.scene_visibility(g["layer_off"], g["layer_depth"], g["ids"]).cpu().numpy()
            for l, t in enumerate(table):
                box = lambda b: (-1, -1, -1, -1) if b[0] < 0 else (int(b[0]), int(b[1]), int(b[2] - b[0] + 1), int(b[3] - b[1] + 1))  # noqa: E731
                j = int(g["layer_object"][l])
                rows.append(dict(cam_id=int(g["layer_camera"][l]), obj_id=j, label=objects[j].label, px_count_all=int(t[0]),
                                 px_count_visib=int(t[1]), visib_fract=float(t[1]) / float(t[0]) if t[0] > 0 else 0.0,
                                 bbox_obj=box(t[2:6]), bbox_visib=box(t[6:10])))
        cols = ["cam_id", "obj_id", "label", "px_count_all", "px_count_visib", "visib_fract", "bbox_obj", "bbox_visib"]
        return pd.DataFrame(rows, columns=cols).sort_values(["cam_id", "obj_id"]).reset_index(drop=True)

    def luts(self) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._luts is None:
            self._luts = tuple(torch.as_tensor(t, device=self.device) for t in overlay_tables())
        return self._luts


def scene_visibility(renderer: SceneRenderer, object_datas, camera_datas):
    """``SceneRenderer.scene_visibility``."""
    return renderer.scene_visibility(object_datas, camera_datas)


def _device_of(device) -> torch.device:
    return torch.device("cuda" if device is None else device)


def _frame(img, dev) -> torch.Tensor:
    a = np.ascontiguousarray(img)
    assert a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8, "an image is (h, w, 3) uint8"
    return torch.as_tensor(a, device=dev)[None]


def make_contour_overlay(img: np.ndarray, render_or_scene, color: Optional[Tuple[int, int, int]] = None, dilate_iterations: int = 1,
                         per_object: bool = False, device=None) -> Dict[str, Any]:
    """``TB/visualization/utils.py:54-82``: ``{"img", "mask", "canny"}`` -- ``img`` with the outline of the rendered region
    painted in ``color`` (default green), the region as a bool mask, and the edge map (uint8, 0 / 255).  ``render_or_scene``: a
    rendered (h, w, 3) uint8 image (region = any channel > 0, the reference's ``get_mask_from_rgb``), a
    ``CameraRenderingData`` (its ``binary_mask`` when present), or one camera's ``ids`` (h, w) int32 tensor / array, which
    ``per_object=True`` also outlines between objects.  The edge is this repository's definition (``hp_scene_contour`` in the
    header), not OpenCV's Canny."""
    color = (0, 255, 0) if color is None else tuple(int(c) for c in color)
    dev = _device_of(device)
    frame = _frame(img, dev)
    src = render_or_scene
    if isinstance(src, CameraRenderingData):
        src = src.binary_mask[..., 0] if src.binary_mask is not None else src.rgb
    if isinstance(src, torch.Tensor):
        src = src.detach().cpu().numpy()
    src = np.asarray(src)
    if src.dtype == np.int32 and src.ndim == 2:
        mask_bool = src >= 0
        out, edge = ops.scene_contour(frame, ids=torch.as_tensor(np.ascontiguousarray(src), device=dev)[None], per_object=per_object,
                                      color=color, dilate_iterations=dilate_iterations)
    else:
        assert not per_object, "per_object needs an ids map"
        mask_bool = (src > 0).any(-1) if src.ndim == 3 else src.astype(bool)
        out, edge = ops.scene_contour(frame, mask=torch.as_tensor(np.ascontiguousarray(mask_bool), device=dev)[None], color=color,
                                      dilate_iterations=dilate_iterations)
    return {"img": out[0].cpu().numpy(), "mask": mask_bool, "canny": edge[0].cpu().numpy()}


def make_overlay(rgb_input: np.ndarray, rgb_rendered: np.ndarray, mask: Optional[np.ndarray] = None, device=None) -> np.ndarray:
    """``BokehPlotter.plot_overlay``'s image: ``render * 0.8 + 255 * 0.2`` where the render has a channel > 0 (or where ``mask``
    is set), ``input * 0.6 + 255 * 0.4`` elsewhere, truncated to uint8."""
    assert rgb_input.dtype == np.uint8 and rgb_rendered.dtype == np.uint8
    dev = _device_of(device)
    lut_r, lut_i = (torch.as_tensor(t) for t in overlay_tables())
    m = None if mask is None else torch.as_tensor(np.ascontiguousarray(np.asarray(mask).reshape(rgb_input.shape[:2]).astype(np.uint8)), device=dev)[None]
    return ops.scene_overlay(_frame(rgb_input, dev), _frame(rgb_rendered, dev), lut_r, lut_i, mask=m)[0].cpu().numpy()


def _ambient_white() -> List[Panda3dLightData]:
    return [Panda3dLightData(light_type="ambient", color=(1.0, 1.0, 1.0, 1))]


def render_prediction_wrt_camera(renderer: SceneRenderer, pred, camera: Optional[dict] = None, resolution=(640, 480)) -> np.ndarray:
    """``CP/visualization/singleview.py:24-38``: the predictions (``infos.label``, ``poses``) drawn in the camera's frame
    (``TWC`` = identity) under white ambient light; (h, w, 3) uint8.  ``resolution`` is (w, h) as in the reference and is
    used when the camera dict carries none (its own ``resolution`` is (h, w))."""
    pred = pred.cpu() if hasattr(pred, "cpu") else pred
    camera = dict(camera)
    camera.update(TWC=np.eye(4))
    camera.setdefault("resolution", (int(resolution[1]), int(resolution[0])))
    list_objects = []
    for n in range(len(pred)):
        row = pred.infos.iloc[n]
        list_objects.append({"name": row.label, "color": (1, 1, 1, 1), "TWO": np.asarray(pred.poses[n])})
    return renderer.render_scene(list_objects, [camera], _ambient_white())[0].rgb


def make_poses_visualization(rgb: np.ndarray, object_dataset, object_datas, camera_data, out_dir,
                             renderer: Optional[SceneRenderer] = None) -> Dict[str, Path]:
    """``TB/inference/example_inference_utils.py:123-175`` without bokeh: the objects drawn in the camera's frame under white
    ambient light, then ``mesh_overlay.png``, ``contour_overlay.png`` and ``all_results.png`` (input, contour overlay and mesh
    overlay side by side as one array) written into ``out_dir`` with PIL.  Returns the three paths."""
    from PIL import Image

    renderer = renderer if renderer is not None else SceneRenderer(object_dataset)
    cam = _camera_data(camera_data)
    cam = Panda3dCameraData(K=cam.K, resolution=cam.resolution, TWC=np.eye(4))
    rendering = renderer.render_scene(object_datas, [cam], _ambient_white())[0]
    mesh_overlay = make_overlay(rgb, rendering.rgb, device=renderer.device)
    contour_overlay = make_contour_overlay(rgb, rendering.rgb, dilate_iterations=1, color=(0, 255, 0), device=renderer.device)["img"]
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    images = {"mesh_overlay.png": mesh_overlay, "contour_overlay.png": contour_overlay,
              "all_results.png": np.concatenate([np.asarray(rgb, np.uint8), contour_overlay, mesh_overlay], axis=1)}
    paths = {}
    for name, im in images.items():
        paths[name] = out_dir / name
        Image.fromarray(im).save(paths[name])
    return paths


def scene_from_predictions(predictions, resolution: Union[Resolution, Sequence[Resolution]], view_group: Optional[int] = None):
    """``MultiviewScenePredictor.predict_scene_state``'s ``scene/objects`` (``infos.label``, ``TWO``) and ``scene/cameras``
    (``TWC``, ``K``) as the two lists ``render_scene`` takes.  ``resolution``: (h, w) of every camera, or one per camera (the
    predictions do not carry it).  Each view group is a world of its own: with more than one, name the ``view_group``."""
    objs, cams = predictions["scene/objects"], predictions["scene/cameras"]

    def rows(x):
        if "view_group" not in x.infos.columns:
            return list(range(len(x.infos)))
        vg = x.infos["view_group"].values
        if view_group is None:
            assert len(np.unique(vg)) <= 1, f"the predictions hold view groups {sorted(set(vg.tolist()))}: pass view_group"
            return list(range(len(vg)))
        return [i for i, v in enumerate(vg) if v == view_group]

    orows, crows = rows(objs), rows(cams)
    per_camera = len(resolution) > 0 and not np.isscalar(resolution[0])
    if per_camera:
        assert len(resolution) == len(crows), "one resolution per camera"
    TWO, TWC, K = (torch.as_tensor(t).detach().cpu().numpy() for t in (objs.TWO, cams.TWC, cams.K))
    object_datas = [Panda3dObjectData(label=str(objs.infos["label"].values[i]), TWO=TWO[i]) for i in orows]
    camera_datas = [Panda3dCameraData(K=K[i].astype(np.float64), resolution=tuple(resolution[n]) if per_camera else tuple(resolution), TWC=TWC[i])
                    for n, i in enumerate(crows)]
    return object_datas, camera_datas
