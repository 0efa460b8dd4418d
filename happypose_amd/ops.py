"""Thin torch-tensor front-ends of the C ABI (one function per entry point).

torch is used for device memory and streams only; every computation below
happens in the HIP library.  Each wrapper validates what the reference asserts
(shapes, dtypes) and enqueues on the current torch stream.
"""

from __future__ import annotations

import ctypes as C
import functools
import math
import weakref
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _ffi
from ._ffi import Strides, check, lib, ptr, stream_ptr
from .mesh_store import MeshDataBase, PackedMeshes, RigidObjectDataset, sample_point_ids

DEPTH_NORM = {None: 0, "none": 0, "tCR_scale": 1, "tCR_scale_clamp_center": 2, "tCR_center_clamp": 3}
MULTIVIEW = {"TCO": (0, 1), "1view_TCO": (0, 1), "TCO+front_1view": (1, 2),
             "TCO+front_3views": (3, 4), "TCO+front_5views": (5, 6)}
ARCH = {"vanilla_resnet34": 0, "resnet34": 1, "resnet18": 2, "efficientnet-b3": 3, "resnet50-fpn": 4}
N_FEATURES = {"vanilla_resnet34": 512, "resnet34": 512, "resnet18": 512, "efficientnet-b3": 1536, "resnet50-fpn": 256}


_GRAPH_EPOCH = 0


def graph_epoch() -> int:
    """Bumped whenever something changes WHICH kernels a forward launches (conv algorithm, profiling events, the
    non-finite guard switching a network to its exact kernels): captured hipGraphs of an older epoch are stale
    (``happypose_amd.graphs``)."""
    return _GRAPH_EPOCH


def scratch_launches() -> int:
    """``hp_scratch_launches``: launches so far of kernels that use scratch (spilled tile variants).  A captured hipGraph with
    such a launch replays wrongly on this runtime: a predictor whose eager call moves this count stays on eager launches."""
    return int(lib().hp_scratch_launches())


def bump_graph_epoch() -> None:
    global _GRAPH_EPOCH
    _GRAPH_EPOCH += 1


def _stream_capturing() -> bool:
    """Is the current stream capturing a graph?  (False before the GPU runtime was initialised: nothing can capture then.)"""
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


def _i32(t, device) -> torch.Tensor:
    return torch.as_tensor(t).to(device=device, dtype=torch.int32).contiguous()


def _check_ids(ids, n: int, what: str) -> None:
    """Index tensors against the table they index.  Ids that still live on the host (numpy arrays, CPU tensors:
    what the estimators build from ``infos``) are checked here for free and raise like the reference's indexing;
    ids already on the device cannot be read without a synchronisation -- the kernels receive the table sizes and
    answer an out-of-range id with NaN poses / zero crops instead of touching memory outside the table."""
    if ids is None:
        return
    t = torch.as_tensor(ids)
    if t.device.type == "cpu" and t.numel():
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= n:
            raise IndexError(f"{what}: ids in [{lo}, {hi}] index a table of {n} rows")


def _assert_ids(ids, n: int, what: str) -> None:
    """The evaluation and detection kernels (``hp_vsd``, ``hp_det_iou``, the detector losses) REQUIRE ids inside their tables: ids that
    still live on the host are checked here, before any launch.  An ``AssertionError``, unlike ``_check_ids``."""
    t = torch.as_tensor(ids)
    if t.device.type == "cpu" and t.numel():
        lo, hi = int(t.min()), int(t.max())
        assert 0 <= lo and hi < n, f"{what}: ids in [{lo}, {hi}] index a table of {n}"


class MeshStore:
    """Device-resident object set: geometry/textures for the rasteriser and the padded
    mesh-point table for the projection kernels (``hp_mesh_store``)."""

    def __init__(self, object_ds: RigidObjectDataset, device="cuda", backface_culling: Optional[bool] = None):
        """``backface_culling``: ``False`` renders this object set two-sided everywhere, as the reference does -- the opt-out for
        sets that may hold self-intersecting closed meshes (the per-component culling decision assumes they do not:
        ``hp_mesh_store_set_backface_culling`` in the header); ``None`` = the library default (on)."""
        self.device = torch.device(device)
        self.object_ds = object_ds
        self.packed = PackedMeshes(object_ds)
        self.mesh_db = MeshDataBase.from_object_ds(object_ds).batched()
        self.labels = list(self.packed.labels)
        self.label_to_id = dict(self.packed.label_to_id)
        pts = np.ascontiguousarray(self.mesh_db.points, dtype=np.float32)
        self.n_pad = pts.shape[1]
        p = self.packed
        with torch.cuda.device(self.device):
            self._h = lib().hp_mesh_store_create(
                _np_ptr(p.verts), _np_ptr(p.normals), _np_ptr(p.uvs), _np_ptr(p.colors), len(p.verts),
                _np_ptr(p.faces), len(p.faces), _np_ptr(p.tex), p.tex.size, _np_ptr(p.obj), len(p.obj),
                _np_ptr(pts), self.n_pad)
        if not self._h:
            raise _ffi.HipLibraryError("hp_mesh_store_create: " + lib().hp_last_error().decode())
        self._point_ids: Dict[int, torch.Tensor] = {}
        self._ids_cache: Dict[tuple, torch.Tensor] = {}
        self.radius = torch.as_tensor(p.radius, device=self.device)
        self._followers: List["weakref.ReferenceType[MeshStore]"] = []  # the lane stores cloned from this one (clone_for_lane)
        if backface_culling is not None:
            self.set_backface_culling(bool(backface_culling))

    def clone_for_lane(self) -> "MeshStore":
        """A second store on the same object set (a lane's own rasteriser scratch) that FOLLOWS this one's render state: the
        conventions record and the culling switch are copied now, and every later ``set_raster_conventions`` /
        ``set_backface_culling`` on this store reaches the clone too -- all lanes of a predictor render identically whichever
        lane runs a chunk."""
        other = MeshStore(self.object_ds, self.device)
        other.set_raster_conventions(self.get_raster_conventions())
        other.set_backface_culling(self.get_backface_culling())
        self._followers.append(weakref.ref(other))
        return other

    def _live_followers(self) -> List["MeshStore"]:
        live = [(r, r()) for r in self._followers]
        self._followers = [r for r, o in live if o is not None]
        return [o for _, o in live if o is not None]

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().hp_mesh_store_destroy(C.c_void_p(h))
            except Exception:
                pass

    @property
    def handle(self):
        return C.c_void_p(self._h)

    def ids_of(self, labels: Sequence[str]) -> torch.Tensor:
        """Object ids of ``labels`` on the device.  The last few label lists are remembered: a refiner is called frame after frame
        with the same table, and the host-to-device copy of the ids sits in front of a call's first launch.  The tensor is SHARED
        between the calls that ask for the same labels: read-only for the callers (they slice it and hand it to kernels)."""
        key = tuple(labels)
        hit = self._ids_cache.get(key)
        if hit is None:
            if len(self._ids_cache) >= 16:
                self._ids_cache.pop(next(iter(self._ids_cache)))
            hit = self._ids_cache[key] = torch.as_tensor([self.label_to_id[l] for l in labels], dtype=torch.int32, device=self.device)
        return hit

    def reserve_raster(self, n_views: int, resolution: Tuple[int, int] = (240, 320), msaa: bool = False) -> None:
        """Size the rasteriser scratch for ``n_views`` views per call once (``hp_mesh_store_reserve_raster``): later
        calls of up to that size never reallocate it, so captured hipGraphs keep valid pointers."""
        with torch.cuda.device(self.device):
            check(lib().hp_mesh_store_reserve_raster(self.handle, int(n_views), resolution[0], resolution[1], 32 if msaa else 0),
                  "hp_mesh_store_reserve_raster")

    def scratch_generation(self) -> int:
        """Number of times the rasteriser scratch was reallocated (``hp_mesh_store_scratch_generation``): graphs
        captured under an older generation hold freed pointers."""
        return int(lib().hp_mesh_store_scratch_generation(self.handle))

    def set_raster_conventions(self, conv: Optional[Dict] = None) -> None:
        """``hp_mesh_store_set_raster_conventions``: the three renderer conventions nobody can pin without Panda3D --
        multisample positions, the anisotropic filter's probe-count / level-of-detail rule, the axis / sign map of the eye-normal
        code (``TB/renderer/panda3d_scene_renderer.py:68-71,221-230``, ``TB/renderer/utils.py:63-79``) -- of THIS store's renders
        (two stores in one process may differ).  ``conv``: ``None`` = defaults, or a dict overriding any of
        :data:`RASTER_CONVENTION_DEFAULTS`.  Read at launch time; captured graphs are dropped (``bump_graph_epoch``).
        ``tools/calibrate_renderer.py`` fits the record to Panda3D renders."""
        if conv is None:
            check(lib().hp_mesh_store_set_raster_conventions(self.handle, None), "hp_mesh_store_set_raster_conventions")
        else:
            d = dict(RASTER_CONVENTION_DEFAULTS)
            unknown = set(conv) - set(d)
            if unknown:
                raise KeyError(f"unknown raster convention(s): {sorted(unknown)}")
            d.update(conv)
            c = RasterConventions((C.c_float * 4)(*d["msaa_x"]), (C.c_float * 4)(*d["msaa_y"]), int(d["aniso_max"]), int(d["aniso_round"]),
                                  int(d["lod_from"]), float(d["lod_bias"]), float(d["aniso_ratio_bias"]), (C.c_int * 3)(*d["normal_axis"]),
                                  (C.c_float * 3)(*d["normal_sign"]))
            check(lib().hp_mesh_store_set_raster_conventions(self.handle, C.byref(c)), "hp_mesh_store_set_raster_conventions")
        for f in self._live_followers():
            f.set_raster_conventions(conv)
        bump_graph_epoch()

    def get_raster_conventions(self) -> Dict:
        c = RasterConventions()
        check(lib().hp_mesh_store_get_raster_conventions(self.handle, C.byref(c)), "hp_mesh_store_get_raster_conventions")
        return dict(msaa_x=tuple(c.msaa_x), msaa_y=tuple(c.msaa_y), aniso_max=c.aniso_max, aniso_round=c.aniso_round, lod_from=c.lod_from,
                    lod_bias=c.lod_bias, aniso_ratio_bias=c.aniso_ratio_bias, normal_axis=tuple(c.normal_axis), normal_sign=tuple(c.normal_sign))

    def set_backface_culling(self, on: bool = True) -> bool:
        """``hp_mesh_store_set_backface_culling``: drop triangles whose inward side is turned to the camera when they belong to a
        closed, consistently oriented connected component of the mesh seen from outside (they can never be seen; the renders stay
        two-sided like the reference's for everything else).  Per store; returns the previous setting.  Default on;
        ``HP_RASTER_NO_CULL=1`` creates stores with it off."""
        prev = bool(lib().hp_mesh_store_set_backface_culling(self.handle, 1 if on else 0))
        for f in self._live_followers():
            f.set_backface_culling(on)
        bump_graph_epoch()
        return prev

    def get_backface_culling(self) -> bool:
        """``hp_mesh_store_get_backface_culling``: the current setting."""
        return bool(lib().hp_mesh_store_get_backface_culling(self.handle))

    def point_ids(self, n_points: int) -> torch.Tensor:
        """ids of ``sample_points(n, deterministic=True)`` (TB/lib3d/mesh_ops.py:74-84)."""
        if n_points not in self._point_ids:
            ids = sample_point_ids(self.n_pad, n_points).astype(np.int32)
            self._point_ids[n_points] = torch.as_tensor(ids, device=self.device)
        return self._point_ids[n_points]


def nchw_strides(c: int, h: int, w: int) -> Strides:
    return Strides(c * h * w, 0, h * w, w, 1)


class RasterConventions(C.Structure):
    """``hp_raster_conventions`` (include/happypose_amd.h)."""
    _fields_ = [("msaa_x", C.c_float * 4), ("msaa_y", C.c_float * 4), ("aniso_max", C.c_int), ("aniso_round", C.c_int),
                ("lod_from", C.c_int), ("lod_bias", C.c_float), ("aniso_ratio_bias", C.c_float), ("normal_axis", C.c_int * 3), ("normal_sign", C.c_float * 3)]


RASTER_CONVENTION_DEFAULTS = dict(msaa_x=(0.375, 0.875, 0.125, 0.625), msaa_y=(0.125, 0.375, 0.625, 0.875), aniso_max=16,
                                  aniso_round=0, lod_from=0, lod_bias=0.0, aniso_ratio_bias=0.0, normal_axis=(0, 1, 2), normal_sign=(1.0, -1.0, -1.0))


def rasterize(store: MeshStore, obj_ids: torch.Tensor, TCO: torch.Tensor, K: torch.Tensor,
              resolution: Tuple[int, int], render_normals=False, render_depth=False,
              render_binary_mask=False, ambient: Optional[torch.Tensor] = None,
              light_pos: Optional[torch.Tensor] = None, light_col: Optional[torch.Tensor] = None,
              quant8: bool = True, msaa: bool = False, aniso: bool = False, render_rgb: bool = True):
    """NCHW outputs shaped like ``BatchRenderOutput`` (TB/renderer/types.py:45-56; ``render_rgb=False``: no colour buffer,
    ``rgbs`` is None -- the depth-only launches of a C caller).  ``msaa``: 4x multisampled colour /
    normal buffers (``HP_RASTER_MSAA4``), ``aniso``: mip-mapped trilinear + anisotropic-16 texture filtering
    (``HP_RASTER_TEX_ANISO``) -- the reference renderer's framebuffer / texture state."""
    dev = store.device
    n = TCO.shape[0]
    assert TCO.shape == (n, 4, 4) and K.shape == (n, 3, 3)
    assert obj_ids.shape == (n,)
    if render_binary_mask:
        assert render_depth, "Binary mask can only be rendered if depth is rendered"
    h, w = resolution
    TCO = _f32(TCO, dev)
    K = _f32(K, dev)
    obj_ids = _i32(obj_ids, dev)
    rgb = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev) if render_rgb else None
    nrm = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev) if render_normals else None
    dep = torch.empty((n, 1, h, w), dtype=torch.float32, device=dev) if render_depth else None
    msk = torch.empty((n, 1, h, w), dtype=torch.uint8, device=dev) if render_binary_mask else None
    n_lights = 0
    if light_pos is not None:
        light_pos, light_col = _f32(light_pos, dev), _f32(light_col, dev)
        n_lights = light_pos.shape[1]
    if ambient is not None:
        ambient = _f32(ambient, dev)
    cs, ds = nchw_strides(3, h, w), nchw_strides(1, h, w)
    with torch.cuda.device(dev):
        check(lib().hp_rasterize(store.handle, n, 1, ptr(obj_ids), ptr(TCO), ptr(K), ptr(ambient), n_lights,
                                 ptr(light_pos), ptr(light_col), h, w, (8 if quant8 else 0) | (32 if msaa else 0) | (64 if aniso else 0), ptr(rgb), ptr(nrm),
                                 C.byref(cs), ptr(dep), C.byref(ds), ptr(msk), None, 0, stream_ptr(dev)),
              "hp_rasterize")
    return rgb, nrm, dep, (msk.bool() if msk is not None else None)


def render_inputs(store: MeshStore, x: torch.Tensor, obj_ids: torch.Tensor, TCV_O: torch.Tensor, KV: torch.Tensor,
                  render_normals: bool, render_depth: bool, *, images: Optional[torch.Tensor] = None,
                  boxes: Optional[torch.Tensor] = None, im_ids: Optional[torch.Tensor] = None, n_img_channels: int = 0,
                  depth_norm_z: Optional[torch.Tensor] = None, depth_norm_mode: int = 0, chan0: Optional[int] = None,
                  layout=None, ambient: Optional[torch.Tensor] = None, light_pos: Optional[torch.Tensor] = None,
                  light_col: Optional[torch.Tensor] = None, msaa: bool = False, aniso: bool = False,
                  sampling_ratio: int = 4) -> None:
    """``hp_render_inputs``: the network input ``x [b,h,w,c_rec]`` (fp32 or fp16) of one iteration in ONE pass -- ``V``
    rendered views per hypothesis (channels rgb, normals, depth in the reference's order,
    ``MP/models/pose_rigid.py:437-453``) and, when ``images`` is given, the observed crop (``crop_images`` =
    torchvision ``roi_align`` of frame ``im_ids[i]`` over ``boxes[i]``, ``TB/lib3d/cropping.py:155-197``, with the RGB-D
    validity rule and the depth normalisation of ``normalize_images``).  Default layout = the reference's
    ``cat((images_crop, renders))``: crop channels ``[0, n_img_channels)`` (written by view 0's workgroups), view ``v`` at
    ``chan0 + v * C_r`` (``chan0`` defaults to ``n_img_channels``).  ``layout`` = ``(view_c0, crop_c0, crop_src0,
    crop_n)`` lists per view overrides it (permuted inputs).  Every pixel record is written once."""
    dev = store.device
    b, h, w, cp = x.shape
    V = TCV_O.shape[1]
    assert TCV_O.shape == (b, V, 4, 4) and KV.shape == (b, V, 3, 3) and 1 <= V <= 8
    c_r = 3 + (3 if render_normals else 0) + (1 if render_depth else 0)
    assert x.dtype in (torch.float32, torch.float16) and x.is_contiguous()
    TCV_O, KV, obj_ids = _f32(TCV_O, dev), _f32(KV, dev), _i32(obj_ids, dev)
    crop = images is not None
    lay = _ffi.InputLayout()
    if layout is None:
        c0 = (n_img_channels if crop else 0) if chan0 is None else chan0
        assert c0 + V * c_r <= cp
        for v in range(V):
            lay.view_c0[v] = c0 + v * c_r
        if crop:
            lay.crop_n[0], lay.crop_c0[0], lay.crop_src0[0] = n_img_channels, 0, 0
    else:
        for name, vals in zip(("view_c0", "crop_c0", "crop_src0", "crop_n"), layout):
            assert len(vals) == V
            for v, val in enumerate(vals):
                getattr(lay, name)[v] = int(val)
    Bi = Ct = H = W = 0
    if crop:
        assert images.dtype == torch.float32 and images.is_contiguous() and images.dim() == 4
        Bi, Ct, H, W = images.shape
        _check_ids(im_ids, Bi, "render_inputs: im_ids -> images")
        boxes, im_ids = _f32(boxes, dev), _i32(im_ids, dev)
        assert boxes.shape == (b, 4) and im_ids.shape == (b,)
    n_lights = 0
    if light_pos is not None:  # [b*V, L, 3] object-frame positions + colours of point lights, ambient [b*V, 3]
        light_pos, light_col = _f32(light_pos, dev), _f32(light_col, dev)
        n_lights = light_pos.shape[1]
        assert light_pos.shape == (b * V, n_lights, 3) and light_col.shape == (b * V, n_lights, 3)
    if ambient is not None:
        ambient = _f32(ambient, dev)
        assert ambient.shape == (b * V, 3)
    flags = 8 | (16 if x.dtype == torch.float16 else 0) | (32 if msaa else 0) | (64 if aniso else 0) | \
        (0x1000 if render_normals else 0) | (0x2000 if render_depth else 0)
    mode = depth_norm_mode if (render_depth or (crop and n_img_channels == 4)) else 0
    with torch.cuda.device(dev):
        check(lib().hp_render_inputs(store.handle, b, V, ptr(obj_ids), ptr(TCV_O), ptr(KV), ptr(ambient), n_lights, ptr(light_pos),
                                     ptr(light_col), h, w, flags, ptr(images) if crop else None, Bi, Ct, H, W,
                                     ptr(boxes) if crop else None, ptr(im_ids) if crop else None, sampling_ratio,
                                     ptr(depth_norm_z) if mode else None, mode, C.c_void_p(x.data_ptr()), cp, C.byref(lay),
                                     stream_ptr(dev)), "hp_render_inputs")


def rasterize_into(store: MeshStore, x: torch.Tensor, chan0: int, obj_ids: torch.Tensor,
                   TCV_O: torch.Tensor, KV: torch.Tensor, render_normals: bool, render_depth: bool,
                   depth_norm_z: Optional[torch.Tensor] = None, depth_norm_mode: int = 0,
                   ambient: Optional[torch.Tensor] = None, msaa: bool = False, aniso: bool = False,
                   light_pos: Optional[torch.Tensor] = None, light_col: Optional[torch.Tensor] = None) -> None:
    """Render ``V`` views per hypothesis straight into channel slices of the NHWC network
    input ``x [b,h,w,c_pad]``: view ``v`` occupies channels ``chan0 + v*C_r ...`` in the
    reference's order rgb, normals, depth (MP/models/pose_rigid.py:437-453).  (:func:`render_inputs` without the crop.)"""
    render_inputs(store, x, obj_ids, TCV_O, KV, render_normals, render_depth, depth_norm_z=depth_norm_z,
                  depth_norm_mode=depth_norm_mode, chan0=chan0, ambient=ambient, light_pos=light_pos, light_col=light_col,
                  msaa=msaa, aniso=aniso)


def pose_prep(store: MeshStore, TCO: torch.Tensor, K: torch.Tensor, im_ids: torch.Tensor,
              obj_ids: torch.Tensor, im_size: Tuple[int, int], crop_size: Tuple[int, int] = (240, 320),
              multiview_type: str = "TCO", normalize: bool = False, n_points: int = 2000,
              n_points_extra: int = 200, lamb: float = 1.4, remove_TCO_rendering: bool = False):
    """Returns ``dict(TCO, tCR, TCV_O [b,V,4,4], boxes_rend, boxes_crop, K_crop [b,V,3,3], K_crop_main [b,3,3])``.
    ``K_crop_main`` is the K of the observed crop (``crop_inputs``): view 0 of ``K_crop`` unless
    ``remove_TCO_rendering`` (the TCO view is then not among the ``V`` rendered views; every view carries the K of its
    own 200-point crop, ``MP/models/pose_rigid.py:598-611``)."""
    dev = store.device
    b = TCO.shape[0]
    assert TCO.shape == (b, 4, 4) and K.dim() == 3 and K.shape[1:] == (3, 3)
    mv, V = MULTIVIEW[multiview_type]
    if remove_TCO_rendering:
        assert V >= 3, "remove_TCO_rendering needs a multi-view type with at least two look-at views"
        V -= 1
    TCO, K = _f32(TCO, dev), _f32(K, dev)
    _check_ids(im_ids, K.shape[0], "pose_prep: im_ids -> K")
    _check_ids(obj_ids, len(store.labels), "pose_prep: obj_ids -> objects")
    im_ids, obj_ids = _i32(im_ids, dev), _i32(obj_ids, dev)
    assert im_ids.shape == (b,) and obj_ids.shape == (b,)
    f = dict(dtype=torch.float32, device=dev)
    out = dict(TCO=torch.empty((b, 4, 4), **f), tCR=torch.empty((b, 3), **f),
               TCV_O=torch.empty((b, V, 4, 4), **f), boxes_rend=torch.empty((b, 4), **f),
               boxes_crop=torch.empty((b, 4), **f), K_crop=torch.empty((b, V, 3, 3), **f))
    ids_main = store.point_ids(n_points)
    multi = V > 1 or remove_TCO_rendering
    ids_extra = store.point_ids(n_points_extra) if multi else None
    with torch.cuda.device(dev):
        if remove_TCO_rendering:
            out["K_crop_main"] = torch.empty((b, 3, 3), **f)
            check(lib().hp_pose_prep_views(store.handle, b, V, mv, 1, int(normalize), ptr(TCO), ptr(K), K.shape[0], ptr(im_ids),
                                           ptr(obj_ids), ptr(ids_main), n_points, ptr(ids_extra), n_points_extra, im_size[0],
                                           im_size[1], crop_size[0], crop_size[1], C.c_float(lamb), ptr(out["TCO"]),
                                           ptr(out["tCR"]), ptr(out["TCV_O"]), ptr(out["boxes_rend"]), ptr(out["boxes_crop"]),
                                           ptr(out["K_crop"]), ptr(out["K_crop_main"]), stream_ptr(dev)), "hp_pose_prep_views")
        else:
            check(lib().hp_pose_prep(store.handle, b, V, mv, int(normalize), ptr(TCO), ptr(K), K.shape[0], ptr(im_ids),
                                     ptr(obj_ids), ptr(ids_main), n_points, ptr(ids_extra),
                                     n_points_extra if multi else 0, im_size[0], im_size[1], crop_size[0],
                                     crop_size[1], C.c_float(lamb), ptr(out["TCO"]), ptr(out["tCR"]),
                                     ptr(out["TCV_O"]), ptr(out["boxes_rend"]), ptr(out["boxes_crop"]),
                                     ptr(out["K_crop"]), stream_ptr(dev)), "hp_pose_prep")
            out["K_crop_main"] = out["K_crop"][:, 0]
    return out


def crop_roi_align(images: torch.Tensor, boxes: torch.Tensor, im_ids: torch.Tensor,
                   output_size=(240, 320), sampling_ratio: int = 4, out: Optional[torch.Tensor] = None,
                   depth_norm_z: Optional[torch.Tensor] = None, depth_norm_mode: int = 0,
                   n_channels: Optional[int] = None, owns_record: bool = False) -> torch.Tensor:
    """``crop_images`` (TB/lib3d/cropping.py:155-197).  ``out=None`` -> NCHW ``[n,C,oh,ow]``;
    otherwise ``out`` is the NHWC network input ``[n,oh,ow,c_pad]`` and channels 0..C-1 are
    written."""
    dev = images.device
    Bi, Ct, H, W = images.shape
    Cc = Ct if n_channels is None else n_channels
    n = boxes.shape[0]
    oh, ow = output_size
    assert images.dtype == torch.float32 and images.is_contiguous()
    _check_ids(im_ids, Bi, "crop_roi_align: im_ids -> images")
    boxes, im_ids = _f32(boxes, dev), _i32(im_ids, dev)
    assert boxes.shape == (n, 4) and im_ids.shape == (n,)
    if out is None:
        res = torch.empty((n, Cc, oh, ow), dtype=torch.float32, device=dev)
        st = Strides(Cc * oh * ow, 0, oh * ow, ow, 1)
    else:
        res = out
        assert out.shape[:3] == (n, oh, ow) and out.shape[3] >= Cc and out.is_contiguous()
        assert out.dtype in (torch.float32, torch.float16)
        cp = out.shape[3]
        st = Strides(oh * ow * cp, 0, 1, ow * cp, cp)
    fn = lib().hp_crop_roi_align_f16 if res.dtype == torch.float16 else lib().hp_crop_roi_align
    mode = depth_norm_mode if Cc == 4 else 0
    # ``owns_record``: the caller promises that the rest of every pixel record may be zeroed (the rasteriser writes it
    # afterwards): the first 8 floats of every record are then stored as a whole 32-B sector (HP_CROP_FULL_RECORD8)
    if owns_record and out is not None and res.shape[3] % (8 if res.dtype == torch.float32 else 16) == 0 and res.data_ptr() % 32 == 0:
        mode |= 0x100
    with torch.cuda.device(dev):
        check(fn(ptr(images), Bi, Ct, Cc, H, W, ptr(boxes), ptr(im_ids), n, oh, ow,
                 sampling_ratio, ptr(res), C.byref(st),
                 ptr(depth_norm_z), mode, stream_ptr(dev)),
              "hp_crop_roi_align")
    return res


def pose_update(TCO: torch.Tensor, K_crop: torch.Tensor, pose9: torch.Tensor,
                tCR: Optional[torch.Tensor] = None) -> torch.Tensor:
    dev = TCO.device
    b = TCO.shape[0]
    assert TCO.shape == (b, 4, 4) and pose9.shape == (b, 9)
    assert K_crop.shape[0] == b and K_crop.shape[-2:] == (3, 3)
    k_stride = K_crop[0].numel()
    TCO, K_crop, pose9 = _f32(TCO, dev), _f32(K_crop, dev), _f32(pose9, dev)
    if tCR is not None:
        assert tCR.shape == (b, 3)
        tCR = _f32(tCR, dev)
    out = torch.empty_like(TCO)
    with torch.cuda.device(dev):
        check(lib().hp_pose_update(b, ptr(TCO), ptr(K_crop), k_stride, ptr(pose9), ptr(tCR), ptr(out),
                                   stream_ptr(dev)), "hp_pose_update")
    return out


def tco_init_autodepth(store: MeshStore, boxes: torch.Tensor, K: torch.Tensor, im_ids, obj_ids,
                       R: Optional[torch.Tensor] = None, box_ids=None, rot_ids=None,
                       n_points: Optional[int] = None) -> torch.Tensor:
    dev = store.device
    n = len(obj_ids)
    boxes, K = _f32(boxes, dev), _f32(K, dev)
    if R is not None:
        R = _f32(R, dev)
    assert boxes.dim() == 2 and boxes.shape[1] == 4 and K.dim() == 3 and K.shape[1:] == (3, 3)
    assert R is None or (R.dim() == 3 and R.shape[1:] == (3, 3))
    assert box_ids is not None or boxes.shape[0] == n, "one box per hypothesis unless box_ids is given"
    assert R is None or rot_ids is not None or R.shape[0] == n, "one rotation per hypothesis unless rot_ids is given"
    _check_ids(im_ids, K.shape[0], "tco_init_autodepth: im_ids -> K")
    _check_ids(obj_ids, len(store.labels), "tco_init_autodepth: obj_ids -> objects")
    _check_ids(box_ids, boxes.shape[0], "tco_init_autodepth: box_ids -> boxes")
    if R is not None:
        _check_ids(rot_ids, R.shape[0], "tco_init_autodepth: rot_ids -> R")
    im_ids, obj_ids = _i32(im_ids, dev), _i32(obj_ids, dev)
    box_ids = None if box_ids is None else _i32(box_ids, dev)
    rot_ids = None if rot_ids is None else _i32(rot_ids, dev)
    out = torch.empty((n, 4, 4), dtype=torch.float32, device=dev)
    pids = None if n_points is None else store.point_ids(n_points)
    with torch.cuda.device(dev):
        check(lib().hp_tco_init_autodepth(store.handle, n, ptr(boxes), boxes.shape[0], ptr(box_ids), ptr(K), K.shape[0],
                                          ptr(im_ids), ptr(obj_ids), ptr(R), 0 if R is None else R.shape[0],
                                          ptr(rot_ids), ptr(pids), n_points or 0,
                                          ptr(out), stream_ptr(dev)),
              "hp_tco_init_autodepth")
    return out


class Net:
    """``hp_net``: backbone + heads with BN folded, on one device."""

    profiling = False  # set_profiling(True): conv stretches are timed with HIP events (no graph capture then)
    tail_split = True  # hp_net_set_tail_split state: changes the launch plan, so it is part of a graph signature
    _exact_only = False  # last seen HP_STATUS_EXACT_ONLY (the guard's switch to the exact-fp32 kernels)
    # An fp16 plan has no exact kernels of its own: its remedy is an fp32 SIBLING -- an ``ops.Net`` of the same parameters
    # and geometry with ``precision="f32"``, forced exact -- built the first time the guard fires (``status``) or
    # ``force_exact(True)`` is called, and used for everything until ``force_exact(False)``.  It costs a second set of
    # weights and a second activation arena at ``max_batch``, which is why it is not built before it is needed.
    _sibling: Optional["Net"] = None
    _on_sibling = False
    _host_params = None  # fp16 plan: the parameters on the host, what the sibling is built from
    # fp16 plan: the head tensors replaced on the device since (set_param_device) -- ``_host_params`` is stale for them, so a
    # sibling built later is given these on top
    _device_params: Optional[Dict[str, torch.Tensor]] = None

    HEAD_PARAMS = ("pose_fc.weight", "pose_fc.bias", "views_logits_head.weight", "views_logits_head.bias", "backbone.fc.weight",
                   "backbone.fc.bias")

    def __init__(self, arch: str, n_inputs: int, state_dict: Dict[str, "np.ndarray | torch.Tensor"],
                 max_batch: int = 128, device="cuda", h: int = 240, w: int = 320, precision: str = "f32"):
        """``precision``: ``"f32"`` (the reference's arithmetic) or ``"f16"`` (fp16 weights and
        activations, fp32 accumulation: configuration C5; inputs / outputs stay fp32)."""
        self.device = torch.device(device)
        self.arch, self.n_inputs, self.h, self.w = arch, n_inputs, h, w
        self.precision = precision
        self.max_batch = max_batch
        self.n_features = N_FEATURES[arch]
        with torch.cuda.device(self.device):
            self._h = lib().hp_net_create(ARCH[arch], n_inputs, h, w)
            if not self._h:
                raise _ffi.HipLibraryError("hp_net_create: " + lib().hp_last_error().decode())
            keep = {} if precision == "f16" else None
            for name, value in state_dict.items():
                if name.endswith("num_batches_tracked"):
                    continue
                arr = value.detach().cpu().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)
                arr = np.ascontiguousarray(arr, dtype=np.float32)
                check(lib().hp_net_set_param(self.handle, name.encode(), _np_ptr(arr), arr.size),
                      f"hp_net_set_param({name})")
                if keep is not None:
                    keep[name] = arr.copy()  # the caller's tensors may change or go away before the sibling is built
            self._host_params = keep
            check(lib().hp_net_set_precision(self.handle, {"f32": 0, "f16": 1}[precision]), "hp_net_set_precision")
            check(lib().hp_net_finalize(self.handle, max_batch), "hp_net_finalize")
        self.c_pad = lib().hp_net_input_channels_padded(self.handle)
        self.c16 = lib().hp_net_input_channels_f16(self.handle) if precision == "f16" else 0  # channels of an fp16 input record
        self.pose_dim = state_dict["pose_fc.weight"].shape[0] if "pose_fc.weight" in state_dict else 0
        self.n_logits = (state_dict["views_logits_head.weight"].shape[0]
                         if "views_logits_head.weight" in state_dict else 0)
        self.flops_per_sample = lib().hp_net_flops_per_sample(self.handle)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().hp_net_destroy(C.c_void_p(h))
            except Exception:
                pass

    @property
    def handle(self):
        return C.c_void_p(self._h)

    def _exact_net(self) -> "Net":
        """The fp32 sibling of an fp16 plan, built on first use.  Building allocates (weights, an activation arena), so
        it only happens at the guard's synchronisation points -- never while a stream captures."""
        assert self.precision == "f16" and self._host_params is not None
        if self._sibling is None:
            assert not _stream_capturing(), "the fp32 sibling of an fp16 network cannot be built while a stream captures"
            sib = Net(self.arch, self.n_inputs, self._host_params, max_batch=self.max_batch, device=self.device,
                      h=self.h, w=self.w, precision="f32")
            # the repeat is the reference's arithmetic, not the split-fp16 kernels: exact from the start (set on the handle, not
            # through force_exact(): the switch-over is ONE launch-plan change and bumps the graph epoch once)
            check(lib().hp_net_force_exact(sib.handle, 1), "hp_net_force_exact")
            sib._exact_only = True
            if not self.tail_split:
                sib.set_tail_split(False)
            if self.profiling:
                check(lib().hp_net_set_profiling(sib.handle, 1), "hp_net_set_profiling")
                sib.profiling = True
            for name, t in (self._device_params or {}).items():  # heads trained since this plan was built
                sib.set_param_device(name, t)
            self._sibling = sib
        return self._sibling

    def head_param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """The head tensors this network has (:attr:`HEAD_PARAMS`), by the reference's names, with their shapes."""
        out: Dict[str, Tuple[int, ...]] = {}
        if self.arch == "vanilla_resnet34":
            out["backbone.fc.weight"], out["backbone.fc.bias"] = (512, 512), (512,)
        if self.pose_dim:
            out["pose_fc.weight"], out["pose_fc.bias"] = (self.pose_dim, self.n_features), (self.pose_dim,)
        if self.n_logits:
            out["views_logits_head.weight"], out["views_logits_head.bias"] = (self.n_logits, self.n_features), (self.n_logits,)
        return out

    def get_param_device(self, name: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``hp_net_get_param_device``: a head tensor as the network holds it now, copied on the current stream (the plan the
        fp16 front was built as; its sibling holds the same heads)."""
        shape = self.head_param_shapes().get(name)
        if shape is None:
            raise KeyError(f"{name!r} is not a head tensor of this network ({sorted(self.head_param_shapes())})")
        out = torch.empty(shape, dtype=torch.float32, device=self.device) if out is None else out
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == int(np.prod(shape))
        with torch.cuda.device(self.device):
            check(lib().hp_net_get_param_device(self.handle, name.encode(), ptr(out), out.numel(), stream_ptr(self.device)),
                  f"hp_net_get_param_device({name})")
        return out

    def set_param_device(self, name: str, value: torch.Tensor) -> None:
        """``hp_net_set_param_device``: replace a head tensor (:attr:`HEAD_PARAMS`) of the finalised network by a float32 tensor
        on its device, with a copy on the current stream -- no host round trip, no re-planning, captured graphs stay valid.  Any
        other name raises (conv and BN weights are folded or packed at finalise).  An fp16 plan hands the tensor to its fp32
        sibling too: at once when the sibling exists, else when the guard builds it -- ``value`` is kept (not copied) for
        that, so it must then still hold what was set (a trainer's master copy does)."""
        assert isinstance(value, torch.Tensor) and value.dtype == torch.float32 and value.is_contiguous(), \
            "set_param_device: a contiguous float32 tensor"
        with torch.cuda.device(self.device):
            check(lib().hp_net_set_param_device(self.handle, name.encode(), ptr(value), value.numel(), stream_ptr(self.device)),
                  f"hp_net_set_param_device({name})")
        if self.precision == "f16":
            if self._device_params is None:
                self._device_params = {}
            self._device_params[name] = value
            if self._sibling is not None:
                self._sibling.set_param_device(name, value)

    def _switch(self, on: bool) -> None:
        """Send every later call to the fp32 sibling (``on``) or back to the fp16 plan; a transition changes the launch
        plan, so it bumps the graph epoch."""
        assert not _stream_capturing(), "the numerical guard is consulted outside graph captures"
        if on:
            self._exact_net()
        if on != self._on_sibling:
            bump_graph_epoch()
        self._on_sibling = self._exact_only = on

    def input_spec(self) -> Tuple[torch.dtype, int]:
        """``(dtype, channels)`` of the record :meth:`new_input` makes NOW (an fp16 plan that fell back to its fp32
        sibling takes fp32 records)."""
        if self._on_sibling:
            return self._sibling.input_spec()
        return (torch.float16, self.c16) if self.precision == "f16" else (torch.float32, self.c_pad)

    def new_input(self, batch: int) -> torch.Tensor:
        """Zeroed NHWC input buffer (pad channels must stay 0): fp32 ``[batch,h,w,c_pad]``, or for an
        fp16 plan fp16 ``[batch,h,w,c16]`` -- crop and rasteriser write it directly and ``forward``
        skips the conversion pass (``hp_net_forward_f16in``)."""
        if self._on_sibling:
            return self._sibling.new_input(batch)
        if self.precision == "f16":
            assert self.c16 > 0, lib().hp_last_error().decode()
            return torch.zeros((batch, self.h, self.w, self.c16), dtype=torch.float16, device=self.device)
        return torch.zeros((batch, self.h, self.w, self.c_pad), dtype=torch.float32, device=self.device)

    def forward(self, x: torch.Tensor, want_pose=True, want_logits=False, want_features=False, pooled_out: Optional[torch.Tensor] = None):
        """``pooled_out [b, 512]`` (networks with the fc, ``arch == "vanilla_resnet34"``): also receives the fc's input, the
        spatial mean (``hp_net_set_pooled_out`` around this call)."""
        if self._on_sibling:
            assert x.dtype == torch.float32, "this fp16 network runs on its fp32 sibling now: take the input from new_input()"
            return self._sibling.forward(x, want_pose=want_pose, want_logits=want_logits, want_features=want_features, pooled_out=pooled_out)
        if pooled_out is not None:
            assert pooled_out.shape == (x.shape[0], 512) and pooled_out.dtype == torch.float32 and pooled_out.is_contiguous()
            check(lib().hp_net_set_pooled_out(self.handle, ptr(pooled_out)), "hp_net_set_pooled_out")
            try:
                return self.forward(x, want_pose=want_pose, want_logits=want_logits, want_features=want_features)
            finally:
                check(lib().hp_net_set_pooled_out(self.handle, None), "hp_net_set_pooled_out")
        b = x.shape[0]
        f = dict(dtype=torch.float32, device=self.device)
        if x.dtype == torch.float16:
            assert self.precision == "f16" and x.is_contiguous() and x.shape[:3] == (b, self.h, self.w)
            assert x.shape[3] == self.c16
            pose = torch.empty((b, self.pose_dim), **f) if (want_pose and self.pose_dim) else None
            logits = torch.empty((b, self.n_logits), **f) if (want_logits and self.n_logits) else None
            feats = torch.empty((b, self.n_features), **f) if want_features else None
            with torch.cuda.device(self.device):
                check(lib().hp_net_forward_f16in(self.handle, C.c_void_p(x.data_ptr()), b, ptr(pose), ptr(logits), ptr(feats),
                                                 stream_ptr(self.device)), "hp_net_forward_f16in")
            return pose, logits, feats
        assert x.shape == (b, self.h, self.w, self.c_pad) and x.is_contiguous() and x.dtype == torch.float32
        pose = torch.empty((b, self.pose_dim), **f) if (want_pose and self.pose_dim) else None
        logits = torch.empty((b, self.n_logits), **f) if (want_logits and self.n_logits) else None
        feats = torch.empty((b, self.n_features), **f) if want_features else None
        with torch.cuda.device(self.device):
            check(lib().hp_net_forward(self.handle, ptr(x), b, ptr(pose), ptr(logits), ptr(feats),
                                       stream_ptr(self.device)), "hp_net_forward")
        return pose, logits, feats

    def feature_maps(self, batch: int):
        """Feature-pyramid networks (``resnet50-fpn``): the output maps of the last ``forward`` as NHWC tensors
        ``[batch, h, w, c]`` (``hp_net_copy_feature_map``)."""
        outs = []
        for i in range(lib().hp_net_n_feature_maps(self.handle)):
            h, w, c = C.c_int(0), C.c_int(0), C.c_int(0)
            check(lib().hp_net_feature_map(self.handle, i, None, C.byref(h), C.byref(w), C.byref(c)), "hp_net_feature_map")
            t = torch.empty((batch, h.value, w.value, c.value), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                check(lib().hp_net_copy_feature_map(self.handle, i, batch, ptr(t), stream_ptr(self.device)), "hp_net_copy_feature_map")
            outs.append(t)
        return outs

    def op_list(self):
        """The ops of the network in execution order (``hp_net_op_info``), one dict each: ``kind`` (a name of
        :data:`OP_KINDS`), ``name`` (weight name of a conv), geometry, arena slots, ``elem_bytes``, and for the LAST forward
        ``path`` (a name of :data:`OP_PATHS`) and ``materialised``."""
        if self._on_sibling:
            return self._sibling.op_list()
        out = []
        n = lib().hp_net_n_ops(self.handle)
        if n < 0:
            check(n, "hp_net_n_ops")
        for i in range(n):
            info = _ffi.OpInfo()
            check(lib().hp_net_op_info(self.handle, i, C.byref(info)), "hp_net_op_info")
            d = {n: getattr(info, n) for n, _ in _ffi.OpInfo._fields_}
            d.update(index=i, kind=OP_KINDS[info.kind], path=OP_PATHS[info.path], name=info.name.decode(),
                     materialised=bool(info.materialised), prologue=bool(info.prologue))
            out.append(d)
        return out

    def set_taps(self, op_indices, batch: int):
        """Layer-level tests (``hp_net_set_taps``): every later forward of up to ``batch`` samples leaves the output map of the
        ops ``op_indices`` in the returned tensors ``{index: [batch, Ho, Wo, Cout]}`` (fp32, or fp16 on an fp16 plan).  An op
        that a fused launch never writes is not copied: see ``materialised`` of :meth:`op_list` after the forward.
        ``set_taps([], 0)`` clears them.  For tests: the library keeps the raw addresses, and only this object's reference keeps
        the tensors alive -- clear the taps before dropping the returned dict's tensors or reusing the network elsewhere."""
        if self._on_sibling:
            return self._sibling.set_taps(op_indices, batch)
        ops_ = self.op_list()
        dtype = torch.float16 if self.precision == "f16" else torch.float32
        self._taps = {i: torch.zeros((batch, ops_[i]["Ho"], ops_[i]["Wo"], ops_[i]["Cout"]), dtype=dtype, device=self.device)
                      for i in op_indices}
        idx = (C.c_int * len(self._taps))(*self._taps)
        dst = (C.c_void_p * len(self._taps))(*[t.data_ptr() for t in self._taps.values()])
        check(lib().hp_net_set_taps(self.handle, len(self._taps), idx, dst), "hp_net_set_taps")
        return self._taps

    def set_profiling(self, on: bool):
        if self._sibling is not None:  # both plans follow, so that the switch is the same on either side of a fallback
            check(lib().hp_net_set_profiling(self._sibling.handle, int(on)), "hp_net_set_profiling")
            self._sibling.profiling = bool(on)
        check(lib().hp_net_set_profiling(self.handle, int(on)), "hp_net_set_profiling")
        self.profiling = bool(on)
        bump_graph_epoch()  # event records change the launch sequence a captured graph holds

    def set_conv_algo(self, name: Optional[str] = None):
        """Kernel families THIS network may use (``hp_net_set_conv_algo``; names of :data:`CONV_ALGOS`);
        ``None`` returns it to ``auto``."""
        check(lib().hp_net_set_conv_algo(self.handle, -1 if name is None else CONV_ALGOS[name]), "hp_net_set_conv_algo")
        bump_graph_epoch()

    def set_tail_split(self, on: bool):
        """K-slicing of the tail tiles of this network's conv launches (``hp_net_set_tail_split``): off while a
        second lane shares the GPU."""
        if self._sibling is not None:
            self._sibling.set_tail_split(on)
        check(lib().hp_net_set_tail_split(self.handle, int(on)), "hp_net_set_tail_split")
        self.tail_split = bool(on)

    def set_act_scale(self, on: bool):
        """Dynamic power-of-two activation scale of the split-fp16 kernels (``hp_net_set_act_scale``; default on)."""
        check(lib().hp_net_set_act_scale(self.handle, int(on)), "hp_net_set_act_scale")
        bump_graph_epoch()  # launch arguments change

    def status(self, stream=None) -> int:
        """``hp_net_status``: waits for ``stream`` (default: the current one) and returns the guard flags --
        bit 0 (:data:`STATUS_NONFINITE`): a forward since the last call produced inf / NaN in a split-fp16
        layer (an activation beyond the fp16 range), its outputs are invalid; bit 1 (:data:`STATUS_EXACT_ONLY`):
        the network now runs the exact-fp32 kernels only, so re-running the same inputs is valid.

        An fp16 plan reports bit 0 when a value one of its layers stored was inf / NaN before the activation or
        overflowed the half it was rounded to.  It then builds its fp32 sibling, sends every later call there and
        returns ``STATUS_NONFINITE | STATUS_EXACT_ONLY`` for this call and ``STATUS_EXACT_ONLY`` afterwards -- the
        same contract, sticky until ``force_exact(False)``.  Not to be called while a stream captures."""
        if self._on_sibling:
            return self._sibling.status(stream) | STATUS_EXACT_ONLY
        flags = C.c_int(0)
        sp = stream_ptr(self.device) if stream is None else C.c_void_p(stream.cuda_stream)
        with torch.cuda.device(self.device):
            check(lib().hp_net_status(self.handle, sp, C.byref(flags)), "hp_net_status")
        if self.precision == "f16":  # the library never latches an fp16 network: the fallback is this object's
            if flags.value & STATUS_NONFINITE:
                self._switch(True)
                return flags.value | STATUS_EXACT_ONLY
            return flags.value
        exact = bool(flags.value & STATUS_EXACT_ONLY)
        if (flags.value & STATUS_NONFINITE) or exact != self._exact_only:
            # the network switched kernels (or just poisoned a forward): captured graphs still hold the old launches.
            # Only the TRANSITION bumps: the sticky EXACT_ONLY bit alone would otherwise drop every graph cache of the
            # process after every stage of the estimators
            bump_graph_epoch()
        self._exact_only = exact
        return flags.value

    def force_exact(self, on: bool = True) -> None:
        """``hp_net_force_exact``: put the network on (or take it off) the exact-fp32 kernels the guard switches to.
        An fp16 plan goes to (returns from) its fp32 sibling instead; input records change dtype with it
        (:meth:`input_spec`).  Not to be called while a stream captures."""
        if self.precision == "f16":
            self._switch(bool(on))
            return
        check(lib().hp_net_force_exact(self.handle, int(bool(on))), "hp_net_force_exact")
        if bool(on) != self._exact_only:
            bump_graph_epoch()
        self._exact_only = bool(on)

    def profile_collect(self):
        """``(conv_ms, n_launches, conv_flops, mfma_flops)`` of the conv launches recorded since
        the last call (HIP events on the launch stream; waits for them): algorithmic FLOPs of the
        direct convolutions and FLOPs the matrix cores executed (Winograd layers execute 2.25x
        fewer, padded tiles more)."""
        if self._on_sibling:
            return self._sibling.profile_collect()
        ms, n, fl, mfl = C.c_double(0), C.c_int64(0), C.c_double(0), C.c_double(0)
        check(lib().hp_net_profile_collect(self.handle, C.byref(ms), C.byref(n), C.byref(fl), C.byref(mfl)),
              "hp_net_profile_collect")
        return ms.value, n.value, fl.value, mfl.value

    def profile_intervals(self):
        """``[(t0_ms, t1_ms), ...]`` of the timed conv stretches pending for this network, relative to
        :func:`profile_mark_reference` (call before :meth:`profile_collect`)."""
        if self._on_sibling:
            return self._sibling.profile_intervals()
        n = lib().hp_net_profile_intervals(self.handle, None, None, 0)
        if n < 0:
            check(n, "hp_net_profile_intervals")
        a, b = (C.c_double * n)(), (C.c_double * n)()
        got = lib().hp_net_profile_intervals(self.handle, a, b, n)
        if got < 0:
            check(got, "hp_net_profile_intervals")
        return list(zip(list(a), list(b)))


class GraphNet(Net):
    """``HP_ARCH_CUSTOM``: a feed-forward graph of convolutions described layer by layer (the detector's RoI heads).
    ``layers``: dicts ``weight, bias, cin, cout, k, stride, pad, relu, H, W, src, dst, res`` in execution order
    (``src = -1`` = the network input, arena slots 0..31); ``outputs``: ``(slot, H, W, C)`` read back by
    :meth:`Net.feature_maps` (``C`` rounded up to 4).  A layer's ``kind`` (default ``"conv"``) may also name the ops of an
    EfficientNet MBConv block (block-level tests; the launches are the ones the EfficientNet plan picks):
    ``"dw"``: ``weight, bn, C, k, stride, pad`` (top / left), ``H, W, Ho, Wo, src, dst`` (``hp_net_add_dwconv``);
    ``"se"``: ``prefix, C, Cse, H, W, src`` (``hp_net_add_se``); a conv layer with ``relu=2`` is activated by swish, one with
    ``gated=True`` takes the gate of the ``"se"`` layer before it on its input (the 1x1 projection)."""

    def __init__(self, c_in: int, h: int, w: int, layers, outputs, state_dict, max_batch: int, device="cuda"):
        self.device = torch.device(device)
        self.arch, self.n_inputs, self.h, self.w, self.precision = "custom", c_in, h, w, "f32"
        self.n_features = self.pose_dim = self.n_logits = 0
        with torch.cuda.device(self.device):
            self._h = lib().hp_net_create(5, c_in, h, w)
            if not self._h:
                raise _ffi.HipLibraryError("hp_net_create: " + lib().hp_last_error().decode())
            for L in layers:
                kind = L.get("kind", "conv")
                if kind == "dw":
                    check(lib().hp_net_add_dwconv(self.handle, L["weight"].encode(), L["bn"].encode(), L["C"], L["k"], L.get("stride", 1),
                                                  L["pad"], L["H"], L["W"], L["Ho"], L["Wo"], L["src"], L["dst"]),
                          f"hp_net_add_dwconv({L['weight']})")
                    continue
                if kind == "se":
                    check(lib().hp_net_add_se(self.handle, L["prefix"].encode(), L["C"], L["Cse"], L["H"], L["W"], L["src"]),
                          f"hp_net_add_se({L['prefix']})")
                    continue
                assert kind == "conv", kind
                act = int(L.get("relu", False)) | (CONV_GATED if L.get("gated") else 0)
                check(lib().hp_net_add_conv(self.handle, L["weight"].encode(), (L.get("bias") or "").encode(), L["cin"], L["cout"], L["k"],
                                            L.get("stride", 1), L.get("pad", 0), act, L["H"], L["W"], L["src"],
                                            L["dst"], L.get("res", -1)), f"hp_net_add_conv({L['weight']})")
            for slot, oh, ow, oc in outputs:
                check(lib().hp_net_add_output(self.handle, slot, oh, ow, (oc + 3) // 4 * 4), "hp_net_add_output")
            for name, value in state_dict.items():
                arr = value.detach().cpu().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)
                arr = np.ascontiguousarray(arr, dtype=np.float32)
                check(lib().hp_net_set_param(self.handle, name.encode(), _np_ptr(arr), arr.size), f"hp_net_set_param({name})")
            check(lib().hp_net_finalize(self.handle, max_batch), "hp_net_finalize")
        self.c_pad = lib().hp_net_input_channels_padded(self.handle)
        self.max_batch = max_batch
        self.flops_per_sample = lib().hp_net_flops_per_sample(self.handle)

    def run(self, x: torch.Tensor):
        """``x [n,h,w,c_in]`` NHWC fp32 -> list of output maps ``[n,oh,ow,oc4]`` (chunks of ``max_batch``)."""
        n = x.shape[0]
        outs = None
        for s in range(0, n, self.max_batch):
            xb = x[s:s + self.max_batch].contiguous()
            self.forward(xb, want_pose=False)
            maps = self.feature_maps(xb.shape[0])
            outs = [[m] for m in maps] if outs is None else [o + [m] for o, m in zip(outs, maps)]
        return [torch.cat(o) for o in outs] if outs is not None else []


STATUS_NONFINITE, STATUS_EXACT_ONLY = 1, 2
OP_KINDS = ("conv", "maxpool", "head", "dw", "se", "resize")  # HP_OP_*
OP_PATHS = ("none", "split3x3", "split3x3+shortcut", "rode", "winograd", "igemm_split", "patch", "generic", "stem7_pool",  # HP_PATH_*
            "stem7_pool_f16", "stem_split_pool", "igemm_split_pool", "mbconv_front", "fused_away", "conv_f16", "maxpool",
            "maxpool_f16", "head", "dw", "se", "resize", "mixed")
CONV_GATED = 0x100  # HP_CONV_GATED


def profile_mark_reference(device) -> None:
    """Record the process-wide reference event of :meth:`Net.profile_intervals` on the current stream."""
    with torch.cuda.device(device):
        check(lib().hp_profile_mark_reference(stream_ptr(device)), "hp_profile_mark_reference")


def probe_mfma_rate(device, random_data: bool = True):
    """``hp_probe_mfma_rate``: ``(TFLOP/s, shader MHz)`` the fp16 matrix pipe sustains on zero / random operands."""
    tf, mhz = C.c_double(0), C.c_double(0)
    with torch.cuda.device(device):
        check(lib().hp_probe_mfma_rate(int(random_data), C.byref(tf), C.byref(mhz), stream_ptr(device)), "hp_probe_mfma_rate")
    return tf.value, mhz.value


CONV_ALGOS = {"auto": 0, "direct": 1, "igemm": 2, "winograd-1wave": 3, "winograd": 4, "split": 5}


def select_conv_algo(name: str = "auto") -> None:
    """The kernel family of the SINGLE-LAYER entry point ``conv2d_nhwc`` (``hp_conv_select_algo``; parity tests and
    ``tools/conv_fuzz.py`` walk the families with it).  Networks never read it -- a network's choice is
    :meth:`Net.set_conv_algo`, default ``auto``.  ``auto`` = the split-fp16 kernels where they apply, else Winograd
    F(2x2,3x3), else the patch-staged direct kernel, else the generic implicit GEMM; ``winograd`` = exact-fp32 arithmetic
    only (``winograd-1wave``: the one-wave-per-SIMD schedule of that kernel); ``direct`` = no Winograd; ``igemm`` = the
    generic implicit-GEMM kernel only; ``split`` = the split-fp16 kernels."""
    check(lib().hp_conv_select_algo(CONV_ALGOS[name]), "hp_conv_select_algo")
    bump_graph_epoch()


def conv2d_nhwc(x, w_packed, stride, pad, bias=None, residual=None, pre_scale=None, pre_shift=None, relu=False):
    """Single conv layer (parity tests).  ``x [n,h,w,cin]``, ``w_packed [cout,kh,kw,cin]``.
    ``relu``: False/0 none, True/1 ReLU, 2 swish.  ``pre_scale [cin]`` + ``pre_shift [cin]`` = the
    BN+ReLU prologue; ``pre_scale [n,cin]`` alone = a squeeze-excitation gate on the input."""
    dev = x.device
    n, h, w, cin = x.shape
    cout, kh, kw, cin2 = w_packed.shape
    assert cin == cin2
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    y = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_conv2d_nhwc(ptr(x), n, h, w, cin, ptr(w_packed), cout, kh, kw, stride, pad, ptr(bias),
                                   ptr(residual), ptr(pre_scale), ptr(pre_shift), int(relu), ptr(y),
                                   stream_ptr(dev)), "hp_conv2d_nhwc")
    return y


def conv2d_nhwc_f16(x, w_packed, stride, pad, bias=None, residual=None, pre_scale=None, pre_shift=None, relu=False):
    """Single conv layer of the fp16 kernel (parity tests): ``x [n,h,w,cin]`` and ``w_packed
    [cout,kh,kw,cin]`` (and residual / pre_scale / pre_shift) fp16, bias fp32; returns fp16."""
    dev = x.device
    n, h, w, cin = x.shape
    cout, kh, kw, cin2 = w_packed.shape
    assert cin == cin2 and x.dtype == torch.float16 and w_packed.dtype == torch.float16
    for t in (residual, pre_scale, pre_shift):
        assert t is None or t.dtype == torch.float16
    assert bias is None or bias.dtype == torch.float32
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    y = torch.empty((n, ho, wo, cout), dtype=torch.float16, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_conv2d_nhwc_f16(ptr(x), n, h, w, cin, ptr(w_packed), cout, kh, kw, stride, pad, ptr(bias),
                                       ptr(residual), ptr(pre_scale), ptr(pre_shift), int(relu), ptr(y),
                                       stream_ptr(dev)), "hp_conv2d_nhwc_f16")
    return y


# ---- multi-view candidate matching (csrc/multiview.hip) ------------------------------------------------------------------------
MV_DIST_3D, MV_DIST_REPROJECTED = 0, 1  # HP_MV_DIST_*
_SEED_COLUMNS = ("view1", "view2", "match1_cand1", "match1_cand2", "match2_cand1", "match2_cand2")
_MATCH_COLUMNS = ("hypothesis_id", "cand1", "cand2")


def _h_i32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a), dtype=np.int32)


def ransac_make_infos(view_ids, label_ids, n_ransac_iter: int, seed: int = 0):
    """``cosypose_cext.make_ransac_infos`` (host): ``(seeds, tmatches)`` dicts of int32 arrays.  ``label_ids``: equal
    integers for equal labels."""
    view_ids, label_ids = _h_i32(view_ids), _h_i32(label_ids)
    assert view_ids.shape == label_ids.shape and view_ids.ndim == 1
    n = len(view_ids)
    ns, nm = C.c_int64(0), C.c_int64(0)
    check(lib().hp_ransac_make_infos(n, _np_ptr(view_ids), _np_ptr(label_ids), int(n_ransac_iter), int(seed), C.byref(ns),
                                     C.byref(nm), None, 0, None, 0), "hp_ransac_make_infos")
    seeds, matches = np.zeros((6, max(ns.value, 1)), np.int32), np.zeros((3, max(nm.value, 1)), np.int32)
    check(lib().hp_ransac_make_infos(n, _np_ptr(view_ids), _np_ptr(label_ids), int(n_ransac_iter), int(seed), C.byref(ns),
                                     C.byref(nm), _np_ptr(seeds), seeds.shape[1], _np_ptr(matches), matches.shape[1]),
          "hp_ransac_make_infos")
    return ({k: seeds[i, :ns.value].copy() for i, k in enumerate(_SEED_COLUMNS)},
            {k: matches[i, :nm.value].copy() for i, k in enumerate(_MATCH_COLUMNS)})


def ransac_find_inliers(seeds_view1, seeds_view2, hypothesis_id, cand1, cand2, dists, dist_threshold: float,
                        n_min_inliers: int):
    """``cosypose_cext.find_ransac_inliers`` (host): dict of ``inlier_matches_cand1`` / ``inlier_matches_cand2`` /
    ``best_hypotheses`` int32 arrays."""
    v1, v2, hid, c1, c2 = (_h_i32(a) for a in (seeds_view1, seeds_view2, hypothesis_id, cand1, cand2))
    dists = np.ascontiguousarray(np.asarray(dists), dtype=np.float32)
    assert len(v1) == len(v2) and len(hid) == len(c1) == len(c2) == len(dists)
    in1, in2, best = (np.zeros(max(len(hid), 1), np.int32), np.zeros(max(len(hid), 1), np.int32),
                      np.zeros(max(len(v1), 1), np.int32))
    ni, nb = C.c_int64(0), C.c_int64(0)
    check(lib().hp_ransac_find_inliers(len(v1), _np_ptr(v1), _np_ptr(v2), len(hid), _np_ptr(hid), _np_ptr(c1), _np_ptr(c2),
                                       _np_ptr(dists), float(dist_threshold), int(n_min_inliers), _np_ptr(in1), _np_ptr(in2),
                                       C.byref(ni), _np_ptr(best), C.byref(nb)), "hp_ransac_find_inliers")
    return {"inlier_matches_cand1": in1[:ni.value].copy(), "inlier_matches_cand2": in2[:ni.value].copy(),
            "best_hypotheses": best[:nb.value].copy()}


def _mv_tables(mesh_db, reads_symmetries: bool = True):
    """Device tables of a ``BatchedMeshes`` that went through ``.to(device)``: (points, symmetries, n_sym, n_obj, n_pts, s_max).
    ``reads_symmetries=False``: the caller's kernel modes never open the symmetry table (ADD, ADD-S), so labels whose
    symmetries could not be tabulated are no obstacle."""
    if reads_symmetries and getattr(mesh_db, "unsupported_symmetries", None):
        raise ValueError("continuous symmetries with an offset or an axis other than +x / +y / +z are not supported "
                         f"(make_bop_symmetries): {mesh_db.unsupported_symmetries}")
    t = getattr(mesh_db, "device_tables", None)
    if t is None:
        raise ValueError("the multi-view kernels need MeshDataBase.batched(...).to(device): no device tables on this mesh_db")
    pts, sym, n_sym = t["points"], t["symmetries"], t["n_sym"]
    assert pts.dim() == 3 and pts.shape[2] == 3 and sym.shape[0] == pts.shape[0] and sym.shape[2:] == (4, 4)
    assert n_sym.shape == (pts.shape[0],) and n_sym.dtype == torch.int32
    return pts, sym, n_sym, pts.shape[0], pts.shape[1], sym.shape[1]


def mv_estimate_camera_poses(poses: torch.Tensor, cand_obj, seeds, mesh_db) -> torch.Tensor:
    """``estimate_camera_poses_batch`` (``CP/multiview/ransac.py:23-75``) in one launch: ``TC1C2 [n_seeds, 4, 4]``.
    ``poses [n_cand, 4, 4]``, ``cand_obj [n_cand]`` = row of each candidate's label in ``mesh_db``, ``seeds`` = the four
    ``match*_cand*`` index columns (dict)."""
    pts, sym, n_sym, n_obj, n_pts, s_max = _mv_tables(mesh_db)
    dev = pts.device
    n_cand = poses.shape[0]
    assert poses.shape == (n_cand, 4, 4) and len(cand_obj) == n_cand
    _check_ids(cand_obj, n_obj, "mv_estimate_camera_poses: cand_obj")
    cols = []
    for k in _SEED_COLUMNS[2:]:
        _check_ids(seeds[k], n_cand, f"mv_estimate_camera_poses: {k}")
        cols.append(_i32(seeds[k], dev))
    n = len(cols[0])
    poses, cand_obj = _f32(poses, dev), _i32(cand_obj, dev)
    out = torch.empty(n, 4, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_mv_estimate_camera_poses(n, ptr(cols[0]), ptr(cols[1]), ptr(cols[2]), ptr(cols[3]), ptr(poses),
                                                ptr(cand_obj), n_cand, ptr(pts), ptr(sym), ptr(n_sym), n_obj, n_pts, s_max,
                                                ptr(out), stream_ptr(dev)), "hp_mv_estimate_camera_poses")
    return out


def mv_score_matches(hypothesis_id, cand1, cand2, TC1C2: torch.Tensor, poses1: torch.Tensor, obj1, poses2: torch.Tensor,
                     mesh_db, K: Optional[torch.Tensor] = None, return_sym_ids: bool = False):
    """``score_tmaches_batch`` (``CP/multiview/ransac.py:78-99``) in one launch over the rows ``(hypothesis_id, cand1,
    cand2)``: the symmetric distance between ``poses1[cand1]`` and ``TC1C2[hypothesis_id] @ poses2[cand2]`` for the
    object ``obj1[cand1]``.  With ``K [n_hyp, 3, 3]`` the reprojected distance (``symmetric_distance_reprojected``) is
    computed instead."""
    pts, sym, n_sym, n_obj, n_pts, s_max = _mv_tables(mesh_db)
    dev = pts.device
    n_hyp, n1, n2 = TC1C2.shape[0], poses1.shape[0], poses2.shape[0]
    assert TC1C2.shape == (n_hyp, 4, 4) and poses1.shape == (n1, 4, 4) and poses2.shape == (n2, 4, 4) and len(obj1) == n1
    assert len(hypothesis_id) == len(cand1) == len(cand2)
    _check_ids(hypothesis_id, n_hyp, "mv_score_matches: hypothesis_id")
    _check_ids(cand1, n1, "mv_score_matches: cand1")
    _check_ids(cand2, n2, "mv_score_matches: cand2")
    _check_ids(obj1, n_obj, "mv_score_matches: obj1")
    hid, c1, c2, obj1 = (_i32(a, dev) for a in (hypothesis_id, cand1, cand2, obj1))
    TC1C2, poses1, poses2 = _f32(TC1C2, dev), _f32(poses1, dev), _f32(poses2, dev)
    mode = MV_DIST_3D
    if K is not None:
        assert K.shape == (n_hyp, 3, 3)
        K, mode = _f32(K, dev), MV_DIST_REPROJECTED
    n = len(hid)
    dists = torch.empty(n, dtype=torch.float32, device=dev)
    sym_ids = torch.empty(n, dtype=torch.int32, device=dev) if return_sym_ids else None
    with torch.cuda.device(dev):
        check(lib().hp_mv_score_matches(n, ptr(hid), ptr(c1), ptr(c2), ptr(TC1C2), n_hyp, ptr(poses1), ptr(obj1), n1, ptr(poses2),
                                        n2, ptr(K), mode, ptr(pts), ptr(sym), ptr(n_sym), n_obj, n_pts, s_max, ptr(dists),
                                        ptr(sym_ids), stream_ptr(dev)), "hp_mv_score_matches")
    return (dists, sym_ids) if return_sym_ids else dists


def mv_ba_linearize(TWO_9d: torch.Tensor, TCW_9d: torch.Tensor, cand_obj, cand_view, TCO_cand: torch.Tensor, K: torch.Tensor,
                    obj_points: torch.Tensor, residuals_threshold: float):
    """One linearisation of the bundle adjustment (``MultiviewRefinement.forward_jacobian``,
    ``CP/multiview/bundle_adjustment.py:223-270``): ``(errors [n_cand, n_pts, 2], clipped [n_cand, n_pts, 2],
    JtJ [n_cand, 18, 18], Jte [n_cand, 18])``, all float64 -- see ``hp_mv_ba_linearize``."""
    dev = TWO_9d.device
    n_obj, n_views, n_cand, n_pts = TWO_9d.shape[0], TCW_9d.shape[0], TCO_cand.shape[0], obj_points.shape[1]
    assert TWO_9d.shape == (n_obj, 9) and TCW_9d.shape == (n_views, 9) and TCO_cand.shape == (n_cand, 4, 4)
    assert K.shape == (n_views, 3, 3) and obj_points.shape == (n_obj, n_pts, 3) and len(cand_obj) == len(cand_view) == n_cand
    _check_ids(cand_obj, n_obj, "mv_ba_linearize: cand_obj")
    _check_ids(cand_view, n_views, "mv_ba_linearize: cand_view")
    TWO_9d, TCW_9d = (t.to(device=dev, dtype=torch.float64).contiguous() for t in (TWO_9d, TCW_9d))
    TCO_cand, K, obj_points = (_f32(t, dev) for t in (TCO_cand, K, obj_points))
    cand_obj, cand_view = _i32(cand_obj, dev), _i32(cand_view, dev)
    errors = torch.empty(n_cand, n_pts, 2, dtype=torch.float64, device=dev)
    clipped = torch.empty_like(errors)
    JtJ = torch.empty(n_cand, 18, 18, dtype=torch.float64, device=dev)
    Jte = torch.empty(n_cand, 18, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_mv_ba_linearize(n_cand, ptr(TWO_9d), n_obj, ptr(TCW_9d), n_views, ptr(cand_obj), ptr(cand_view),
                                       ptr(TCO_cand), ptr(K), ptr(obj_points), n_pts, float(residuals_threshold), ptr(errors),
                                       ptr(clipped), ptr(JtJ), ptr(Jte), stream_ptr(dev)), "hp_mv_ba_linearize")
    return errors, clipped, JtJ, Jte


def seed_row_tables(seeds, tmatches):
    """Compact form of the tentative-match rows of ``ransac_make_infos``: ``(row_offsets [n_seeds + 1], pair_offsets [n_seeds],
    pair_cand1, pair_cand2)`` int32 on the host.  The rows of a seed are contiguous and are the match list of its view pair in
    the pair's order, so the list is kept once per view pair."""
    n_seeds = len(seeds["view1"])
    hid = np.asarray(tmatches["hypothesis_id"])
    row_off = np.searchsorted(hid, np.arange(n_seeds + 1)).astype(np.int32)
    pair_key = np.asarray(seeds["view1"]).astype(np.int64) * (1 << 32) + np.asarray(seeds["view2"]).astype(np.int64)
    first = np.flatnonzero(np.r_[True, pair_key[1:] != pair_key[:-1]]) if n_seeds else np.zeros(0, np.int64)
    counts = row_off[first + 1] - row_off[first]
    table_off = np.r_[0, np.cumsum(counts)].astype(np.int64)
    pair_of_seed = np.cumsum(np.r_[True, pair_key[1:] != pair_key[:-1]]) - 1 if n_seeds else np.zeros(0, np.int64)
    take = np.concatenate([np.arange(row_off[f], row_off[f + 1]) for f in first]) if n_seeds else np.zeros(0, np.int64)
    return (row_off, table_off[pair_of_seed].astype(np.int32), _h_i32(np.asarray(tmatches["cand1"])[take]),
            _h_i32(np.asarray(tmatches["cand2"])[take]))


def mv_score_seed_matches(seeds, tmatches, TC1C2: torch.Tensor, poses: torch.Tensor, cand_obj, mesh_db) -> torch.Tensor:
    """``score_tmaches_batch`` for the rows of ``ransac_make_infos`` without uploading them: the device holds the per-seed
    offsets and each view pair's match list once (``seed_row_tables``); the only per-row device memory is the result."""
    pts, sym, n_sym, n_obj, n_pts, s_max = _mv_tables(mesh_db)
    dev = pts.device
    n_rows, n_seeds, n_cand = len(tmatches["hypothesis_id"]), TC1C2.shape[0], poses.shape[0]
    assert TC1C2.shape == (n_seeds, 4, 4) and poses.shape == (n_cand, 4, 4) and len(cand_obj) == n_cand == len(poses)
    assert len(seeds["view1"]) == n_seeds
    _check_ids(cand_obj, n_obj, "mv_score_seed_matches: cand_obj")
    _check_ids(tmatches["cand1"], n_cand, "mv_score_seed_matches: cand1")
    _check_ids(tmatches["cand2"], n_cand, "mv_score_seed_matches: cand2")
    row_off, pair_off, pc1, pc2 = (torch.as_tensor(a).to(dev) for a in seed_row_tables(seeds, tmatches))
    TC1C2, poses, cand_obj = _f32(TC1C2, dev), _f32(poses, dev), _i32(cand_obj, dev)
    dists = torch.empty(n_rows, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_mv_score_seed_matches(n_rows, n_seeds, ptr(row_off), ptr(pair_off), ptr(pc1), ptr(pc2), len(pc1), ptr(TC1C2),
                                             ptr(poses), ptr(cand_obj), n_cand, ptr(pts), ptr(sym), ptr(n_sym), n_obj, n_pts, s_max,
                                             ptr(dists), stream_ptr(dev)), "hp_mv_score_seed_matches")
    return dists


# ---- pose-error metrics (csrc/pose_errors.hip) ---------------------------------------------------------------------------------
POSE_ERR_MODES = {"ADD": 0, "ADD-S": 1, "ADD-SYM": 2, "MSSD": 3, "MSPD": 4}  # HP_POSE_ERR_*
POSE_ERR_PRED_TILE, POSE_ERR_GT_BLOCK = 512, 1024  # HP_POSE_ERR_PRED_TILE / HP_POSE_ERR_GT_BLOCK (tests/test_pose_errors_host.py)
_POSE_ERR_MAX_ROWS = 65535  # rows of one hp_pose_errors call
_POSE_ERR_READS_SYM = (2, 3, 4)


def pose_errors_workspace_bytes(n_rows: int, max_pts: int) -> int:
    """``hp_pose_errors_workspace_bytes``: rows x blocks of ground-truth points x 32 bytes."""
    n = int(lib().hp_pose_errors_workspace_bytes(int(n_rows), int(max_pts)))
    assert n >= 0, "pose_errors_workspace_bytes: n_rows >= 0 and max_pts >= 1"
    return n


def pose_errors_tables(pred_id, gt_id, obj_id, mode, poses_pred: torch.Tensor, poses_gt: torch.Tensor, points: torch.Tensor,
                       symmetries: torch.Tensor, n_sym: torch.Tensor, n_pts: torch.Tensor, K: Optional[torch.Tensor] = None,
                       return_assign: bool = False) -> Dict[str, torch.Tensor]:
    """``hp_pose_errors`` on explicit device tables (``points [n_obj, max_pts, 3]``, ``symmetries [n_obj, s_max, 4, 4]``,
    ``n_sym`` / ``n_pts [n_obj]`` int32).  Row ``r`` scores ``poses_pred[pred_id[r]]`` against ``poses_gt[gt_id[r]]`` on object
    ``obj_id[r]`` in mode ``mode[r]`` (``POSE_ERR_MODES`` values); ``K [n_rows, 3, 3]`` for MSPD rows.  Returns ``norm_avg``,
    ``xyz_avg [n, 3]``, ``norm_max``, ``sym_id``, ``TCO_xyz [n, 3]``, ``TCO_norm`` and, on request, ``assign [n, max_pts]``."""
    dev = points.device
    n_obj, max_pts, s_max = points.shape[0], points.shape[1], symmetries.shape[1]
    assert points.shape == (n_obj, max_pts, 3) and symmetries.shape == (n_obj, s_max, 4, 4)
    assert n_sym.shape == (n_obj,) and n_sym.dtype == torch.int32 and n_pts.shape == (n_obj,) and n_pts.dtype == torch.int32
    n_pred, n_gt = poses_pred.shape[0], poses_gt.shape[0]
    assert poses_pred.shape == (n_pred, 4, 4) and poses_gt.shape == (n_gt, 4, 4)
    n = len(pred_id)
    assert len(gt_id) == len(obj_id) == len(mode) == n
    _check_ids(pred_id, n_pred, "pose_errors: pred_id")
    _check_ids(gt_id, n_gt, "pose_errors: gt_id")
    _check_ids(obj_id, n_obj, "pose_errors: obj_id")
    _check_ids(mode, len(POSE_ERR_MODES), "pose_errors: mode")
    # a mode column still on the host says whether any row is ADD-S: without one the ADD-S launches and their workspace are skipped
    host_mode = torch.as_tensor(mode)
    host_mode = host_mode.numpy() if host_mode.device.type == "cpu" else None
    pred_id, gt_id, obj_id, mode = (_i32(a, dev) for a in (pred_id, gt_id, obj_id, mode))
    poses_pred, poses_gt, points, symmetries = (_f32(t, dev) for t in (poses_pred, poses_gt, points, symmetries))
    n_sym, n_pts = n_sym.to(dev).contiguous(), n_pts.to(dev).contiguous()
    if K is not None:
        assert K.shape == (n, 3, 3), "pose_errors: one K per row"
        K = _f32(K, dev)
    out = {"norm_avg": torch.empty(n, dtype=torch.float32, device=dev), "xyz_avg": torch.empty(n, 3, dtype=torch.float32, device=dev),
           "norm_max": torch.empty(n, dtype=torch.float32, device=dev), "sym_id": torch.empty(n, dtype=torch.int32, device=dev),
           "TCO_xyz": torch.empty(n, 3, dtype=torch.float32, device=dev), "TCO_norm": torch.empty(n, dtype=torch.float32, device=dev)}
    if return_assign:
        out["assign"] = torch.empty(n, max_pts, dtype=torch.int32, device=dev)
    step = _POSE_ERR_MAX_ROWS
    if return_assign:
        step = max(1, min(step, ((1 << 31) - 1) // max_pts))
    with torch.cuda.device(dev):
        for r0 in range(0, max(n, 1), step):  # one launch for anything an evaluation batch holds; chunks only past the grid limit
            m = min(step, n - r0)
            sl = slice(r0, r0 + m)
            n_add_s = -1 if host_mode is None else int((host_mode[sl] == POSE_ERR_MODES["ADD-S"]).sum())
            nbytes = pose_errors_workspace_bytes(m, max_pts) if n_add_s else 0
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None
            check(lib().hp_pose_errors(m, ptr(pred_id[sl]), ptr(gt_id[sl]), ptr(obj_id[sl]), ptr(mode[sl]), n_add_s, ptr(poses_pred), n_pred,
                                       ptr(poses_gt), n_gt, ptr(K[sl]) if K is not None else None, ptr(points), ptr(symmetries),
                                       ptr(n_sym), ptr(n_pts), n_obj, max_pts, s_max, ptr(out["norm_avg"][sl]), ptr(out["xyz_avg"][sl]),
                                       ptr(out["norm_max"][sl]), ptr(out["sym_id"][sl]), ptr(out["TCO_xyz"][sl]),
                                       ptr(out["TCO_norm"][sl]), ptr(out["assign"][sl]) if return_assign else None, ptr(ws),
                                       nbytes, stream_ptr(dev)), "hp_pose_errors")
    return out


def pose_errors(pred_id, gt_id, obj_id, mode, poses_pred: torch.Tensor, poses_gt: torch.Tensor, mesh_db,
                K: Optional[torch.Tensor] = None, exact_meshes: bool = True, return_assign: bool = False):
    """``hp_pose_errors`` on the device tables of ``mesh_db`` (``MeshDataBase.batched().to(device)``).  ``exact_meshes=True``
    counts each object's own ``n_points`` (the reference's exact mode), ``False`` the whole padded table.  ``mode``: one
    ``POSE_ERR_MODES`` value per row, on the host -- the symmetry-reading modes refuse a ``mesh_db`` with
    ``unsupported_symmetries`` like the multi-view wrappers; a ``mode`` column that already lives on the device cannot be
    inspected and is treated as reading symmetries."""
    m = torch.as_tensor(mode)
    reads_sym = m.device.type != "cpu" or bool(np.isin(m.numpy(), _POSE_ERR_READS_SYM).any())
    pts, sym, n_sym, n_obj, n_pad, s_max = _mv_tables(mesh_db, reads_symmetries=reads_sym)
    if exact_meshes:
        n_pts = torch.as_tensor(np.asarray([mesh_db.infos[label]["n_points"] for label in mesh_db.labels], dtype=np.int32)).to(pts.device)
    else:
        n_pts = torch.full((n_obj,), n_pad, dtype=torch.int32, device=pts.device)
    return pose_errors_tables(pred_id, gt_id, obj_id, mode, poses_pred, poses_gt, pts, sym, n_sym, n_pts, K=K,
                              return_assign=return_assign)


# ---- training / validation losses (csrc/pose_losses.hip) -----------------------------------------------------------------------
POSE_LOSS_SYM_CHUNK = 8  # HP_POSE_LOSS_SYM_CHUNK


def _loss_tables(what: str, TCO_possible_gt: torch.Tensor, points: torch.Tensor, **per_row: Tuple[torch.Tensor, tuple]):
    """Shapes as the reference asserts them; float32 contiguous device tensors back (there is no CPU path)."""
    assert TCO_possible_gt.dim() == 4 and TCO_possible_gt.shape[-2:] == (4, 4), f"{what}: TCO_possible_gt [B, S, 4, 4]"
    b, s = TCO_possible_gt.shape[:2]
    assert points.dim() == 3 and points.shape[0] == b and points.shape[-1] == 3, f"{what}: points [B, N, 3]"
    tensors = {"TCO_possible_gt": TCO_possible_gt, "points": points}
    for name, (t, shape) in per_row.items():
        if t is not None:
            assert tuple(t.shape) == (b, *shape), f"{what}: {name} {[b, *shape]}"
            tensors[name] = t
    dev = points.device
    for name, t in tensors.items():
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"{what}: {name} is on {t.device}; every input lives on one GPU (happypose_amd has no CPU path)")
    return b, s, points.shape[1], {name: _f32(t, dev) for name, t in tensors.items()}


def _loss_workspace(b: int, s: int, dev) -> Tuple[torch.Tensor, int]:
    nbytes = int(lib().hp_pose_loss_workspace_bytes(b, max(s, 1)))
    return torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev), nbytes


def loss_co_symmetric_forward(TCO_possible_gt: torch.Tensor, TCO_pred: torch.Tensor, points: torch.Tensor):
    """``hp_loss_co_symmetric``: ``(loss [B], sym_id [B] int32, TCO_assign [B, 4, 4])``."""
    b, s, n, t = _loss_tables("loss_CO_symmetric", TCO_possible_gt, points, TCO_pred=(TCO_pred, (4, 4)))
    dev = t["points"].device
    loss = torch.empty(b, dtype=torch.float32, device=dev)
    sym_id = torch.empty(b, dtype=torch.int32, device=dev)
    assign = torch.empty(b, 4, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws, nbytes = _loss_workspace(b, s, dev)
        check(lib().hp_loss_co_symmetric(b, s, n, ptr(t["TCO_possible_gt"]), ptr(t["TCO_pred"]), ptr(t["points"]), ptr(loss), ptr(sym_id),
                                         ptr(assign), ptr(ws), nbytes, stream_ptr(dev)), "hp_loss_co_symmetric")
    return loss, sym_id, assign


def loss_co_symmetric_backward(TCO_possible_gt: torch.Tensor, TCO_pred: torch.Tensor, points: torch.Tensor, sym_id: torch.Tensor,
                               grad_loss: torch.Tensor) -> torch.Tensor:
    """``hp_loss_co_symmetric_backward``: the gradient with respect to ``TCO_pred`` ``[B, 4, 4]`` (last row zero)."""
    b, s, n, t = _loss_tables("loss_CO_symmetric", TCO_possible_gt, points, TCO_pred=(TCO_pred, (4, 4)), grad_loss=(grad_loss, ()))
    dev = t["points"].device
    assert sym_id.shape == (b,) and sym_id.dtype == torch.int32 and sym_id.device == dev
    grad = torch.empty(b, 4, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_loss_co_symmetric_backward(b, s, n, ptr(t["TCO_possible_gt"]), ptr(t["TCO_pred"]), ptr(t["points"]),
                                                  ptr(sym_id.contiguous()), ptr(t["grad_loss"]), ptr(grad), stream_ptr(dev)),
              "hp_loss_co_symmetric_backward")
    return grad


def loss_refiner_forward(TCO_possible_gt: torch.Tensor, TCO_input: torch.Tensor, refiner_outputs: torch.Tensor, K_crop: torch.Tensor,
                         points: torch.Tensor, tCR: Optional[torch.Tensor] = None):
    """``hp_loss_refiner_disentangled`` (``tCR=None``: CosyPose's form): ``(loss [B], parts [B, 3] = orn, xy, z, sym_ids [B, 3]
    int32)``."""
    b, s, n, t = _loss_tables("loss_refiner_CO_disentangled", TCO_possible_gt, points, TCO_input=(TCO_input, (4, 4)),
                              refiner_outputs=(refiner_outputs, (9,)), K_crop=(K_crop, (3, 3)), tCR=(tCR, (3,)))
    dev = t["points"].device
    loss = torch.empty(b, dtype=torch.float32, device=dev)
    parts = torch.empty(b, 3, dtype=torch.float32, device=dev)
    sym_ids = torch.empty(b, 3, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws, nbytes = _loss_workspace(b, s, dev)
        check(lib().hp_loss_refiner_disentangled(b, s, n, ptr(t["TCO_possible_gt"]), ptr(t["TCO_input"]), ptr(t["refiner_outputs"]),
                                                 ptr(t["K_crop"]), ptr(t["points"]), ptr(t.get("tCR")), ptr(loss), ptr(parts),
                                                 ptr(sym_ids), ptr(ws), nbytes, stream_ptr(dev)), "hp_loss_refiner_disentangled")
    return loss, parts, sym_ids


def loss_refiner_backward(TCO_possible_gt: torch.Tensor, TCO_input: torch.Tensor, refiner_outputs: torch.Tensor, K_crop: torch.Tensor,
                          points: torch.Tensor, tCR: Optional[torch.Tensor], sym_ids: torch.Tensor, grad_loss: torch.Tensor,
                          return_parts: bool = False):
    """``hp_loss_refiner_disentangled_backward``: the gradient with respect to ``refiner_outputs`` ``[B, 9]``; with
    ``return_parts`` also the same gradient split by term ``[B, 3, 9]``."""
    b, s, n, t = _loss_tables("loss_refiner_CO_disentangled", TCO_possible_gt, points, TCO_input=(TCO_input, (4, 4)),
                              refiner_outputs=(refiner_outputs, (9,)), K_crop=(K_crop, (3, 3)), tCR=(tCR, (3,)),
                              grad_loss=(grad_loss, ()))
    dev = t["points"].device
    assert sym_ids.shape == (b, 3) and sym_ids.dtype == torch.int32 and sym_ids.device == dev
    grad = torch.empty(b, 9, dtype=torch.float32, device=dev)
    grad_parts = torch.empty(b, 3, 9, dtype=torch.float32, device=dev) if return_parts else None
    with torch.cuda.device(dev):
        check(lib().hp_loss_refiner_disentangled_backward(b, s, n, ptr(t["TCO_possible_gt"]), ptr(t["TCO_input"]),
                                                          ptr(t["refiner_outputs"]), ptr(t["K_crop"]), ptr(t["points"]), ptr(t.get("tCR")),
                                                          ptr(sym_ids.contiguous()), ptr(t["grad_loss"]), ptr(grad), ptr(grad_parts),
                                                          stream_ptr(dev)), "hp_loss_refiner_disentangled_backward")
    return (grad, grad_parts) if return_parts else grad


def _bce_tables(logits: torch.Tensor, targets: torch.Tensor, temperature: float, grad_loss: Optional[torch.Tensor] = None):
    dev = _on_device("renderings_confidence_loss", logits=logits, is_positive=targets, grad_loss=grad_loss)
    assert logits.shape == targets.shape, f"renderings_confidence_loss: logits {list(logits.shape)} and is_positive {list(targets.shape)}"
    assert grad_loss is None or grad_loss.shape == logits.shape
    assert float(temperature) > 0 and math.isfinite(float(temperature)), "renderings_confidence_loss: temperature > 0"
    return dev, _f32(logits, dev), _f32(targets, dev), None if grad_loss is None else _f32(grad_loss, dev)


def loss_bce_logits_forward(logits: torch.Tensor, targets: torch.Tensor, temperature: float = 1.0) -> torch.Tensor:
    """``hp_loss_bce_logits``: per element ``BCEWithLogitsLoss(reduction="none")(logits / temperature, targets)``."""
    dev, logits, targets, _ = _bce_tables(logits, targets, temperature)
    loss = torch.empty(logits.shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_loss_bce_logits(logits.numel(), ptr(logits), ptr(targets), float(temperature), ptr(loss), stream_ptr(dev)),
              "hp_loss_bce_logits")
    return loss


def loss_bce_logits_backward(logits: torch.Tensor, targets: torch.Tensor, temperature: float, grad_loss: torch.Tensor) -> torch.Tensor:
    """``hp_loss_bce_logits_backward``: ``(sigmoid(logits / temperature) - targets) / temperature * grad_loss``."""
    dev, logits, targets, grad_loss = _bce_tables(logits, targets, temperature, grad_loss)
    grad = torch.empty(logits.shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_loss_bce_logits_backward(logits.numel(), ptr(logits), ptr(targets), float(temperature), ptr(grad_loss), ptr(grad),
                                                stream_ptr(dev)), "hp_loss_bce_logits_backward")
    return grad


# ---- training hypotheses (csrc/train_hyp.hip) ------------------------------------------------------------------------------------
def _on_device(what: str, **tensors) -> torch.device:
    """Every given tensor lives on one GPU (there is no CPU path): its device."""
    dev = None
    for name, t in tensors.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or (dev is not None and t.device != dev):
            where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{what}: {name} is on {where}; every input lives on one GPU (happypose_amd has no CPU path)")
        dev = t.device
    return dev


def pose_add_noise(TCO: torch.Tensor, euler_deg_std=(15, 15, 15), trans_std=(0.01, 0.01, 0.05), *, seed: int = 0, row_offset: int = 0,
                   repeat: int = 1, noise: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                   return_noise: bool = False):
    """``hp_pose_add_noise``: ``TCO [m, 4, 4]`` -> ``[m * repeat, 4, 4]``, row ``i`` a noisy copy of pose ``i // repeat``.
    ``noise [m * repeat, 6]`` (angles in radians, metres) is used as it is; without it the noise is drawn from
    ``(seed, row_offset + i)`` with the given standard deviations.  ``out`` may be ``TCO`` itself when ``repeat == 1``.
    ``return_noise``: also the six values of every row ``[m * repeat, 6]``."""
    dev = _on_device("pose_add_noise", TCO=TCO, noise=noise, out=out)
    assert TCO.dim() == 3 and TCO.shape[1:] == (4, 4), "pose_add_noise: TCO [m, 4, 4]"
    assert repeat >= 1, "pose_add_noise: repeat >= 1"
    assert 0 <= seed < 2 ** 64 and 0 <= row_offset < 2 ** 64, "pose_add_noise: seed and row_offset are unsigned 64-bit integers"
    n = TCO.shape[0] * repeat
    assert n < 2 ** 31, "pose_add_noise: at most 2^31 - 1 rows"
    TCO = _f32(TCO, dev)
    if out is None:
        out = torch.empty(n, 4, 4, dtype=torch.float32, device=dev)
    assert out.shape == (n, 4, 4) and out.dtype == torch.float32 and out.is_contiguous(), "pose_add_noise: out [m * repeat, 4, 4] float32"
    std = (C.c_float * 3)(*[float(v) for v in euler_deg_std]), (C.c_float * 3)(*[float(v) for v in trans_std])
    if noise is not None:
        assert noise.shape == (n, 6), "pose_add_noise: noise [m * repeat, 6]"
        noise = _f32(noise, dev)
    noise_out = torch.empty(n, 6, dtype=torch.float32, device=dev) if return_noise else None
    with torch.cuda.device(dev):
        check(lib().hp_pose_add_noise(n, repeat, ptr(TCO), std[0], std[1], seed, row_offset, ptr(noise), ptr(out), ptr(noise_out),
                                      stream_ptr(dev)), "hp_pose_add_noise")
    return (out, noise_out) if return_noise else out


def tco_init_from_boxes(boxes: torch.Tensor, K: torch.Tensor, z_range=(1.0, 1.0), im_ids=None, box_ids=None) -> torch.Tensor:
    """``hp_tco_init_from_boxes``: one pose per row of ``im_ids`` / ``box_ids`` (without either: per box, box ``i`` with ``K[i]``)."""
    dev = _on_device("tco_init_from_boxes", boxes=boxes, K=K)
    assert len(z_range) == 2
    assert boxes.dim() == 2 and boxes.shape[-1] == 4 and K.dim() == 3 and K.shape[1:] == (3, 3)
    n = len(im_ids) if im_ids is not None else len(box_ids) if box_ids is not None else boxes.shape[0]
    assert box_ids is not None or boxes.shape[0] == n, "one box per row unless box_ids is given"
    assert im_ids is not None or K.shape[0] == n, "one intrinsics matrix per row unless im_ids is given"
    _check_ids(im_ids, K.shape[0], "tco_init_from_boxes: im_ids -> K")
    _check_ids(box_ids, boxes.shape[0], "tco_init_from_boxes: box_ids -> boxes")
    boxes, K = _f32(boxes, dev), _f32(K, dev)
    im_ids = None if im_ids is None else _i32(im_ids, dev)
    box_ids = None if box_ids is None else _i32(box_ids, dev)
    assert (im_ids is None or im_ids.shape == (n,)) and (box_ids is None or box_ids.shape == (n,))
    out = torch.empty(n, 4, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_tco_init_from_boxes(n, ptr(boxes), boxes.shape[0], ptr(box_ids), ptr(K), K.shape[0], ptr(im_ids),
                                           C.c_float(z_range[0]), C.c_float(z_range[1]), ptr(out), stream_ptr(dev)),
              "hp_tco_init_from_boxes")
    return out


SPHERE26_VIEWS, SPHERE26_CANDIDATES = 26, 104


def views_sphere26(TCO: torch.Tensor, tCR: Optional[torch.Tensor] = None, inplane_rotations: bool = True) -> torch.Tensor:
    """``hp_views_sphere26``: ``TCO [B, 4, 4]`` -> the candidate views of the coarse classifier ``[B, 104, 4, 4]`` (candidate
    ``view * 4 + rot``), or ``[B, 26, 4, 4]`` without the in-plane rotations: ``make_TCO_multiview(TCO, tCR, "sphere_26views",
    remove_TCO_rendering=True, views_inplane_rotations=True)``.  ``tCR [B, 3]`` defaults to the pose's translation.  Candidate 0
    is camera 0 re-aimed at the reference point.  The header states the offsets' order and the degenerate look-at rule."""
    dev = _on_device("views_sphere26", TCO=TCO, tCR=tCR)
    assert TCO.dim() == 3 and TCO.shape[1:] == (4, 4), "views_sphere26: TCO [B, 4, 4]"
    b = TCO.shape[0]
    assert b * SPHERE26_CANDIDATES < 2 ** 31, "views_sphere26: too many poses"
    TCO = _f32(TCO, dev)
    if tCR is not None:
        assert tCR.shape == (b, 3), "views_sphere26: tCR [B, 3]"
        tCR = _f32(tCR, dev)
    out = torch.empty(b, SPHERE26_CANDIDATES if inplane_rotations else SPHERE26_VIEWS, 4, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_views_sphere26(b, ptr(TCO), ptr(tCR), int(bool(inplane_rotations)), ptr(out), stream_ptr(dev)), "hp_views_sphere26")
    return out


def coarse_hypotheses(TCO: torch.Tensor, n_hypotheses: int, *, seed: int, row_offset: int = 0, n_rendered_views: int = 1,
                      p_force_positive: float = 0.7) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``hp_coarse_hypotheses``: per image ``n_hypotheses`` distinct candidates of :func:`views_sphere26` in one launch --
    ``(hyp [B, n_hyp, 4, 4], view_ids [B, n_hyp] int32, is_positive [B, n_hyp] float32)``.  ``view_ids[b]`` are the first entries
    of a uniform random permutation of ``0 .. 103`` drawn from ``(seed, row_offset + b)`` alone; where id 0 (the positive) is
    absent it is forced into slot ``randint(n_rendered_views)`` with probability ``p_force_positive``.  Only the selected
    candidates' poses are evaluated, with the bits :func:`views_sphere26` gives them.  The reference's ``np.random`` stream is
    not reproduced; the header states the counter layout."""
    dev = _on_device("coarse_hypotheses", TCO=TCO)
    assert TCO.dim() == 3 and TCO.shape[1:] == (4, 4), "coarse_hypotheses: TCO [B, 4, 4]"
    assert 0 <= seed < 2 ** 64 and 0 <= row_offset < 2 ** 64, "coarse_hypotheses: seed and row_offset are unsigned 64-bit integers"
    b, n_hyp = TCO.shape[0], int(n_hypotheses)
    assert b < 2 ** 31 // SPHERE26_CANDIDATES, "coarse_hypotheses: too many images"
    TCO = _f32(TCO, dev)
    hyp = torch.empty(b, max(n_hyp, 0), 4, 4, dtype=torch.float32, device=dev)
    view_ids = torch.empty(b, max(n_hyp, 0), dtype=torch.int32, device=dev)
    is_positive = torch.empty(b, max(n_hyp, 0), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_coarse_hypotheses(b, n_hyp, int(n_rendered_views), float(p_force_positive), ptr(TCO), seed, row_offset, ptr(hyp),
                                         ptr(view_ids), ptr(is_positive), stream_ptr(dev)), "hp_coarse_hypotheses")
    return hyp, view_ids, is_positive


# ---- head training (csrc/head_train.hip) -----------------------------------------------------------------------------------------
def _f32_in(what: str, name: str, t: Optional[torch.Tensor], shape) -> None:
    if t is not None:
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape), \
            f"{what}: {name} must be contiguous float32 {list(shape)}, got {t.dtype} {list(t.shape)}"


def head_backward(feat: torch.Tensor, d_pose: Optional[torch.Tensor], W: Optional[torch.Tensor] = None, *,
                  d_logits: Optional[torch.Tensor] = None,
                  n_logits: int = 0, w: Optional[torch.Tensor] = None, dW: Optional[torch.Tensor] = None,
                  db: Optional[torch.Tensor] = None, accumulate: bool = False, return_d_feat: bool = False):
    """``hp_head_backward``: ``feat [B, C]``, ``d_pose [B, pose_dim]`` and ``d_logits [B, n_logits]`` (None: zeros; ``n_logits``
    then gives the width) -> ``dW [O, C]``, ``db [O]`` with ``O = pose_dim + n_logits``, the pose rows first; optional row
    weights ``w [B]``.  ``d_pose`` None: a network without a pose head (``pose_dim == 0``, the coarse classifier), the logits rows
    alone.  ``dW`` / ``db`` given: written in place, added to with ``accumulate``.  ``return_d_feat``: also
    ``d_feat [B, C] = (w d_out) @ W`` -- ``W [O, C]`` is needed for it alone.  Bit-identical from run to run (the header states the
    order of the sums)."""
    dev = _on_device("head_backward", feat=feat, d_pose=d_pose, d_logits=d_logits, w=w, W=W, dW=dW, db=db)
    assert feat.dim() == 2 and (d_pose is None or d_pose.dim() == 2), "head_backward: feat [B, C], d_pose [B, pose_dim]"
    B, Cf = feat.shape
    pose_dim = 0 if d_pose is None else d_pose.shape[1]
    if pose_dim == 0:
        d_pose = None  # nothing to read: the library takes a null pointer for an absent pose head
    if d_logits is not None:
        assert d_logits.dim() == 2, "head_backward: d_logits [B, n_logits]"
        n_logits = d_logits.shape[1]
    O = pose_dim + n_logits
    assert 1 <= O <= 32, "head_backward: pose_dim + n_logits must be 1 .. 32"
    assert not accumulate or (dW is not None and db is not None), "head_backward: accumulate adds to given dW / db"
    assert not return_d_feat or W is not None, "head_backward: d_feat needs the head matrix W [O, C]"
    _f32_in("head_backward", "feat", feat, (B, Cf))
    _f32_in("head_backward", "d_pose", d_pose, (B, pose_dim))
    _f32_in("head_backward", "d_logits", d_logits, (B, n_logits))
    _f32_in("head_backward", "w", w, (B,))
    _f32_in("head_backward", "W", W, (O, Cf))
    f = dict(dtype=torch.float32, device=dev)
    dW = torch.empty((O, Cf), **f) if dW is None else dW
    db = torch.empty((O,), **f) if db is None else db
    _f32_in("head_backward", "dW", dW, (O, Cf))
    _f32_in("head_backward", "db", db, (O,))
    d_feat = torch.empty((B, Cf), **f) if return_d_feat else None
    n_ws = int(lib().hp_head_backward_ws_floats(B, Cf, O))
    ws = torch.empty((max(n_ws, 1),), **f)
    with torch.cuda.device(dev):
        check(lib().hp_head_backward(B, Cf, pose_dim, n_logits, ptr(feat), ptr(d_pose), ptr(d_logits), ptr(w), ptr(W), int(bool(accumulate)),
                                     ptr(dW), ptr(db), ptr(d_feat), ptr(ws), n_ws, stream_ptr(dev)), "hp_head_backward")
    return (dW, db, d_feat) if return_d_feat else (dW, db)


def fc_backward(d_out: torch.Tensor, x: torch.Tensor, *, dW: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None,
                accumulate: bool = False):
    """``hp_fc_backward``: ``d_out [B, O]`` (the ``d_feat`` of :func:`head_backward`), the layer's input ``x [B, C]`` ->
    ``dW [O, C] = d_out^T x`` and ``db [O]``, the sum over the rows one chain in index order."""
    dev = _on_device("fc_backward", d_out=d_out, x=x, dW=dW, db=db)
    assert d_out.dim() == 2 and x.dim() == 2 and d_out.shape[0] == x.shape[0], "fc_backward: d_out [B, O], x [B, C]"
    (B, O), Cx = d_out.shape, x.shape[1]
    assert O >= 1 and Cx >= 1, "fc_backward: empty layer"
    assert not accumulate or (dW is not None and db is not None), "fc_backward: accumulate adds to given dW / db"
    _f32_in("fc_backward", "d_out", d_out, (B, O))
    _f32_in("fc_backward", "x", x, (B, Cx))
    f = dict(dtype=torch.float32, device=dev)
    dW = torch.empty((O, Cx), **f) if dW is None else dW
    db = torch.empty((O,), **f) if db is None else db
    _f32_in("fc_backward", "dW", dW, (O, Cx))
    _f32_in("fc_backward", "db", db, (O,))
    with torch.cuda.device(dev):
        check(lib().hp_fc_backward(B, O, Cx, ptr(d_out), ptr(x), int(bool(accumulate)), ptr(dW), ptr(db), stream_ptr(dev)), "hp_fc_backward")
    return dW, db


def grad_sq_norm(g: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hp_grad_sq_norm``: the sum of squares of a flat float32 buffer as a device scalar ``[1]`` (fixed-order two-level
    reduction, bit-identical from run to run).  Its square root is ``clip_grad_norm_``'s total norm."""
    dev = _on_device("grad_sq_norm", g=g, out=out)
    assert g.dim() == 1 and g.dtype == torch.float32 and g.is_contiguous(), "grad_sq_norm: a flat contiguous float32 buffer"
    n = g.shape[0]
    assert n < 2 ** 31, "grad_sq_norm: at most 2^31 - 1 elements"
    out = torch.empty((1,), dtype=torch.float32, device=dev) if out is None else out
    _f32_in("grad_sq_norm", "out", out, (1,))
    n_ws = int(lib().hp_grad_sq_norm_ws_floats(n))
    ws = torch.empty((max(n_ws, 1),), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_grad_sq_norm(n, ptr(g), ptr(out), ptr(ws), n_ws, stream_ptr(dev)), "hp_grad_sq_norm")
    return out


def adamw_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, *, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
               weight_decay: float = 0.0, step: int, decoupled: bool = False, sq_norm: Optional[torch.Tensor] = None,
               max_norm: Optional[torch.Tensor] = None) -> None:
    """``hp_adamw_step``: one launch over the flat float32 buffers ``p``, ``g``, ``m``, ``v [N]``; ``p``, ``m``, ``v`` are updated
    in place in the operation order of torch's ``_single_tensor_adam`` (``decoupled``: ``AdamW``; else ``Adam`` with L2).
    ``sq_norm`` (from :func:`grad_sq_norm`) and ``max_norm``, device scalars ``[1]``, both or neither: the gradient is clipped by
    ``min(1, max_norm / (sqrt(sq_norm) + 1e-6))`` inside the launch.  ``step`` counts from 1."""
    dev = _on_device("adamw_step", p=p, g=g, m=m, v=v, sq_norm=sq_norm, max_norm=max_norm)
    assert p.dim() == 1 and p.shape[0] < 2 ** 31, "adamw_step: flat buffers of at most 2^31 - 1 elements"
    n = p.shape[0]
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _f32_in("adamw_step", name, t, (n,))
    _f32_in("adamw_step", "sq_norm", sq_norm, (1,))
    _f32_in("adamw_step", "max_norm", max_norm, (1,))
    assert (sq_norm is None) == (max_norm is None), "adamw_step: sq_norm and max_norm come together"
    assert int(step) >= 1, "adamw_step: step counts from 1"
    with torch.cuda.device(dev):
        check(lib().hp_adamw_step(n, ptr(p), ptr(g), ptr(m), ptr(v), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                  float(weight_decay), int(step), int(bool(decoupled)), ptr(sq_norm), ptr(max_norm), stream_ptr(dev)),
              "hp_adamw_step")


# --------------------------------------------------------------------------------------------------------------- scenes (scene.hip)
SCENE_VIS_FIELDS = 10  # HP_SCENE_VIS_FIELDS
SCENE_MAX_DILATE = 3   # HP_SCENE_MAX_DILATE
SCENE_VIS_COLUMNS = ("px_count_all", "px_count_visib", "all_x_min", "all_y_min", "all_x_max", "all_y_max",
                     "visib_x_min", "visib_y_min", "visib_x_max", "visib_y_max")


def _scene_layers(layer_off, depth: torch.Tensor):
    """Checks shared by the layer-reading wrappers: ``layer_off`` [n_cam + 1] (checked where it still lives on the host: starts
    at 0, ascends, ends at the layer count) and ``depth`` [L, 1, H, W] float32 on the device."""
    assert depth.dim() == 4 and depth.shape[1] == 1 and depth.dtype == torch.float32 and depth.is_cuda, "layer depth: [L, 1, H, W] float32 on the device"
    n_layers, _, h, w = depth.shape
    off = torch.as_tensor(layer_off)
    assert off.dim() == 1 and off.numel() >= 1, "layer_off: [n_cam + 1]"
    if off.device.type == "cpu":
        o = off.numpy().astype(np.int64)
        assert o[0] == 0 and o[-1] == n_layers and (np.diff(o) >= 0).all(), f"layer_off {o.tolist()} does not partition {n_layers} layers"
    return _i32(off, depth.device), off.numel() - 1, n_layers, h, w


def scene_compose(layer_off, rgb: torch.Tensor, nrm: Optional[torch.Tensor], depth: torch.Tensor) -> Dict[str, Optional[torch.Tensor]]:
    """``hp_scene_compose``: per-pixel z-merge of rasterised layers (``rasterize(..., render_depth=True)`` outputs: ``rgb`` /
    ``nrm`` [L, 3, H, W], ``depth`` [L, 1, H, W], 0 = background), sorted by camera with ``layer_off`` [n_cam + 1] giving each
    camera's range.  The winner of a pixel is the camera's layer with the smallest depth > 0, the lowest layer on a tie.  Returns
    ``rgb`` [n_cam, 3, H, W], ``normals`` (or None), ``depth`` [n_cam, 1, H, W], ``ids`` [n_cam, H, W] int32 (index within the
    camera, -1 = nothing) and ``mask`` [n_cam, 1, H, W] uint8 -- copies of the winner's values, bit for bit."""
    dev = depth.device
    off, n_cam, n_layers, h, w = _scene_layers(layer_off, depth)
    assert rgb.shape == (n_layers, 3, h, w) and rgb.dtype == torch.float32 and rgb.device == dev, "layer rgb: [L, 3, H, W] float32"
    assert nrm is None or (nrm.shape == (n_layers, 3, h, w) and nrm.dtype == torch.float32 and nrm.device == dev), "layer normals: [L, 3, H, W] float32"
    rgb, depth = rgb.contiguous(), depth.contiguous()
    nrm = None if nrm is None else nrm.contiguous()
    out = {"rgb": torch.empty((n_cam, 3, h, w), dtype=torch.float32, device=dev),
           "normals": torch.empty((n_cam, 3, h, w), dtype=torch.float32, device=dev) if nrm is not None else None,
           "depth": torch.empty((n_cam, 1, h, w), dtype=torch.float32, device=dev),
           "ids": torch.empty((n_cam, h, w), dtype=torch.int32, device=dev),
           "mask": torch.empty((n_cam, 1, h, w), dtype=torch.uint8, device=dev)}
    with torch.cuda.device(dev):
        check(lib().hp_scene_compose(n_cam, ptr(off), n_layers, h, w, ptr(rgb), ptr(nrm), ptr(depth), ptr(out["rgb"]), ptr(out["normals"]),
                                     ptr(out["depth"]), ptr(out["ids"]), ptr(out["mask"]), stream_ptr(dev)), "hp_scene_compose")
    return out


def scene_visibility(layer_off, depth: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """``hp_scene_visibility``: int32 [L, 10] (``SCENE_VIS_COLUMNS``) -- pixel counts of every layer alone and as visible in the
    composed ``ids`` [n_cam, H, W], with the two inclusive bounding boxes (-1 where the count is 0)."""
    dev = depth.device
    off, n_cam, n_layers, h, w = _scene_layers(layer_off, depth)
    assert ids.shape == (n_cam, h, w) and ids.dtype == torch.int32 and ids.device == dev, "ids: [n_cam, H, W] int32"
    table = torch.empty((n_layers, SCENE_VIS_FIELDS), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_scene_visibility(n_cam, ptr(off), n_layers, h, w, ptr(depth.contiguous()), ptr(ids.contiguous()), ptr(table),
                                        stream_ptr(dev)), "hp_scene_visibility")
    return table


def _u8_frames(t: torch.Tensor, what: str) -> torch.Tensor:
    assert t.dim() == 4 and t.shape[-1] == 3 and t.dtype == torch.uint8 and t.is_cuda, f"{what}: [n, H, W, 3] uint8 on the device"
    return t.contiguous()


def scene_contour(frame: torch.Tensor, mask: Optional[torch.Tensor] = None, ids: Optional[torch.Tensor] = None, per_object: bool = False,
                  color: Tuple[int, int, int] = (0, 255, 0), dilate_iterations: int = 1, return_edge: bool = True):
    """``hp_scene_contour``: a copy of ``frame`` [n, H, W, 3] uint8 with the outline of ``mask`` ([n, H, W] or [n, 1, H, W]
    uint8 / bool) or of ``ids`` [n, H, W] int32 (``per_object``: between objects too) painted in ``color``, and the edge map
    [n, H, W] uint8 (0 / 255).  The outline's definition is in the header."""
    frame = _u8_frames(frame, "frame")
    n, h, w, _ = frame.shape
    dev = frame.device
    assert (mask is None) != (ids is None), "scene_contour: exactly one of mask and ids"
    if mask is not None:
        assert mask.numel() == n * h * w and mask.dtype in (torch.uint8, torch.bool) and mask.device == dev, "mask: [n, H, W] uint8 / bool"
        mask = mask.contiguous().view(torch.uint8)
    else:
        assert ids.shape == (n, h, w) and ids.dtype == torch.int32 and ids.device == dev, "ids: [n, H, W] int32"
        ids = ids.contiguous()
    out = torch.empty_like(frame)
    edge = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if return_edge else None
    r, g, b = (int(c) for c in color)
    with torch.cuda.device(dev):
        check(lib().hp_scene_contour(n, h, w, ptr(frame), ptr(mask), ptr(ids), 1 if per_object else 0, r, g, b, int(dilate_iterations),
                                     ptr(out), ptr(edge), stream_ptr(dev)), "hp_scene_contour")
    return out, edge


def scene_overlay(rgb_input: torch.Tensor, rgb_rendered: torch.Tensor, lut_render: torch.Tensor, lut_input: torch.Tensor,
                  mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hp_scene_overlay`` on [n, H, W, 3] uint8 frames with the two 256-entry uint8 tables of
    ``happypose_amd.scene.overlay_tables``; ``mask`` ([n, H, W] / [n, 1, H, W] uint8 / bool) replaces "any render channel > 0"."""
    rgb_input, rgb_rendered = _u8_frames(rgb_input, "rgb_input"), _u8_frames(rgb_rendered, "rgb_rendered")
    assert rgb_input.shape == rgb_rendered.shape and rgb_input.device == rgb_rendered.device
    n, h, w, _ = rgb_input.shape
    dev = rgb_input.device
    for t in (lut_render, lut_input):
        assert t.shape == (256,) and t.dtype == torch.uint8, "overlay tables: 256 uint8 entries"
    lut_render, lut_input = lut_render.to(dev).contiguous(), lut_input.to(dev).contiguous()
    if mask is not None:
        assert mask.numel() == n * h * w and mask.dtype in (torch.uint8, torch.bool) and mask.device == dev, "mask: [n, H, W] uint8 / bool"
        mask = mask.contiguous().view(torch.uint8)
    out = torch.empty_like(rgb_input)
    with torch.cuda.device(dev):
        check(lib().hp_scene_overlay(n, h, w, ptr(rgb_input), ptr(rgb_rendered), ptr(mask), ptr(lut_render), ptr(lut_input), ptr(out),
                                     stream_ptr(dev)), "hp_scene_overlay")
    return out


# ------------------------------------------------------------------------------------------ visible-surface discrepancy (vsd.hip)
VSD_MAX_TAUS = 16      # HP_VSD_MAX_TAUS
VSD_COUNT_FIELDS = 4   # HP_VSD_COUNT_FIELDS
VSD_COUNT_COLUMNS = ("n_union", "n_inter", "n_visib_est", "n_visib_gt")


def vsd_workspace_bytes(n_rows: int, h: int, w: int) -> int:
    """``hp_vsd_workspace_bytes``: rows x blocks of 4096 pixels x 80 bytes."""
    n = int(lib().hp_vsd_workspace_bytes(int(n_rows), int(h), int(w)))
    assert n >= 0, "vsd_workspace_bytes: n_rows >= 0, h and w positive, h * w < 2^31"
    return n


def vsd_tables(est_layer, gt_layer, frame, diameter, depth_test: torch.Tensor, depth_layers: torch.Tensor, K: torch.Tensor,
               delta: float, taus, normalized_by_diameter: bool = True) -> Dict[str, torch.Tensor]:
    """``hp_vsd``: row ``r`` compares the depth renders ``depth_layers[est_layer[r]]`` and ``depth_layers[gt_layer[r]]``
    ([L, H, W] or the rasteriser's [L, 1, H, W], metres, 0 = background) with the measured ``depth_test[frame[r]]`` [F, H, W]
    under ``K[frame[r]]`` [F, 3, 3]; ``diameter`` [n] in metres.  Returns ``errors`` [n, n_tau] float32 (BOP's VSD, BOP19
    visibility, step cost), ``cost`` [n, n_tau] int32 (pixels of the intersection at or past every tau) and ``counts``
    [n, 4] int32 (``VSD_COUNT_COLUMNS``).  One launch pair, no synchronisation."""
    assert depth_layers.is_cuda and depth_layers.dtype == torch.float32, "depth_layers: float32 on the device"
    dev = depth_layers.device
    if depth_layers.dim() == 4:
        assert depth_layers.shape[1] == 1, "depth_layers: [L, H, W] or [L, 1, H, W]"
        depth_layers = depth_layers[:, 0]
    if depth_test.dim() == 4:
        assert depth_test.shape[1] == 1, "depth_test: [F, H, W] or [F, 1, H, W]"
        depth_test = depth_test[:, 0]
    assert depth_layers.dim() == 3 and depth_test.dim() == 3 and depth_test.shape[1:] == depth_layers.shape[1:], "depth_test [F, H, W] and depth_layers [L, H, W]"
    n_layers, h, w = depth_layers.shape
    n_frames = depth_test.shape[0]
    assert K.shape == (n_frames, 3, 3), "vsd: one K per frame"
    taus = np.ascontiguousarray(np.asarray(taus, dtype=np.float32).reshape(-1))
    n_tau = len(taus)
    assert 1 <= n_tau <= VSD_MAX_TAUS, f"vsd: 1 to {VSD_MAX_TAUS} taus"
    n = len(est_layer)
    assert len(gt_layer) == len(frame) == len(diameter) == n
    _assert_ids(est_layer, n_layers, "vsd: est_layer")
    _assert_ids(gt_layer, n_layers, "vsd: gt_layer")
    _assert_ids(frame, n_frames, "vsd: frame")
    est_layer, gt_layer, frame = (_i32(a, dev) for a in (est_layer, gt_layer, frame))
    diameter = _f32(torch.as_tensor(diameter), dev)
    depth_test, depth_layers, K = _f32(depth_test, dev), depth_layers.contiguous(), _f32(K, dev)
    out = {"errors": torch.empty((n, n_tau), dtype=torch.float32, device=dev),
           "cost": torch.empty((n, n_tau), dtype=torch.int32, device=dev),
           "counts": torch.empty((n, VSD_COUNT_FIELDS), dtype=torch.int32, device=dev)}
    if n == 0:
        return out
    nbytes = vsd_workspace_bytes(n, h, w)
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_vsd(n, ptr(est_layer), ptr(gt_layer), ptr(frame), ptr(diameter), ptr(depth_test), n_frames, ptr(depth_layers),
                           n_layers, ptr(K), h, w, float(delta), n_tau, _np_ptr(taus), 1 if normalized_by_diameter else 0,
                           ptr(out["counts"]), ptr(out["cost"]), ptr(out["errors"]), ptr(ws), nbytes, stream_ptr(dev)), "hp_vsd")
    return out


# ------------------------------------------------------------------------------------ detection and mask scoring (det_eval.hip)
MASK_MAX_PIXELS = 1 << 24  # hp_mask_pack: every pixel count is exact in float32


def mask_pack_words(h: int, w: int) -> int:
    """``hp_mask_pack_words``: ``ceil(h * w / 64)``."""
    n = int(lib().hp_mask_pack_words(int(h), int(w)))
    assert n >= 0, f"mask_pack_words: h and w positive, h * w <= {MASK_MAX_PIXELS}"
    return n


def mask_pack(masks: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``hp_mask_pack``: ``masks`` [n, H, W] bool / uint8 on the device (non-zero = set) -> ``words`` [n, ceil(H W / 64)] int64
    (the uint64 words bit for bit: bit ``i`` of word ``k`` is pixel ``64 k + i``, the tail bits of the last word are 0) and ``area``
    [n] int32.  A view whose planes are dense is packed where it lies, whatever its base address."""
    assert masks.dim() == 3 and masks.dtype in (torch.bool, torch.uint8) and masks.is_cuda, "masks: [n, H, W] bool / uint8 on the device"
    n, h, w = masks.shape
    dev = masks.device
    masks = masks.contiguous().view(torch.uint8)
    words = torch.empty((n, mask_pack_words(h, w)), dtype=torch.int64, device=dev)
    area = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_mask_pack(n, h, w, ptr(masks), ptr(words), ptr(area), stream_ptr(dev)), "hp_mask_pack")
    return words, area


def _packed(p, what: str):
    words, area = p
    assert words.dim() == 2 and words.dtype == torch.int64 and words.is_cuda and words.shape[1] >= 1, f"{what}: words [n, W64] int64 on the device"
    assert area.shape == (words.shape[0],) and area.dtype == torch.int32 and area.device == words.device, f"{what}: area [n] int32"
    return words.contiguous(), area.contiguous()


def det_iou(pred_idx, gt_idx, boxes_pred: Optional[torch.Tensor] = None, boxes_gt: Optional[torch.Tensor] = None,
            packed_pred=None, packed_gt=None) -> Dict[str, Optional[torch.Tensor]]:
    """``hp_det_iou``: row ``r`` compares prediction ``pred_idx[r]`` with ground truth ``gt_idx[r]``.  ``boxes_*`` [n, 4] xyxy
    give ``box_iou`` [n_rows] float32 (torchvision's ``box_iou``; 0 / 0 is NaN); ``packed_*`` = ``mask_pack(...)`` give ``inter`` /
    ``union`` [n_rows] int32 and ``mask_iou`` [n_rows] float32 (0 where the union is empty).  The outputs of a family that was
    not given are None.  One launch per family, no synchronisation."""
    assert (boxes_pred is None) == (boxes_gt is None) and (packed_pred is None) == (packed_gt is None), "det_iou: both sides of a family"
    assert boxes_pred is not None or packed_pred is not None, "det_iou: boxes, packed masks or both"
    n = len(pred_idx)
    assert len(gt_idx) == n
    dev = boxes_pred.device if boxes_pred is not None else packed_pred[0].device
    out: Dict[str, Optional[torch.Tensor]] = {"box_iou": None, "inter": None, "union": None, "mask_iou": None}
    n_pred = n_gt = None
    wp = ap = wg = ag = None
    w64 = 0
    if boxes_pred is not None:
        assert boxes_pred.dim() == 2 and boxes_pred.shape[1] == 4 and boxes_gt.dim() == 2 and boxes_gt.shape[1] == 4, "boxes: [n, 4] xyxy"
        assert boxes_pred.is_cuda and boxes_gt.device == dev, "boxes: on one device"
        boxes_pred, boxes_gt = _f32(boxes_pred, dev), _f32(boxes_gt, dev)
        n_pred, n_gt = boxes_pred.shape[0], boxes_gt.shape[0]
        out["box_iou"] = torch.empty((n,), dtype=torch.float32, device=dev)
    if packed_pred is not None:
        (wp, ap), (wg, ag) = _packed(packed_pred, "packed_pred"), _packed(packed_gt, "packed_gt")
        assert wg.device == wp.device == dev and wp.shape[1] == wg.shape[1], "packed masks: one device, one plane size"
        assert n_pred in (None, wp.shape[0]) and n_gt in (None, wg.shape[0]), "det_iou: boxes and masks describe the same instances"
        n_pred, n_gt, w64 = wp.shape[0], wg.shape[0], wp.shape[1]
        out["inter"] = torch.empty((n,), dtype=torch.int32, device=dev)
        out["union"] = torch.empty((n,), dtype=torch.int32, device=dev)
        out["mask_iou"] = torch.empty((n,), dtype=torch.float32, device=dev)
    _assert_ids(pred_idx, n_pred, "det_iou: pred_idx")
    _assert_ids(gt_idx, n_gt, "det_iou: gt_idx")
    if n == 0:
        return out
    pred_idx, gt_idx = _i32(pred_idx, dev), _i32(gt_idx, dev)
    with torch.cuda.device(dev):
        check(lib().hp_det_iou(n, ptr(pred_idx), ptr(gt_idx), n_pred, n_gt, ptr(boxes_pred), ptr(boxes_gt), ptr(wp), ptr(ap), ptr(wg), ptr(ag),
                               w64, ptr(out["box_iou"]), ptr(out["inter"]), ptr(out["union"]), ptr(out["mask_iou"]), stream_ptr(dev)),
              "hp_det_iou")
    return out


def coco_thresholds(thresholds) -> np.ndarray:
    """The float32 thresholds ``hp_det_match`` compares with: ``float32(min(t, 1 - 1e-10))``, pycocotools' cap."""
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    return np.ascontiguousarray(np.minimum(t, 1 - 1e-10).astype(np.float32))


def det_match(iou: torch.Tensor, n_det, n_gt, gt_ignore, thresholds) -> Dict[str, torch.Tensor]:
    """``hp_det_match``: COCO's greedy matching of every group at every threshold.  ``iou`` [sum n_det * n_gt] float32 on the
    device holds the groups' dense detection-major matrices one after the other; ``n_det`` / ``n_gt`` [n_groups] are host
    columns; ``gt_ignore`` [sum n_gt] bool.  Detections must already be in descending-score order and ground truths with the
    non-ignored ones first (``evaluation.plan_detection_rows``).  Returns ``det_match`` [n_thr, sum n_det] int32 (ground truth's
    position in its group or -1), ``det_ignore`` [n_thr, sum n_det] bool and ``gt_match`` [n_thr, sum n_gt] int32."""
    assert iou.dim() == 1 and iou.dtype == torch.float32 and iou.is_cuda, "iou: [rows] float32 on the device"
    dev = iou.device
    n_det, n_gt = np.asarray(n_det, dtype=np.int64).reshape(-1), np.asarray(n_gt, dtype=np.int64).reshape(-1)
    assert len(n_det) == len(n_gt) and (n_det >= 0).all() and (n_gt >= 0).all(), "det_match: one non-negative n_det and n_gt per group"
    rows = n_det * n_gt
    total_rows, total_dets, total_gts = int(rows.sum()), int(n_det.sum()), int(n_gt.sum())
    assert iou.numel() == total_rows, f"det_match: iou has {iou.numel()} entries, the groups need {total_rows}"
    assert max(total_rows, total_dets, total_gts) < 2 ** 31, "det_match: tables of 2^31 entries or more"
    gt_ignore = torch.as_tensor(np.asarray(gt_ignore.cpu() if isinstance(gt_ignore, torch.Tensor) else gt_ignore).astype(np.uint8).reshape(-1))
    assert gt_ignore.numel() == total_gts, "det_match: one gt_ignore flag per ground truth"
    thr = coco_thresholds(thresholds)
    n_thr, n_groups = len(thr), len(n_det)
    out = {"det_match": torch.empty((n_thr, total_dets), dtype=torch.int32, device=dev),
           "det_ignore": torch.empty((n_thr, total_dets), dtype=torch.uint8, device=dev),
           "gt_match": torch.empty((n_thr, total_gts), dtype=torch.int32, device=dev)}
    if n_groups and n_thr:
        start = lambda c: np.concatenate([[0], np.cumsum(c)[:-1]])  # noqa: E731
        tables = [_i32(a, dev) for a in (n_det, n_gt, start(rows), start(n_det), start(n_gt))]
        gt_ignore, thr_d = gt_ignore.to(dev), torch.as_tensor(thr).to(dev)
        with torch.cuda.device(dev):
            check(lib().hp_det_match(n_groups, *[ptr(t) for t in tables], ptr(iou.contiguous()), total_rows, total_dets, total_gts,
                                     ptr(gt_ignore), ptr(thr_d), n_thr, ptr(out["det_match"]), ptr(out["det_ignore"]), ptr(out["gt_match"]),
                                     stream_ptr(dev)), "hp_det_match")
    out["det_ignore"] = out["det_ignore"].view(torch.bool)
    return out


# ------------------------------------------------------------------------------------------- mesh resampling (mesh_sample.hip)
MESH_SAMPLE_SCAN_CHUNK = 1024  # faces per step of the area scan (csrc/mesh_sample.hip: kScanChunk)


def mesh_sample_workspace_bytes(n_obj: int, total_faces: int) -> int:
    """``hp_mesh_sample_workspace_bytes``: ``8 (n_obj + total_faces)``."""
    n = int(lib().hp_mesh_sample_workspace_bytes(int(n_obj), int(total_faces)))
    assert n >= 0, "mesh_sample_workspace_bytes: n_obj >= 0 and 0 <= total_faces < 2^31"
    return n


def mesh_sample_surface_tables(vertices: torch.Tensor, faces: torch.Tensor, vert_offset: torch.Tensor, face_offset: torch.Tensor,
                               n_samples: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """``hp_mesh_sample_surface`` on explicit device tables: ``vertices [V_tot, 3]`` float32, ``faces [F_tot, 3]`` int32 (ids local
    to their object), ``vert_offset`` / ``face_offset [n_obj + 1]`` int32.  Nothing is checked here: the kernels guard every
    object (NaN points, ``face_id`` -1).  Returns ``points [n_obj, n_samples, 3]`` float32, ``face_id [n_obj, n_samples]`` int32
    and ``area [n_obj]`` float64."""
    dev = vertices.device
    assert vertices.is_cuda and vertices.dtype == torch.float32 and vertices.dim() == 2 and vertices.shape[1] == 3, "vertices: [V, 3] float32 on the device"
    assert faces.device == dev and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3, "faces: [F, 3] int32 on the device"
    n_obj = vert_offset.numel() - 1
    assert n_obj >= 0 and face_offset.numel() == n_obj + 1, "offsets: [n_obj + 1] each"
    assert vert_offset.dtype == torch.int32 and face_offset.dtype == torch.int32 and vert_offset.device == dev and face_offset.device == dev
    n_samples = int(n_samples)
    assert n_samples >= 0, "mesh_sample_surface: negative n_samples"
    out = {"points": torch.empty((n_obj, n_samples, 3), dtype=torch.float32, device=dev),
           "face_id": torch.empty((n_obj, n_samples), dtype=torch.int32, device=dev),
           "area": torch.empty((n_obj,), dtype=torch.float64, device=dev)}
    if n_obj == 0 or n_samples == 0:
        out["area"].fill_(float("nan"))  # nothing is launched: no area is computed
        return out
    nbytes = mesh_sample_workspace_bytes(n_obj, faces.shape[0])
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    vertices, faces, vert_offset, face_offset = vertices.contiguous(), faces.contiguous(), vert_offset.contiguous(), face_offset.contiguous()
    with torch.cuda.device(dev):
        check(lib().hp_mesh_sample_surface(n_obj, ptr(vertices), ptr(faces), ptr(vert_offset), ptr(face_offset), n_samples,
                                           int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out["points"]), ptr(out["face_id"]), ptr(out["area"]),
                                           ptr(ws), nbytes, stream_ptr(dev)), "hp_mesh_sample_surface")
    return out


def mesh_sample_surface(vertices_list, faces_list, n_samples: int, seed: int = 0, return_face_ids: bool = False,
                        return_areas: bool = False, device="cuda"):
    """``n_samples`` points drawn uniformly from the surface of each mesh (``include/happypose_amd.h``, mesh surface resampling):
    ``vertices_list[o] [V_o, 3]``, ``faces_list[o] [F_o, 3]``.  Object ``o`` of the random stream is the position in the lists.
    The face indices are range-checked here, on the host, before any launch.  Returns ``points [n_obj, n_samples, 3]`` float32 on
    the device, followed on request by ``face_ids [n_obj, n_samples]`` int32 and ``areas [n_obj]`` float64.  A mesh without faces
    or without area gives NaN points and face id -1."""
    assert len(vertices_list) == len(faces_list), "mesh_sample_surface: one face table per vertex table"
    verts = [np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1, 3)) for v in vertices_list]
    faces = [np.ascontiguousarray(np.asarray(f).reshape(-1, 3)) for f in faces_list]
    for o, (v, f) in enumerate(zip(verts, faces)):
        if f.size:
            lo, hi = int(f.min()), int(f.max())
            assert 0 <= lo and hi < len(v), f"mesh_sample_surface: faces of object {o} in [{lo}, {hi}] index {len(v)} vertices"
    voff = np.concatenate([[0], np.cumsum([len(v) for v in verts])]).astype(np.int64)
    foff = np.concatenate([[0], np.cumsum([len(f) for f in faces])]).astype(np.int64)
    assert voff[-1] < 2 ** 31 and foff[-1] < 2 ** 31, "mesh_sample_surface: tables of 2^31 rows or more"
    dev = torch.device(device)
    # one unused row closes each table, so that neither is ever empty (the offsets do not reach it)
    v_all = np.concatenate(verts + [np.zeros((1, 3), np.float32)])
    f_all = np.concatenate([f.astype(np.int32) for f in faces] + [np.zeros((1, 3), np.int32)])
    out = mesh_sample_surface_tables(torch.as_tensor(v_all).to(dev), torch.as_tensor(f_all).to(dev), _i32(voff, dev), _i32(foff, dev),
                                     n_samples, seed)
    res = [out["points"]] + ([out["face_id"]] if return_face_ids else []) + ([out["area"]] if return_areas else [])
    return res[0] if len(res) == 1 else tuple(res)


def farthest_point_ids(points: torch.Tensor, counts, k: int) -> torch.Tensor:
    """``hp_teaser_fps``: farthest-point sampling of ``points [n, n_max, 3]`` float32 on the device, set ``i`` holding
    ``counts[i]`` points.  Starts at index 0, takes the point farthest from the chosen set, ties to the lowest index.  Returns
    ``[n, k]`` int32: ``min(k, counts[i])`` indices in selection order, then -1."""
    assert points.dim() == 3 and points.shape[2] == 3 and points.is_cuda, "points: [n, n_max, 3] on the device"
    dev = points.device
    n, n_max, k = points.shape[0], points.shape[1], int(k)
    assert n_max >= 1 and k >= 1, "farthest_point_ids: n_max >= 1 and k >= 1"
    counts = _i32(counts, dev)
    assert counts.shape == (n,), "farthest_point_ids: one count per set"
    points = _f32(points, dev)
    idx = torch.empty((n, k), dtype=torch.int32, device=dev)
    if n == 0:
        return idx
    scratch = torch.empty((n, n_max), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_teaser_fps(n, n_max, ptr(points), ptr(counts), k, ptr(scratch), ptr(idx), stream_ptr(dev)), "hp_teaser_fps")
    return idx


# ------------------------------------------------------------------------------------ training-image augmentations (augment.hip)
AUG_OPS = {"brightness": 0, "color": 1, "contrast": 2, "sharpness": 3}  # HP_AUG_OP_*


def _aug_frames(t: torch.Tensor, what: str, dtype, channels: bool) -> torch.Tensor:
    """A dense batch on the device: ``[B, H, W, 3]`` uint8 or ``[B, H, W]`` of ``dtype``.  A CPU tensor raises ValueError: there is
    no host implementation and none is substituted."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{what}: a tensor on the device is required (no CPU implementation)")
    if t.dtype != dtype or t.dim() != (4 if channels else 3) or (channels and t.shape[-1] != 3) or not t.is_contiguous():
        raise ValueError(f"{what}: dense {'[B, H, W, 3]' if channels else '[B, H, W]'} {dtype} expected, got {tuple(t.shape)} {t.dtype}")
    if t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError(f"{what}: empty frames")
    return t


def _aug_param(v, n: int, dtype, dev, what: str) -> torch.Tensor:
    """A per-image parameter: a scalar or ``n`` values, as a device array of ``dtype``.  The caller holds the result in a local
    until the call is enqueued: a temporary would hand its block back to the allocator, and the next parameter would land on it."""
    t = torch.as_tensor(v).to(dtype).reshape(-1)
    if t.numel() == 1 and n != 1:
        t = t.expand(n)
    if t.numel() != n:
        raise ValueError(f"{what}: one value per image ({n}), got {t.numel()}")
    return t.contiguous().to(dev)


def _aug_apply(apply, n: int, dev) -> torch.Tensor:
    return _aug_param(True if apply is None else apply, n, torch.bool, dev, "apply").view(torch.uint8)


def _aug_out(x: torch.Tensor, out: Optional[torch.Tensor], in_place_ok: bool, what: str) -> torch.Tensor:
    if out is None:
        return torch.empty_like(x)
    if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise ValueError(f"{what}: out must match the input")
    if not in_place_ok and out.data_ptr() == x.data_ptr():
        raise ValueError(f"{what}: reads a neighbourhood, out must not alias the input")
    return out


def aug_workspace(B: int, h: int, w: int, max_ellipses: int, dev) -> Tuple[torch.Tensor, int]:
    """``hp_aug_workspace_bytes`` and a buffer of that size (8-byte aligned)."""
    n = int(lib().hp_aug_workspace_bytes(int(B), int(h), int(w), int(max_ellipses)))
    if n < 0:
        raise ValueError("augmentations: at most 65535 frames of at most 2^28 pixels")
    return torch.empty(max(n // 8, 1), dtype=torch.int64, device=dev), n


def aug_rgb_enhance(rgb: torch.Tensor, op, factor, apply=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hp_aug_rgb_enhance``: Pillow's ``ImageEnhance`` per image.  ``op`` names (``AUG_OPS``) or codes and ``factor``: a scalar or
    one per image; ``apply [B]`` bool (default all).  Not in place."""
    rgb = _aug_frames(rgb, "aug_rgb_enhance: rgb", torch.uint8, True)
    B, h, w, dev = rgb.shape[0], rgb.shape[1], rgb.shape[2], rgb.device
    out = _aug_out(rgb, out, False, "aug_rgb_enhance")
    if B == 0:
        return out
    codes = [op] if isinstance(op, (str, int)) else list(op)
    codes = [AUG_OPS[c] if isinstance(c, str) else int(c) for c in codes]
    ws, nbytes = aug_workspace(B, h, w, 0, dev)
    _p0 = _aug_param(codes, B, torch.int32, dev, "op")
    _p1 = _aug_param(factor, B, torch.float32, dev, "factor")
    _p2 = _aug_apply(apply, B, dev)
    with torch.cuda.device(dev):
        check(lib().hp_aug_rgb_enhance(B, h, w, ptr(rgb), ptr(_p0),
                                       ptr(_p1), ptr(_p2), ptr(out),
                                       ptr(ws), nbytes, stream_ptr(dev)), "hp_aug_rgb_enhance")
    return out


def aug_blur_params(k) -> Tuple[int, int, int]:
    """``(r, ww, fw)`` of the box filter whose three passes stand for Pillow's Gaussian blur of radius ``k``: float32, as the
    header writes it."""
    f32 = np.float32
    sigma2 = f32(f32(f32(k) * f32(k)) / f32(3))
    L = f32(np.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(np.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * sigma2)))
    a = f32(a / f32(f32(6) * f32(sigma2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    r_f = f32(l + a)
    r = int(r_f)
    ww = int(f32(f32(1 << 24) / f32(f32(r_f * f32(2)) + f32(1))))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def aug_rgb_blur(rgb: torch.Tensor, radius, apply=None, out: Optional[torch.Tensor] = None, force_general: bool = False) -> torch.Tensor:
    """``hp_aug_rgb_blur``: Pillow's ``GaussianBlur(k)`` with ``k = radius`` (a positive number, scalar or one per image).
    ``force_general`` takes the one-launch-per-pass path whatever the frame size (same bytes).  Not in place."""
    rgb = _aug_frames(rgb, "aug_rgb_blur: rgb", torch.uint8, True)
    B, h, w, dev = rgb.shape[0], rgb.shape[1], rgb.shape[2], rgb.device
    out = _aug_out(rgb, out, False, "aug_rgb_blur")
    if B == 0:
        return out
    ks = np.broadcast_to(np.asarray(radius, np.float64).reshape(-1), (B,)) if np.size(radius) in (1, B) else None
    if ks is None or not (ks > 0).all():
        raise ValueError("aug_rgb_blur: one positive radius per image")
    par = np.array([aug_blur_params(k) for k in ks], np.int64).reshape(B, 3)
    ws, nbytes = aug_workspace(B, h, w, 0, dev)
    _p0 = _aug_param(par[:, 0], B, torch.int32, dev, "radius")
    _p1 = _aug_param(par[:, 1], B, torch.int32, dev, "ww")
    _p2 = _aug_param(par[:, 2], B, torch.int32, dev, "fw")
    _p3 = _aug_apply(apply, B, dev)
    with torch.cuda.device(dev):
        check(lib().hp_aug_rgb_blur(B, h, w, ptr(rgb), ptr(_p0),
                                    ptr(_p1), ptr(_p2),
                                    ptr(_p3), ptr(out), int(bool(force_general)), ptr(ws), nbytes, stream_ptr(dev)),
              "hp_aug_rgb_blur")
    return out


def _aug_seg(seg: torch.Tensor, like: torch.Tensor, what: str) -> torch.Tensor:
    seg = _aug_frames(seg, what, torch.int32, False)
    if seg.shape != like.shape[:3] or seg.device != like.device:
        raise ValueError(f"{what}: [B, H, W] of the frames")
    return seg


def aug_replace_background(rgb: torch.Tensor, segmentation: torch.Tensor, background: torch.Tensor, apply=None,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hp_aug_replace_background``: ``background`` where ``segmentation == 0``.  May run in place (``out=rgb``)."""
    rgb = _aug_frames(rgb, "aug_replace_background: rgb", torch.uint8, True)
    background = _aug_frames(background, "aug_replace_background: background", torch.uint8, True)
    seg = _aug_seg(segmentation, rgb, "aug_replace_background: segmentation")
    if background.shape != rgb.shape or background.device != rgb.device:
        raise ValueError("aug_replace_background: background must already have the frames' size")
    B, h, w, dev = rgb.shape[0], rgb.shape[1], rgb.shape[2], rgb.device
    out = _aug_out(rgb, out, True, "aug_replace_background")
    if B:
        _p0 = _aug_apply(apply, B, dev)
        with torch.cuda.device(dev):
            check(lib().hp_aug_replace_background(B, h, w, ptr(rgb), ptr(seg), ptr(background), ptr(_p0), ptr(out),
                                                  stream_ptr(dev)), "hp_aug_replace_background")
    return out


def _aug_depth(depth: torch.Tensor, out, in_place_ok: bool, what: str):
    depth = _aug_frames(depth, f"{what}: depth", torch.float32, False)
    return depth, _aug_out(depth, out, in_place_ok, what), depth.shape[0], depth.shape[1], depth.shape[2], depth.device


def aug_depth_noise(depth: torch.Tensor, std, seed: int, grid=None, apply=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hp_aug_depth_noise``: Gaussian noise of ``std`` on the valid pixels; with ``grid = (grid_h, grid_w)`` (scalars or one per
    image) the noise is drawn on that grid and upsampled bicubically.  May run in place."""
    depth, out, B, h, w, dev = _aug_depth(depth, out, True, "aug_depth_noise")
    if B == 0:
        return out
    gh = gw = ws = None
    nbytes = 0
    if grid is not None:
        gh, gw = _aug_param(grid[0], B, torch.int32, dev, "grid_h"), _aug_param(grid[1], B, torch.int32, dev, "grid_w")
        ws, nbytes = aug_workspace(B, h, w, 0, dev)
    _p0 = _aug_param(std, B, torch.float32, dev, "std")
    _p1 = _aug_apply(apply, B, dev)
    with torch.cuda.device(dev):
        check(lib().hp_aug_depth_noise(B, h, w, ptr(depth), ptr(_p0), int(grid is not None), ptr(gh),
                                       ptr(gw), ptr(_p1), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out), ptr(ws), nbytes,
                                       stream_ptr(dev)), "hp_aug_depth_noise")
    return out


def aug_depth_missing(depth: torch.Tensor, fraction, seed: int, apply=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hp_aug_depth_missing``: exactly ``int(fraction * n_valid)`` of an image's valid pixels become 0.  May run in place."""
    depth, out, B, h, w, dev = _aug_depth(depth, out, True, "aug_depth_missing")
    if B == 0:
        return out
    ws, nbytes = aug_workspace(B, h, w, 0, dev)
    _p0 = _aug_param(fraction, B, torch.float64, dev, "fraction")
    _p1 = _aug_apply(apply, B, dev)
    with torch.cuda.device(dev):
        check(lib().hp_aug_depth_missing(B, h, w, ptr(depth), ptr(_p0),
                                         ptr(_p1), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out), ptr(ws), nbytes,
                                         stream_ptr(dev)), "hp_aug_depth_missing")
    return out


def aug_depth_ellipses(depth: torch.Tensor, table, count, noise: bool, apply=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hp_aug_depth_ellipses``: ``table [B, E, 5]`` = (u, rx, ry, angle_deg, value), ``count [B]``.  ``noise=False`` zeroes the
    pixels inside, ``noise=True`` adds the last covering ellipse's value to the valid ones.  May run in place."""
    depth, out, B, h, w, dev = _aug_depth(depth, out, True, "aug_depth_ellipses")
    if B == 0:
        return out
    table = torch.as_tensor(table).to(torch.float32)
    if table.dim() != 3 or table.shape[0] != B or table.shape[2] != 5:
        raise ValueError("aug_depth_ellipses: table [B, E, 5]")
    E = table.shape[1]
    table = table.contiguous().to(dev) if E else None
    ws, nbytes = aug_workspace(B, h, w, E, dev)
    _p0 = _aug_param(count, B, torch.int32, dev, "count")
    _p1 = _aug_apply(apply, B, dev)
    with torch.cuda.device(dev):
        check(lib().hp_aug_depth_ellipses(B, h, w, ptr(depth), ptr(table), ptr(_p0), E,
                                          int(bool(noise)), ptr(_p1), ptr(out), ptr(ws), nbytes, stream_ptr(dev)),
              "hp_aug_depth_ellipses")
    return out


def aug_depth_blur(depth: torch.Tensor, ksize, apply=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hp_aug_depth_blur``: the ``k x k`` box filter, ``k = ksize`` (scalar or one per image, each >= 1).  A frame side shorter
    than the largest ``k`` raises AssertionError (the library's argument error) and launches nothing.  Not in place."""
    depth, out, B, h, w, dev = _aug_depth(depth, out, False, "aug_depth_blur")
    if B == 0:
        return out
    ks = np.asarray(ksize, np.int64).reshape(-1)
    if ks.size not in (1, B) or (ks < 1).any():
        raise ValueError("aug_depth_blur: one k >= 1 per image")
    _p0 = _aug_param(ks, B, torch.int32, dev, "ksize")
    _p1 = _aug_apply(apply, B, dev)
    with torch.cuda.device(dev):
        check(lib().hp_aug_depth_blur(B, h, w, ptr(depth), ptr(_p0), int(ks.max()),
                                      ptr(_p1), ptr(out), stream_ptr(dev)), "hp_aug_depth_blur")
    return out


def aug_depth_mask(depth: torch.Tensor, segmentation: Optional[torch.Tensor] = None, apply=None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hp_aug_depth_mask``: all zeros without ``segmentation``, else zero where ``segmentation == 0``.  May run in place."""
    depth, out, B, h, w, dev = _aug_depth(depth, out, True, "aug_depth_mask")
    seg = None if segmentation is None else _aug_seg(segmentation, depth, "aug_depth_mask: segmentation")
    if B:
        _p0 = _aug_apply(apply, B, dev)
        with torch.cuda.device(dev):
            check(lib().hp_aug_depth_mask(B, h, w, ptr(depth), ptr(seg), ptr(_p0), ptr(out), stream_ptr(dev)),
                  "hp_aug_depth_mask")
    return out


# ------------------------------------------------------------------------------------------------- frame geometry (resize.hip)
RESIZE_FILTERS = {"bilinear": 1.0, "bicubic": 2.0}  # the filter's support
RESIZE_PRECISION_BITS = 22
RESIZE_TILE = 256        # output pixels per workgroup of the pass along x (csrc/resize.hip: kTile)
RESIZE_MAX_BAND = 12288  # csrc/resize.hip: kMaxBand
SEG_BOXES_MAX_IDS = 256


def _resize_filter(name: str, x: np.ndarray) -> np.ndarray:
    x = np.abs(x)
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


@functools.lru_cache(maxsize=256)
def _resize_axis(size: int, b0: int, b1: int, out: int, filt: str) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's coefficients of one axis in float64: ``bounds [out, 2]`` = (first source index, count) and the fixed-point
    ``weights [out, ksize]`` (0 beyond the count).  The header writes the formulas out."""
    scale = (b1 - b0) / out
    fscale = max(scale, 1.0)
    support = RESIZE_FILTERS[filt] * fscale
    ksize = int(np.ceil(support)) * 2 + 1
    centre = b0 + (np.arange(out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((centre - support + 0.5).astype(np.int64), 0)  # the cast truncates, as C's
    hi = np.minimum((centre + support + 0.5).astype(np.int64), size)
    n = np.maximum(hi - lo, 0)
    k = np.arange(ksize)
    w = _resize_filter(filt, (k[None, :] + lo[:, None] - centre[:, None] + 0.5) * (1.0 / fscale))
    w = np.where(k[None, :] < n[:, None], w, 0.0)
    total = np.zeros(out)
    for j in range(ksize):  # the window's sum in Pillow's order
        total = total + w[:, j]
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    q = np.trunc(np.where(w < 0, -0.5, 0.5) + w * float(1 << RESIZE_PRECISION_BITS)).astype(np.int32)
    return np.stack([lo, n], axis=1).astype(np.int32), q


@functools.lru_cache(maxsize=256)
def _nearest_axis(size: int, b0: int, b1: int, out: int) -> np.ndarray:
    """Pillow's NEAREST source index per output index: the running double sum, -1 outside ``0 .. size - 1``."""
    step = (b1 - b0) / out
    t = np.add.accumulate(np.concatenate([[b0 + step * 0.5], np.full(out - 1, step)]))  # sequential: t[i + 1] = t[i] + step
    j = np.where(t < 0.0, -1, np.minimum(t, 2.0 ** 31).astype(np.int64))
    return np.where((j >= 0) & (j < size), j, -1).astype(np.int32)


def _resize_geometry(in_size, box, crop) -> Tuple[int, int, int, int, int, int, int, int, int, int]:
    h, w = int(in_size[0]), int(in_size[1])
    cx0, cy0, cx1, cy1 = (0, 0, w, h) if crop is None else (int(v) for v in crop)
    if cx1 <= cx0 or cy1 <= cy0:
        raise ValueError(f"resize: empty crop rectangle {(cx0, cy0, cx1, cy1)}")
    vw, vh = cx1 - cx0, cy1 - cy0
    x0, y0, x1, y1 = (0, 0, vw, vh) if box is None else (int(v) for v in box)
    if not (0 <= x0 < x1 <= vw and 0 <= y0 < y1 <= vh):  # Pillow: "box can't exceed original image size / can't be empty"
        raise ValueError(f"resize: box {(x0, y0, x1, y1)} must be non-empty and inside the {vh} x {vw} image")
    return h, w, cx0, cy0, vw, vh, x0, y0, x1, y1


def resize_tables(in_size, out_size, box=None, filter: str = "bilinear", crop=None) -> Dict[str, object]:
    """The host half of ``hp_resize_rgb`` for ONE geometry: frames of ``in_size = (h, w)`` are cropped to the integer rectangle
    ``crop = (x0, y0, x1, y1)`` as ``PIL.Image.crop`` does (default: the frame; outside the frame is 0), then resized to
    ``out_size = (h, w)`` with ``box`` (integer pixels of the cropped image, default: all of it) and ``filter``.  Returns
    ``xbounds [ow, 2]``, ``xweights [ow, ksize_x]``, ``ybounds``, ``yweights`` (int32, bounds in SOURCE pixels), ``skip_x`` /
    ``skip_y`` (Pillow would skip the pass AND the pass is the identity in source pixels) and ``band_x``."""
    if filter not in RESIZE_FILTERS:
        raise ValueError(f"resize: filter must be one of {sorted(RESIZE_FILTERS)}, got {filter!r}")
    h, w, cx0, cy0, vw, vh, x0, y0, x1, y1 = _resize_geometry(in_size, box, crop)
    oh, ow = int(out_size[0]), int(out_size[1])
    if oh < 1 or ow < 1:
        raise ValueError("resize: empty output")
    xb, xw = _resize_axis(vw, x0, x1, ow, filter)
    yb, yw = _resize_axis(vh, y0, y1, oh, filter)
    xb, yb = xb + np.array([cx0, 0], np.int32), yb + np.array([cy0, 0], np.int32)
    first = np.arange(0, ow, RESIZE_TILE)
    last = np.minimum(first + RESIZE_TILE, ow) - 1
    lo = np.clip(xb[first, 0], 0, w)
    band = int(np.max(np.minimum(np.maximum(xb[last, 0] + xb[last, 1], lo), w) - lo))
    return {"xbounds": xb, "xweights": xw, "ybounds": yb, "yweights": yw, "band_x": max(band, 1),
            "skip_x": ow == vw == w and (cx0, x0, x1) == (0, 0, vw), "skip_y": oh == vh == h and (cy0, y0, y1) == (0, 0, vh)}


def _resize_rects(v, B: int, what: str) -> List[Optional[Tuple[int, ...]]]:
    """``None``, one rectangle or one per image -> ``B`` tuples of 4 integers (or ``None``)."""
    if v is None:
        return [None] * B
    a = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)
    if a.shape not in ((4,), (B, 4)) or not np.issubdtype(a.dtype, np.number) or (a != np.round(a)).any():
        raise ValueError(f"{what}: 4 integers (x0, y0, x1, y1), or [B, 4]")
    a = np.broadcast_to(a.astype(np.int64), (B, 4))
    return [tuple(int(x) for x in r) for r in a]


def _resize_sets(B: int, box, crop, what: str):
    """The distinct (box, crop) pairs of a batch and ``table_of [B]``."""
    pairs = list(zip(_resize_rects(box, B, f"{what}: box"), _resize_rects(crop, B, f"{what}: crop")))
    keys: Dict[tuple, int] = {}
    table_of = np.array([keys.setdefault(p, len(keys)) for p in pairs], np.int32)
    return list(keys), table_of


def _resize_out(x: torch.Tensor, out_size, out: Optional[torch.Tensor], partial: bool, what: str) -> torch.Tensor:
    oh, ow = int(out_size[0]), int(out_size[1])
    if oh < 1 or ow < 1:
        raise ValueError(f"{what}: empty output")
    shape = (x.shape[0], oh, ow) + tuple(x.shape[3:])
    if out is None:  # an image that is not applied keeps what out held: zeros here
        return (torch.zeros if partial else torch.empty)(shape, dtype=x.dtype, device=x.device)
    if tuple(out.shape) != shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise ValueError(f"{what}: out must be {shape} {x.dtype} on the input's device")
    if out.data_ptr() == x.data_ptr():
        raise ValueError(f"{what}: out must not alias the input")
    return out


def _pad_stack(tables: List[np.ndarray]) -> np.ndarray:
    k = max(t.shape[1] for t in tables)
    return np.stack([np.pad(t, ((0, 0), (0, k - t.shape[1]))) for t in tables])


def resize_rgb(rgb: torch.Tensor, out_size, filter: str = "bilinear", box=None, crop=None, apply=None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hp_resize_rgb``: ``PIL.Image.resize(out_size[::-1], filter, box)`` of every frame of ``rgb [B, H, W, 3]`` uint8, after
    ``PIL.Image.crop(crop)`` when ``crop`` is given; byte for byte.  ``box`` / ``crop``: 4 integers ``(x0, y0, x1, y1)`` or one row
    per image (``[B, 4]``); images with the same pair share one table set.  ``apply [B]`` bool (default all): an image that is
    not applied keeps what ``out`` held (zeros without ``out``).  Not in place."""
    rgb = _aug_frames(rgb, "resize_rgb: rgb", torch.uint8, True)
    B, h, w, dev = rgb.shape[0], rgb.shape[1], rgb.shape[2], rgb.device
    if filter not in RESIZE_FILTERS:
        raise ValueError(f"resize_rgb: filter must be one of {sorted(RESIZE_FILTERS)}, got {filter!r}")
    out = _resize_out(rgb, out_size, out, apply is not None, "resize_rgb")
    if B == 0:
        return out
    oh, ow = out.shape[1], out.shape[2]
    sets, table_of = _resize_sets(B, box, crop, "resize_rgb")
    tabs = [resize_tables((h, w), (oh, ow), bx, filter, cr) for bx, cr in sets]
    pass_x, pass_y = not all(t["skip_x"] for t in tabs), not all(t["skip_y"] for t in tabs)
    band = max(t["band_x"] for t in tabs)
    if pass_x and band > RESIZE_MAX_BAND:
        raise ValueError(f"resize_rgb: {RESIZE_TILE} output pixels cover {band} source pixels, more than the {RESIZE_MAX_BAND} one band holds")
    xb = xw = yb = yw = ws = None
    ksx = ksy = nbytes = 0
    if pass_x:
        xb, xw = torch.from_numpy(np.stack([t["xbounds"] for t in tabs])).to(dev), torch.from_numpy(_pad_stack([t["xweights"] for t in tabs])).to(dev)
        ksx = xw.shape[2]
    if pass_y:
        yb, yw = torch.from_numpy(np.stack([t["ybounds"] for t in tabs])).to(dev), torch.from_numpy(_pad_stack([t["yweights"] for t in tabs])).to(dev)
        ksy = yw.shape[2]
    if pass_x and pass_y:
        nbytes = int(lib().hp_resize_workspace_bytes(B, h, ow))
        if nbytes < 0:
            raise ValueError("resize_rgb: at most 65535 frames of at most 2^28 pixels")
        ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
    _p0 = torch.from_numpy(table_of).to(dev)
    _p1 = _aug_apply(apply, B, dev)
    with torch.cuda.device(dev):
        check(lib().hp_resize_rgb(B, h, w, oh, ow, ptr(rgb), len(tabs), ptr(_p0), ptr(xb), ptr(xw), ksx, band if pass_x else 0, ptr(yb), ptr(yw),
                                  ksy, ptr(_p1), ptr(out), ptr(ws), nbytes, stream_ptr(dev)), "hp_resize_rgb")
    return out


def resize_nearest(x: torch.Tensor, out_size, box=None, crop=None, apply=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hp_resize_nearest``: ``PIL.Image.resize(out_size[::-1], NEAREST, box)`` of ``x [B, H, W]`` int32 (mode I) or float32 (mode
    F), after ``PIL.Image.crop(crop)`` when given: a copy of bits.  ``box``, ``crop``, ``apply``, ``out`` as for ``resize_rgb``."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("resize_nearest: a tensor on the device is required (no CPU implementation)")
    if x.dtype not in (torch.int32, torch.float32):
        raise ValueError(f"resize_nearest: int32 or float32 frames expected, got {x.dtype}")
    x = _aug_frames(x, "resize_nearest: x", x.dtype, False)
    B, h, w, dev = x.shape[0], x.shape[1], x.shape[2], x.device
    out = _resize_out(x, out_size, out, apply is not None, "resize_nearest")
    if B == 0:
        return out
    oh, ow = out.shape[1], out.shape[2]
    sets, table_of = _resize_sets(B, box, crop, "resize_nearest")
    xi, yi = [], []
    for bx, cr in sets:
        _, _, cx0, cy0, vw, vh, x0, y0, x1, y1 = _resize_geometry((h, w), bx, cr)
        jx, jy = _nearest_axis(vw, x0, x1, ow), _nearest_axis(vh, y0, y1, oh)
        xi.append(np.where(jx >= 0, jx + cx0, -1))
        yi.append(np.where(jy >= 0, jy + cy0, -1))
    _p0 = torch.from_numpy(table_of).to(dev)
    _p1 = torch.from_numpy(np.stack(xi).astype(np.int32)).to(dev)
    _p2 = torch.from_numpy(np.stack(yi).astype(np.int32)).to(dev)
    _p3 = _aug_apply(apply, B, dev)
    with torch.cuda.device(dev):
        check(lib().hp_resize_nearest(B, h, w, oh, ow, ptr(x), len(sets), ptr(_p0), ptr(_p1), ptr(_p2), ptr(_p3), ptr(out), stream_ptr(dev)),
              "hp_resize_nearest")
    return out


def seg_boxes_table(ids, B: int) -> Tuple[np.ndarray, np.ndarray]:
    """Per-image id lists (or an array ``[B, max_ids]``) -> ``(table [B, max_ids] int32, count [B] int32)``, padded with 0."""
    rows = [np.asarray(r.detach().cpu() if isinstance(r, torch.Tensor) else r, np.int64).reshape(-1) for r in ids]
    if len(rows) != B:
        raise ValueError(f"seg_boxes: one id list per image ({B}), got {len(rows)}")
    count = np.array([r.size for r in rows], np.int32)
    table = np.zeros((B, max(int(count.max()) if B else 0, 1)), np.int32)
    for b, r in enumerate(rows):
        if r.size and (r.min() < -2 ** 31 or r.max() >= 2 ** 31):
            raise ValueError("seg_boxes: ids must fit int32")
        table[b, :r.size] = r
    return table, count


def seg_boxes(segmentation: torch.Tensor, ids, count=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``hp_seg_boxes``: ``(boxes [B, max_ids, 4] int32 (x1, y1, x2, y2), inclusive; n_px [B, max_ids] int32)`` of the ids of
    every image in ``segmentation [B, H, W]`` int32.  ``ids``: per-image lists, or an int32 device tensor ``[B, max_ids]`` with
    ``count [B]`` (default: all ``max_ids``).  A slot with ``n_px == 0`` (absent id, padding) has an unspecified box."""
    seg = _aug_frames(segmentation, "seg_boxes: segmentation", torch.int32, False)
    B, h, w, dev = seg.shape[0], seg.shape[1], seg.shape[2], seg.device
    if isinstance(ids, torch.Tensor) and ids.is_cuda:
        if ids.dtype != torch.int32 or ids.dim() != 2 or ids.shape[0] != B or ids.shape[1] < 1 or not ids.is_contiguous() or ids.device != dev:
            raise ValueError("seg_boxes: ids must be a dense [B, max_ids] int32 tensor on the segmentation's device")
        table = ids
        cnt = _aug_param(ids.shape[1] if count is None else count, B, torch.int32, dev, "count")
    else:
        if count is not None:
            raise ValueError("seg_boxes: count goes with a device tensor of ids; lists carry their own lengths")
        t, c = seg_boxes_table(ids, B)
        table, cnt = torch.from_numpy(t).to(dev), torch.from_numpy(c).to(dev)
    max_ids = int(table.shape[1])
    if max_ids > SEG_BOXES_MAX_IDS:
        raise ValueError(f"seg_boxes: at most {SEG_BOXES_MAX_IDS} ids per image, got {max_ids}")
    boxes = torch.empty((B, max_ids, 4), dtype=torch.int32, device=dev)
    n_px = torch.empty((B, max_ids), dtype=torch.int32, device=dev)
    if B:
        with torch.cuda.device(dev):
            check(lib().hp_seg_boxes(B, h, w, ptr(seg), ptr(table), ptr(cnt), max_ids, ptr(boxes), ptr(n_px), stream_ptr(dev)), "hp_seg_boxes")
    return boxes, n_px


# ---- the detector's training targets and losses (csrc/det_losses.hip) --------------------------------------------------------------
def _det_rows(what: str, image_of, n: int, n_images: int, dev) -> torch.Tensor:
    _assert_ids(image_of, n_images, f"{what}: image_of")
    image_of = _i32(image_of, dev)
    assert image_of.shape == (n,), f"{what}: image_of [n]"
    return image_of


def _det_device_ids(ids: torch.Tensor, lo: int, hi: int, what: str) -> None:
    """Index columns that live on the device are range-checked too before the launch that gathers through them (one read-back of
    two numbers): the training step is not a latency path."""
    if ids.numel():
        a, b = torch.stack([ids.min(), ids.max()]).tolist()
        assert lo <= a and b < hi, f"{what}: ids in [{a}, {b}] outside [{lo}, {hi})"


def _det_gt(what: str, gt: torch.Tensor, gt_off, dev):
    assert gt.dim() == 2 and gt.shape[1] == 4, f"{what}: gt [G, 4] xyxy"
    off = np.asarray(torch.as_tensor(gt_off).cpu(), dtype=np.int64).reshape(-1)
    assert off.size >= 2 and off[0] == 0 and off[-1] == gt.shape[0] and (np.diff(off) >= 0).all(), \
        f"{what}: gt_off [B + 1] ascends from 0 to G"
    return _f32(gt, dev), torch.as_tensor(off.astype(np.int32), device=dev), off.size - 1


def det_assign(boxes: torch.Tensor, image_of, gt: torch.Tensor, gt_off, high: float, low: float,
               allow_low_quality: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """``hp_det_assign``: torchvision's ``Matcher`` on ``box_iou(gt of the row's image, boxes)`` -> ``(match [n] int32, iou [n])``.
    ``match`` indexes the batch's ground-truth table ``gt [G, 4]`` (image ``b`` owns rows ``gt_off[b] .. gt_off[b + 1] - 1``);
    -1 below ``low``, -2 between the thresholds."""
    dev = _on_device("det_assign", boxes=boxes, gt=gt)
    assert boxes.dim() == 2 and boxes.shape[1] == 4, "det_assign: boxes [n, 4] xyxy"
    n = boxes.shape[0]
    gt, off, n_images = _det_gt("det_assign", gt, gt_off, dev)
    image_of = _det_rows("det_assign", image_of, n, n_images, dev)
    _det_device_ids(image_of, 0, n_images, "det_assign: image_of")
    boxes = _f32(boxes, dev)
    match = torch.empty(n, dtype=torch.int32, device=dev)
    iou = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return match, iou
    G = gt.shape[0]
    nbytes = int(lib().hp_det_assign_workspace_bytes(n, G))
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_det_assign(n, ptr(boxes), ptr(image_of), n_images, ptr(gt) if G else None, G, ptr(off), C.c_float(high), C.c_float(low),
                                  int(bool(allow_low_quality)), ptr(match), ptr(iou), ptr(ws), nbytes, stream_ptr(dev)), "hp_det_assign")
    return match, iou


def det_sample_keys(image_of: torch.Tensor, n_images: int, seed: int, stream: int = 0) -> torch.Tensor:
    """``hp_det_sample_keys``: one Philox word per row ``[n]`` (int64 tensor holding uint32 values), from ``(index of the row
    within its image, image, stream, seed)`` alone."""
    dev = _on_device("det_sample_keys", image_of=image_of)
    n = image_of.shape[0]
    image_of = _det_rows("det_sample_keys", image_of, n, n_images, dev)
    assert 0 <= seed < 2 ** 64 and 0 <= stream < 2 ** 32, "det_sample_keys: seed is an unsigned 64-bit, stream a 32-bit integer"
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return keys.to(torch.int64)
    _det_device_ids(image_of, 0, n_images, "det_sample_keys: image_of")
    # the index of a row among the rows of its image, whatever the order of the images
    order = image_of.argsort(stable=True)
    starts = torch.cumsum(torch.bincount(image_of, minlength=n_images), 0) - torch.bincount(image_of, minlength=n_images)
    index = torch.empty(n, dtype=torch.int64, device=dev)
    index[order] = torch.arange(n, device=dev) - starts[image_of[order].long()]
    index = index.to(torch.int32)
    with torch.cuda.device(dev):
        check(lib().hp_det_sample_keys(n, ptr(index), ptr(image_of), stream, seed, ptr(keys), stream_ptr(dev)), "hp_det_sample_keys")
    return keys.to(torch.int64) & 0xFFFFFFFF


def det_sample(labels: torch.Tensor, image_of, n_images: int, batch_size_per_image: int, positive_fraction: float, seed: int,
               stream: int = 0) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """``BalancedPositiveNegativeSampler``: per image ``(positive rows, negative rows)``, ascending row indices of the batch.
    Positives are ``labels >= 1``, negatives ``labels == 0``; of each class the ``k`` rows with the smallest ``(key, row)`` are
    kept, ``k_pos = min(n_pos, int(batch_size_per_image * positive_fraction))``, ``k_neg = min(n_neg, batch_size_per_image -
    k_pos)`` -- torchvision's arithmetic on this library's keys (``det_sample_keys``), not torch's ``randperm`` stream."""
    dev = _on_device("det_sample", labels=labels)
    n = labels.shape[0]
    image_of = _det_rows("det_sample", image_of, n, n_images, dev)
    keys = det_sample_keys(image_of, n_images, seed, stream)
    rows = torch.arange(n, device=dev)
    composite = keys * (1 << 31) + rows  # (key, row): rows < 2^31
    num_pos_max = int(batch_size_per_image * positive_fraction)
    out = []
    for b in range(n_images):
        mine = image_of == b
        pos, neg = rows[mine & (labels >= 1)], rows[mine & (labels == 0)]
        k_pos = min(pos.numel(), num_pos_max)
        k_neg = min(neg.numel(), batch_size_per_image - k_pos)
        pos = pos[composite[pos].argsort()[:k_pos]].sort().values
        neg = neg[composite[neg].argsort()[:k_neg]].sort().values
        out.append((pos, neg))
    return out


def det_box_encode(boxes: torch.Tensor, match: torch.Tensor, gt: torch.Tensor, weights=(1.0, 1.0, 1.0, 1.0)) -> torch.Tensor:
    """``hp_det_box_encode``: ``BoxCoder(weights).encode_single(gt[match], boxes)`` ``[n, 4]``; the zero box where ``match < 0``."""
    dev = _on_device("det_box_encode", boxes=boxes, match=match, gt=gt)
    assert boxes.dim() == 2 and boxes.shape[1] == 4 and gt.dim() == 2 and gt.shape[1] == 4, "det_box_encode: boxes [n, 4], gt [G, 4]"
    n, G = boxes.shape[0], gt.shape[0]
    assert match.shape == (n,) and len(weights) == 4
    boxes, gt, match = _f32(boxes, dev), _f32(gt, dev), _i32(match, dev)
    _det_device_ids(match, -2, G, "det_box_encode: match")
    out = torch.empty(n, 4, dtype=torch.float32, device=dev)
    if n:
        with torch.cuda.device(dev):
            check(lib().hp_det_box_encode(n, ptr(boxes), ptr(match), ptr(gt) if G else None, G, *[C.c_float(float(w)) for w in weights],
                                          ptr(out), stream_ptr(dev)), "hp_det_box_encode")
    return out


def det_mask_targets(masks: torch.Tensor, match: torch.Tensor, rois: torch.Tensor, M: int) -> torch.Tensor:
    """``hp_det_mask_targets``: ``roi_align(masks[match][:, None], rois, (M, M), 1)[:, 0]`` with the adaptive sampling ratio,
    ``aligned=False``: ``masks [G, H, W]`` uint8, ``rois [n, 4]`` -> ``[n, M, M]`` float32."""
    dev = _on_device("det_mask_targets", masks=masks, match=match, rois=rois)
    assert masks.dim() == 3 and masks.dtype in (torch.uint8, torch.bool), "det_mask_targets: masks [G, H, W] uint8"
    assert rois.dim() == 2 and rois.shape[1] == 4 and match.shape == (rois.shape[0],), "det_mask_targets: rois [n, 4], match [n]"
    n, (G, H, W) = rois.shape[0], masks.shape
    out = torch.empty(n, M, M, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    masks, match, rois = masks.to(torch.uint8).contiguous(), _i32(match, dev), _f32(rois, dev)
    _det_device_ids(match, 0, G, "det_mask_targets: match")
    with torch.cuda.device(dev):
        check(lib().hp_det_mask_targets(n, ptr(masks), G, H, W, ptr(match), ptr(rois), M, ptr(out), stream_ptr(dev)), "hp_det_mask_targets")
    return out


def _det_loss_workspace(rows: int, dev) -> Tuple[torch.Tensor, int]:
    nbytes = int(lib().hp_det_loss_workspace_bytes(rows))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=dev), nbytes


def loss_rpn(objectness: torch.Tensor, pred_deltas: torch.Tensor, labels: torch.Tensor, targets: torch.Tensor, sampled: torch.Tensor):
    """``hp_loss_rpn``: ``objectness [A]``, ``pred_deltas [A, 4]``, ``labels [A]`` (>= 1 positive, 0 negative), ``targets [A, 4]``,
    ``sampled [k]`` distinct rows -> ``(loss [2] = objectness, box, grad_objectness [A], grad_deltas [A, 4])`` for an upstream
    gradient of 1.  ``k == 0``: zeros."""
    dev = _on_device("loss_rpn", objectness=objectness, pred_deltas=pred_deltas, labels=labels, targets=targets, sampled=sampled)
    A = objectness.numel()
    assert pred_deltas.shape == (A, 4) and labels.shape == (A,) and targets.shape == (A, 4), "loss_rpn: [A], [A, 4], [A], [A, 4]"
    objectness, pred_deltas, targets = _f32(objectness.reshape(-1), dev), _f32(pred_deltas, dev), _f32(targets, dev)
    labels, sampled = _i32(labels, dev), _i32(sampled.reshape(-1), dev)
    k = sampled.numel()
    _det_device_ids(sampled, 0, A, "loss_rpn: sampled")
    loss = torch.zeros(2, dtype=torch.float32, device=dev)
    g_obj = torch.empty(A, dtype=torch.float32, device=dev)
    g_del = torch.empty(A, 4, dtype=torch.float32, device=dev)
    if k == 0:
        return loss, g_obj.zero_(), g_del.zero_()
    with torch.cuda.device(dev):
        ws, nbytes = _det_loss_workspace((k + 255) // 256, dev)
        check(lib().hp_loss_rpn(A, k, ptr(sampled), ptr(objectness), ptr(pred_deltas), ptr(labels), ptr(targets), ptr(loss), ptr(g_obj),
                                ptr(g_del), ptr(ws), nbytes, stream_ptr(dev)), "hp_loss_rpn")
    return loss, g_obj, g_del


def loss_fastrcnn(class_logits: torch.Tensor, box_regression: torch.Tensor, labels: torch.Tensor, targets: torch.Tensor,
                  num_classes: Optional[int] = None):
    """``hp_loss_fastrcnn``: ``class_logits [n, ld]`` of which the first ``num_classes`` columns are classes, ``box_regression
    [n, >= 4 num_classes]``, ``labels [n]``, ``targets [n, 4]`` -> ``(loss [2] = classifier, box, grad_logits, grad_regression)``
    in the shapes of the inputs.  ``n == 0``: zeros."""
    dev = _on_device("loss_fastrcnn", class_logits=class_logits, box_regression=box_regression, labels=labels, targets=targets)
    assert class_logits.dim() == 2 and box_regression.dim() == 2, "loss_fastrcnn: class_logits [n, ld], box_regression [n, ld_reg]"
    n, ld = class_logits.shape
    ld_reg = box_regression.shape[1]
    Cn = ld if num_classes is None else int(num_classes)
    assert 1 <= Cn <= ld and 4 * Cn <= ld_reg, "loss_fastrcnn: num_classes <= ld and 4 num_classes <= ld_reg"
    assert box_regression.shape[0] == n and labels.shape == (n,) and targets.shape == (n, 4), "loss_fastrcnn: one row per proposal"
    class_logits, box_regression, targets, labels = _f32(class_logits, dev), _f32(box_regression, dev), _f32(targets, dev), _i32(labels, dev)
    _det_device_ids(labels, 0, Cn, "loss_fastrcnn: labels")
    loss = torch.zeros(2, dtype=torch.float32, device=dev)
    g_cls = torch.empty(n, ld, dtype=torch.float32, device=dev)
    g_reg = torch.empty(n, ld_reg, dtype=torch.float32, device=dev)
    if n == 0:
        return loss, g_cls, g_reg
    with torch.cuda.device(dev):
        ws, nbytes = _det_loss_workspace((n + 255) // 256, dev)
        check(lib().hp_loss_fastrcnn(n, Cn, ld, ld_reg, ptr(class_logits), ptr(box_regression), ptr(labels), ptr(targets), ptr(loss),
                                     ptr(g_cls), ptr(g_reg), ptr(ws), nbytes, stream_ptr(dev)), "hp_loss_fastrcnn")
    return loss, g_cls, g_reg


def loss_mask(mask_logits: torch.Tensor, labels: torch.Tensor, targets: torch.Tensor):
    """``hp_loss_mask``: ``mask_logits [n, C, M, M]``, ``labels [n]``, ``targets [n, M, M]`` -> ``(loss [1], grad_logits)``.
    ``n == 0``: a loss of 0, nothing launched."""
    dev = _on_device("loss_mask", mask_logits=mask_logits, labels=labels, targets=targets)
    assert mask_logits.dim() == 4 and mask_logits.shape[2] == mask_logits.shape[3], "loss_mask: mask_logits [n, C, M, M]"
    n, Cn, M, _ = mask_logits.shape
    assert labels.shape == (n,) and targets.shape == (n, M, M), "loss_mask: labels [n], targets [n, M, M]"
    mask_logits, targets, labels = _f32(mask_logits, dev), _f32(targets, dev), _i32(labels, dev)
    _det_device_ids(labels, 0, Cn, "loss_mask: labels")
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    grad = torch.empty(n, Cn, M, M, dtype=torch.float32, device=dev)
    if n == 0:
        return loss, grad
    with torch.cuda.device(dev):
        ws, nbytes = _det_loss_workspace(n, dev)
        check(lib().hp_loss_mask(n, Cn, M, ptr(mask_logits), ptr(labels), ptr(targets), ptr(loss), ptr(grad), ptr(ws), nbytes,
                                 stream_ptr(dev)), "hp_loss_mask")
    return loss, grad


# ---- batch assembly of the training data sets (csrc/batch_data.hip) ------------------------------------------------------------------
def _dense(t, dtype, shape: tuple, what: str) -> torch.Tensor:
    """A dense device tensor of ``dtype`` and ``shape`` (None: any size); a CPU tensor raises ValueError (no host implementation)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{what}: a tensor on the device is required (no CPU implementation)")
    ok = t.dtype == dtype and t.dim() == len(shape) and all(s is None or int(d) == s for d, s in zip(t.shape, shape)) and t.is_contiguous()
    if not ok:
        want = "[" + ", ".join("*" if s is None else str(s) for s in shape) + "]"
        raise ValueError(f"{what}: dense {want} {dtype} expected, got {tuple(t.shape)} {t.dtype}")
    return t


def _one_device(what: str, dev, *tensors) -> None:
    for t in tensors:
        if t is not None and t.device != dev:
            raise ValueError(f"{what}: every tensor lives on one device, got {t.device} beside {dev}")


def pose_batch_select(n_px: torch.Tensor, boxes: torch.Tensor, TWC: torch.Tensor, TWO: torch.Tensor, count=None,
                      keep: Optional[torch.Tensor] = None, min_area: Optional[float] = None, first: bool = False, *, seed: int = 0,
                      row_offset: int = 0):
    """``hp_pose_batch_select``: one object per frame.  ``n_px [B, max_ids]``, ``boxes [B, max_ids, 4]`` int32 as ``seg_boxes``
    returns them, ``TWC [B, 4, 4]``, ``TWO [B, max_ids, 4, 4]`` float32, ``count`` (a scalar or ``[B]``; default ``max_ids``),
    ``keep [B, max_ids]`` bool / uint8 or None, ``min_area`` None or a number (``area >= min_area`` on the inclusive box without
    + 1), ``first``: the first valid slot instead of the seeded one (``seed``, ``row_offset + b``).  Returns ``(chosen [B] int32,
    valid [B] bool, bbox [B, 4] float32, TCO [B, 4, 4] float32, dst [B] int32, n_valid [1] int32)``, all on the device."""
    n_px = _dense(n_px, torch.int32, (None, None), "pose_batch_select: n_px")
    B, max_ids, dev = int(n_px.shape[0]), int(n_px.shape[1]), n_px.device
    boxes = _dense(boxes, torch.int32, (B, max_ids, 4), "pose_batch_select: boxes")
    TWC = _dense(TWC, torch.float32, (B, 4, 4), "pose_batch_select: TWC")
    TWO = _dense(TWO, torch.float32, (B, max_ids, 4, 4), "pose_batch_select: TWO")
    if keep is not None:
        if isinstance(keep, torch.Tensor) and keep.dtype == torch.bool:
            keep = keep.view(torch.uint8)
        keep = _dense(keep, torch.uint8, (B, max_ids), "pose_batch_select: keep")
    _one_device("pose_batch_select", dev, boxes, TWC, TWO, keep)
    if not 1 <= max_ids <= SEG_BOXES_MAX_IDS:
        raise ValueError(f"pose_batch_select: 1 .. {SEG_BOXES_MAX_IDS} ids per image, got {max_ids}")
    if not (0 <= seed < 2 ** 64 and 0 <= row_offset < 2 ** 64):
        raise ValueError("pose_batch_select: seed and row_offset are unsigned 64-bit integers")
    area = -1.0 if min_area is None else float(min_area)
    if not area >= 0.0 and min_area is not None:
        raise ValueError(f"pose_batch_select: min_area is None or a number >= 0, got {min_area}")
    chosen = torch.empty(B, dtype=torch.int32, device=dev)
    valid = torch.empty(B, dtype=torch.uint8, device=dev)
    bbox = torch.empty(B, 4, dtype=torch.float32, device=dev)
    TCO = torch.empty(B, 4, 4, dtype=torch.float32, device=dev)
    dst = torch.empty(B, dtype=torch.int32, device=dev)
    n_valid = torch.zeros(1, dtype=torch.int32, device=dev)
    if B:
        cnt = _aug_param(max_ids if count is None else count, B, torch.int32, dev, "count")
        with torch.cuda.device(dev):
            check(lib().hp_pose_batch_select(B, max_ids, ptr(n_px), ptr(boxes), ptr(cnt), ptr(keep), C.c_float(area), int(bool(first)), seed,
                                             row_offset, ptr(TWC), ptr(TWO), ptr(chosen), ptr(valid), ptr(bbox), ptr(TCO), ptr(dst),
                                             ptr(n_valid), stream_ptr(dev)), "hp_pose_batch_select")
    return chosen, valid.view(torch.bool), bbox, TCO, dst, n_valid


def batch_gather_chw(rgb: torch.Tensor, valid: torch.Tensor, dst: torch.Tensor, n_out: Optional[int] = None,
                     depth: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_depth: Optional[torch.Tensor] = None):
    """``hp_batch_gather_chw``: ``rgb [B, H, W, 3]`` uint8 -> ``[n_out, 3, H, W]``, frame ``b`` with ``valid[b]`` to row ``dst[b]``
    (``valid [B]`` bool / uint8 and ``dst [B]`` int32 as ``pose_batch_select`` returns them); with ``depth [B, H, W]`` float32 also
    ``[n_out, H, W]``, bits copied.  ``n_out`` is the number of output rows (or pass ``out`` / ``out_depth``, which may be larger
    than the number of valid frames: the rows no frame names are left as they are).  Returns ``(rgbs, depths or None)``."""
    rgb = _aug_frames(rgb, "batch_gather_chw: rgb", torch.uint8, True)
    B, h, w, dev = int(rgb.shape[0]), int(rgb.shape[1]), int(rgb.shape[2]), rgb.device
    if isinstance(valid, torch.Tensor) and valid.dtype == torch.bool:
        valid = valid.view(torch.uint8)
    valid = _dense(valid, torch.uint8, (B,), "batch_gather_chw: valid")
    dst = _dense(dst, torch.int32, (B,), "batch_gather_chw: dst")
    if depth is not None:
        depth = _dense(depth, torch.float32, (B, h, w), "batch_gather_chw: depth")
    elif out_depth is not None:
        raise ValueError("batch_gather_chw: out_depth without depth")
    if n_out is None:
        if out is None:
            raise ValueError("batch_gather_chw: n_out or out is required (the number of valid frames lives on the device)")
        n_out = int(out.shape[0])
    if n_out < 0:
        raise ValueError(f"batch_gather_chw: n_out = {n_out}")
    if out is None:
        out = torch.empty(n_out, 3, h, w, dtype=torch.uint8, device=dev)
    out = _dense(out, torch.uint8, (n_out, 3, h, w), "batch_gather_chw: out")
    if depth is not None:
        if out_depth is None:
            out_depth = torch.empty(n_out, h, w, dtype=torch.float32, device=dev)
        out_depth = _dense(out_depth, torch.float32, (n_out, h, w), "batch_gather_chw: out_depth")
    _one_device("batch_gather_chw", dev, valid, dst, depth, out, out_depth)
    if B and n_out:
        with torch.cuda.device(dev):
            check(lib().hp_batch_gather_chw(B, h, w, ptr(rgb), ptr(depth), ptr(valid), ptr(dst), n_out, ptr(out), ptr(out_depth),
                                            stream_ptr(dev)), "hp_batch_gather_chw")
    return out, out_depth


def instance_masks(segmentation: torch.Tensor, ids, slot_row, G: int, count=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``hp_instance_masks``: ``masks [G, H, W]`` uint8, ``masks[slot_row[b, k]] = (segmentation[b] == ids[b, k])`` for the slots
    with ``0 <= slot_row[b, k] < G`` (distinct rows).  ``segmentation [B, H, W]`` int32; ``ids`` and ``slot_row`` ``[B, max_ids]``
    (arrays, or int32 device tensors), ``count`` a scalar or ``[B]`` (default ``max_ids``).  Rows are written completely."""
    seg = _aug_frames(segmentation, "instance_masks: segmentation", torch.int32, False)
    B, h, w, dev = int(seg.shape[0]), int(seg.shape[1]), int(seg.shape[2]), seg.device
    tables = []
    for name, t in (("ids", ids), ("slot_row", slot_row)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            a = np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t)
            if a.ndim != 2 or a.shape[0] != B or a.dtype.kind not in "iu" or (a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31)):
                raise ValueError(f"instance_masks: {name} must be [B, max_ids] integers that fit int32")
            t = torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
        tables.append(_dense(t, torch.int32, (B, None), f"instance_masks: {name}"))
    table, rows = tables
    max_ids = int(table.shape[1])
    if rows.shape != table.shape or not 1 <= max_ids <= SEG_BOXES_MAX_IDS:
        raise ValueError(f"instance_masks: ids and slot_row [B, max_ids] with 1 .. {SEG_BOXES_MAX_IDS} ids per image")
    G = int(G)
    if G < 0:
        raise ValueError(f"instance_masks: G = {G}")
    if out is None:
        out = torch.empty(G, h, w, dtype=torch.uint8, device=dev)
    out = _dense(out, torch.uint8, (G, h, w), "instance_masks: out")
    _one_device("instance_masks", dev, table, rows, out)
    if B and G:
        cnt = _aug_param(max_ids if count is None else count, B, torch.int32, dev, "count")
        with torch.cuda.device(dev):
            check(lib().hp_instance_masks(B, h, w, ptr(seg), ptr(table), ptr(cnt), ptr(rows), max_ids, G, ptr(out), stream_ptr(dev)),
                  "hp_instance_masks")
    return out
