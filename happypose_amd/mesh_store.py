"""Object/mesh containers of the path.

Mirrors (API names, argument meaning) the reference's
``RigidObject`` / ``RigidObjectDataset`` (``TB/datasets/object_dataset.py:32-174``),
``MeshDataBase`` / ``BatchedMeshes`` / ``Meshes``
(``TB/lib3d/rigid_mesh_database.py:52-200``) and adds ``PackedMeshes``: the flat,
device-friendly layout the HIP rasteriser and the pose-prep kernel read
(all objects concatenated; one ``int64[8]`` descriptor row per object).
"""

from __future__ import annotations

from copy import deepcopy
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

from .mesh_io import MeshData, load_mesh


class RigidObject:
    """``TB/datasets/object_dataset.py:32-143``.  ``mesh_path`` may also be an
    in-memory :class:`MeshData` (synthetic scenes)."""

    def __init__(
        self,
        label: str,
        mesh_path,
        category: Optional[str] = None,
        mesh_diameter: Optional[float] = None,
        mesh_units: str = "m",
        symmetries_discrete: Sequence = (),
        symmetries_continuous: Sequence = (),
        ypr_offset_deg: Tuple[float, float, float] = (0.0, 0.0, 0.0),
        scaling_factor: float = 1.0,
        scaling_factor_mesh_units_to_meters: Optional[float] = None,
    ):
        self.label = label
        self.category = category
        self.mesh_path = mesh_path
        self.mesh_units = mesh_units
        if scaling_factor_mesh_units_to_meters is not None:
            self.scaling_factor_mesh_units_to_meters = scaling_factor_mesh_units_to_meters
        else:
            self.scaling_factor_mesh_units_to_meters = {"m": 1.0, "mm": 0.001}[mesh_units]
        self.scaling_factor = scaling_factor
        self.mesh_diameter = mesh_diameter
        self.diameter_meters = None
        self.symmetries_discrete = list(symmetries_discrete)
        self.symmetries_continuous = list(symmetries_continuous)
        self.ypr_offset_deg = ypr_offset_deg
        self._mesh: Optional[MeshData] = mesh_path if isinstance(mesh_path, MeshData) else None

    @property
    def is_symmetric(self) -> bool:
        return len(self.symmetries_discrete) > 0 or len(self.symmetries_continuous) > 0

    @property
    def scale(self) -> float:
        return self.scaling_factor_mesh_units_to_meters * self.scaling_factor

    def load(self) -> MeshData:
        if self._mesh is None:
            self._mesh = load_mesh(self.mesh_path)
        return self._mesh


class RigidObjectDataset:
    """``TB/datasets/object_dataset.py:146-174``."""

    def __init__(self, objects: List[RigidObject]):
        self.list_objects = objects
        self.label_to_objects = {obj.label: obj for obj in objects}
        if len(self.list_objects) != len(self.label_to_objects):
            raise RuntimeError("There are objects with duplicate labels")

    def __getitem__(self, idx: int) -> RigidObject:
        return self.list_objects[idx]

    def get_object_by_label(self, label: str) -> RigidObject:
        return self.label_to_objects[label]

    def __len__(self) -> int:
        return len(self.list_objects)

    @property
    def objects(self) -> List[RigidObject]:
        return self.list_objects

    def filter_objects(self, keep_labels: Set[str]) -> "RigidObjectDataset":
        return RigidObjectDataset([o for o in self.list_objects if o.label in keep_labels])


def pad_stack_points(points_list: List[np.ndarray]) -> np.ndarray:
    """``pad_stack_tensors(fill="select_random", deterministic=True)``
    (``TB/lib3d/rigid_mesh_database.py:172-200``): shorter point sets are padded by
    re-sampling their own vertices from ONE ``RandomState(0)`` stream shared by all
    objects in order."""
    n_max = max(len(p) for p in points_list)
    rs = np.random.RandomState(0)
    out = []
    for p in points_list:
        n_pad = n_max - len(p)
        if n_pad > 0:
            ids_pad = rs.choice(np.arange(len(p)), size=n_pad)
            p = np.concatenate((p, p[ids_pad]), axis=0)
        out.append(p)
    return np.stack(out)


def sample_point_ids(n_pad: int, n_points: int) -> np.ndarray:
    """Deterministic ids of ``sample_points(..., deterministic=True)``
    (``TB/lib3d/mesh_ops.py:74-84``)."""
    assert n_points <= n_pad
    return np.random.RandomState(0).choice(n_pad, size=n_points, replace=False)


class Meshes:
    """``TB/lib3d/rigid_mesh_database.py:151-169`` (tensor-collection of selected
    objects).  ``points`` is ``[b, N_pad, 3]``, ``symmetries`` ``[b, S_max, 4, 4]`` (or None)."""

    def __init__(self, infos, labels, points, symmetries=None):
        self.infos = infos
        self.labels = np.asarray(labels)
        self.points = points
        self.symmetries = symmetries

    def sample_points(self, n_points: int, deterministic: bool = False):
        n_pad = self.points.shape[1]
        assert n_points <= n_pad
        rs = np.random.RandomState(0) if deterministic else np.random
        ids = rs.choice(n_pad, size=n_points, replace=False)
        return self.points[:, ids]


class BatchedMeshes:
    """``TB/lib3d/rigid_mesh_database.py:133-149``: ``points [n_obj, N_pad, 3]``
    float32, metres.  ``points`` is a numpy array on the host and, after
    :meth:`to`, a torch tensor on the compute device."""

    def __init__(self, infos, labels, points, symmetries=None, unsupported_symmetries=()):
        self.infos = infos
        # labels whose symmetries could not be tabulated: the multi-view path refuses them (ops._mv_tables)
        self.unsupported_symmetries = list(unsupported_symmetries)
        self.label_to_id: Dict[str, int] = {label: n for n, label in enumerate(labels)}
        self.labels = np.asarray(labels)
        self.points = points
        # [n_obj, S_max, 4, 4] float32, rows past an object's own count are identity (CP/lib3d/rigid_mesh_database.py:73-77)
        self.symmetries = symmetries
        self._n_sym_device = None

    @property
    def device_tables(self):
        """What the multi-view kernels read (csrc/multiview.hip): float32 views of ``points`` / ``symmetries`` as they are NOW
        (after ``to`` / ``float`` / ``half`` there is one copy, not two) and the per-object ``n_sym``.  None before ``to()``."""
        if self.symmetries is None or isinstance(self.points, np.ndarray):
            return None
        import torch

        if self._n_sym_device is None or self._n_sym_device.device != self.points.device:
            self._n_sym_device = torch.as_tensor(self.n_sym).to(self.points.device)
        return {"points": self.points.to(torch.float32).contiguous(), "symmetries": self.symmetries.to(torch.float32).contiguous(),
                "n_sym": self._n_sym_device}

    @property
    def n_sym_mapping(self) -> Dict[str, int]:
        """``CP/lib3d/rigid_mesh_database.py:90-92``."""
        return {label: obj["n_sym"] for label, obj in self.infos.items()}

    @property
    def n_sym(self) -> np.ndarray:
        """Per-object symmetry count ``[n_obj]`` int32, in table order."""
        return np.asarray([self.infos[label]["n_sym"] for label in self.labels], dtype=np.int32)

    def select(self, labels) -> Meshes:
        ids = [self.label_to_id[label] for label in labels]
        sym = None if self.symmetries is None else self.symmetries[ids]
        return Meshes([self.infos[label] for label in labels], self.labels[ids], self.points[ids], sym)

    def ids_of(self, labels) -> np.ndarray:
        return np.asarray([self.label_to_id[label] for label in labels], dtype=np.int32)

    def to(self, device):
        import torch

        self.points = torch.as_tensor(self.points).to(device)
        if self.symmetries is not None:
            self.symmetries = torch.as_tensor(self.symmetries).to(device)
        return self

    def float(self):
        return self

    def cuda(self):
        return self.to("cuda")


class MeshDataBase:
    """``TB/lib3d/rigid_mesh_database.py:52-130``."""

    def __init__(self, obj_list: List[RigidObject]):
        self.obj_dict = {obj.label: obj for obj in obj_list}
        self.obj_list = obj_list
        self.infos = {obj.label: {} for obj in obj_list}
        self.meshes = {label: obj.load() for label, obj in self.obj_dict.items()}
        for label, obj in self.obj_dict.items():
            if obj.diameter_meters is None:
                points = np.asarray(self.meshes[label].vertices) * obj.scale
                extent = points.max(0) - points.min(0)
                obj.diameter_meters = float(np.linalg.norm(extent))
            # what the evaluation reads per label (CP/lib3d/rigid_mesh_database.py keeps the object's dict as its infos)
            self.infos[label].update(diameter_m=obj.diameter_meters, is_symmetric=obj.is_symmetric)

    @staticmethod
    def from_object_ds(object_ds: RigidObjectDataset) -> "MeshDataBase":
        return MeshDataBase([object_ds[n] for n in range(len(object_ds))])

    def batched(self, aabb: bool = False, resample_n_points: Optional[int] = None, n_sym: int = 64, resample_seed: int = 0,
                resample_method: str = "random", resample_oversample: int = 8) -> BatchedMeshes:
        """``CP/lib3d/rigid_mesh_database.py:27-78``.  ``aabb=True``: the points are the 8 corners of the bounding
        box; ``n_sym``: rotations per continuous symmetry axis.  The no-argument call gives the same points as
        before; the symmetry table is always attached.

        ``resample_n_points=N``: every object's table is ``N`` points.  A mesh with faces is resampled on the device
        (:meth:`resample_surface`); a mesh without faces (a point cloud) takes the reference's other branch
        (``TB/lib3d/rigid_mesh_database.py:96-101``), the deterministic vertex subset :func:`sample_point_ids`, on the host."""
        if aabb:
            assert resample_n_points is None
        resampled = {}
        if resample_n_points:
            resampled = self.resample_surface(int(resample_n_points), seed=resample_seed, method=resample_method,
                                              oversample=resample_oversample)
        labels, points, symmetries, unsupported = [], [], [], []
        new_infos = deepcopy(self.infos)
        for label, mesh in self.meshes.items():
            obj = self.obj_dict[label]
            pts = np.asarray(mesh.vertices, dtype=np.float64)
            if aabb:
                pts = bounding_box_corners(pts)
            elif resample_n_points:
                pts = resampled[label] if label in resampled else pts[sample_point_ids(len(pts), int(resample_n_points))]
            pts = pts * obj.scale
            try:
                sym = make_bop_symmetries(obj.symmetries_discrete, obj.symmetries_continuous, n_sym,
                                          obj.scaling_factor_mesh_units_to_meters)
            except UnsupportedSymmetryError:
                # a continuous symmetry the reference's formula does not cover (offset, non-unit or negative axis): the
                # single-view path never needed the table, so batching still works; the multi-view path says why it cannot
                sym, unsupported = np.eye(4)[None], unsupported + [label]
            new_infos[label]["n_points"] = pts.shape[0]
            new_infos[label]["n_sym"] = sym.shape[0]
            points.append(pts)
            symmetries.append(sym)
            labels.append(label)
        pts = pad_stack_points(points).astype(np.float32)
        s_max = max(len(s) for s in symmetries)
        sym = np.tile(np.eye(4), (len(symmetries), s_max, 1, 1))
        for n, s in enumerate(symmetries):
            sym[n, :len(s)] = s
        return BatchedMeshes(new_infos, np.array(labels), pts, sym.astype(np.float32), unsupported_symmetries=unsupported)

    def resample_surface(self, n_points: int, seed: int = 0, method: str = "random", oversample: int = 8, device="cuda") -> Dict[str, np.ndarray]:
        """``n_points`` points on the surface of every mesh that has faces: ``{label: [n_points, 3] float64}`` in MESH units,
        drawn on the device by ``ops.mesh_sample_surface`` (area-uniform; the definition is in ``include/happypose_amd.h``).
        Object ``o`` of the random stream is the object's position in ``self.meshes``, so a label's points do not depend on
        which other meshes have faces.  ``method="fps"`` draws ``oversample * n_points`` samples and keeps ``n_points`` of them
        by farthest-point sampling (``ops.farthest_point_ids``; the first sample starts the selection), in selection order."""
        assert method in ("random", "fps"), f"resample_method {method!r}: 'random' or 'fps'"
        assert n_points >= 1 and (method == "random" or oversample >= 1)
        labels = list(self.meshes)
        with_faces = [label for label in labels if len(self.meshes[label].faces)]
        if not with_faces:
            return {}
        import torch

        if not torch.cuda.is_available():  # there is no CPU implementation of the surface draw, and none is substituted
            raise NotImplementedError("resample_n_points on a mesh with faces is drawn on the device (hp_mesh_sample_surface): "
                                      "no GPU is available and there is no CPU implementation")
        from . import ops  # the device library is needed from here on (ops imports this module)

        # every mesh keeps its position; one without faces is passed empty and its (NaN) rows are not read
        verts = [self.meshes[label].vertices if label in with_faces else np.zeros((0, 3)) for label in labels]
        faces = [self.meshes[label].faces if label in with_faces else np.zeros((0, 3), np.int32) for label in labels]
        n_draw = n_points * oversample if method == "fps" else n_points
        pts = ops.mesh_sample_surface(verts, faces, n_draw, seed=seed, device=device)
        if method == "fps":
            counts = torch.as_tensor([n_draw if label in with_faces else 0 for label in labels], dtype=torch.int32)
            ids = ops.farthest_point_ids(pts, counts, n_points).long().clamp_(min=0)
            pts = torch.gather(pts, 1, ids.unsqueeze(-1).expand(-1, -1, 3))
        pts = pts.cpu().numpy().astype(np.float64)
        out = {label: pts[o] for o, label in enumerate(labels) if label in with_faces}
        no_area = [label for label, p in out.items() if not np.isfinite(p).all()]
        if no_area:  # the kernels answer a surface without (finite) area with NaN points
            raise ValueError(f"resample_n_points: the faces of {no_area} have no finite, positive area")
        return out


def bounding_box_corners(pts: np.ndarray) -> np.ndarray:
    """The 8 corners of the axis-aligned box of ``pts [n, 3]`` in the order of ``get_meshes_bounding_boxes``
    (``CP/lib3d/mesh_ops.py:15-37``)."""
    (x0, y0, z0), (x1, y1, z1) = pts.min(0), pts.max(0)
    return np.array([[x0, y1, z1], [x1, y1, z1], [x1, y0, z1], [x0, y0, z1],
                     [x0, y1, z0], [x1, y1, z0], [x1, y0, z0], [x0, y0, z0]], dtype=pts.dtype)


class UnsupportedSymmetryError(ValueError):
    """A continuous symmetry outside what ``make_bop_symmetries`` covers (offset, or an axis other than +x / +y / +z)."""


def make_bop_symmetries(symmetries_discrete, symmetries_continuous, n_symmetries_continuous: int = 64,
                        scale: float = 0.001) -> np.ndarray:
    """Symmetry table of one object ``[S, 4, 4]`` float64, after ``make_bop_symmetries``
    (``CP/lib3d/symmetries.py:7-35``): identity plus the discrete transforms (translation times ``scale``), each
    composed on the left with ``n_symmetries_continuous`` rotations about every continuous axis (``sym_c * sym_d``,
    continuous index fastest).  The rotation is ``euler2quat(axis * angle)`` in the ``sxyz`` convention, i.e.
    ``Rz(a_z) @ Ry(a_y) @ Rx(a_x)``.  **Parity unpinned**: the reference builds these through pinocchio and
    transforms3d, which are absent here; the table is restated from the formula."""
    discrete = [np.eye(4)]
    for sym_n in symmetries_discrete:
        M = np.array(sym_n, dtype=np.float64).reshape(4, 4).copy()
        M[:3, 3] *= scale
        discrete.append(M)
    continuous = []
    for sym_n in symmetries_continuous:
        axis = np.array(sym_n["axis"], dtype=np.float64)
        if not np.allclose(sym_n["offset"], 0) or axis.sum() != 1:  # the reference asserts both (CP/lib3d/symmetries.py:20-22)
            raise UnsupportedSymmetryError(f"continuous symmetry with axis {sym_n['axis']} and offset {sym_n['offset']}")
        for n in range(n_symmetries_continuous):
            ax, ay, az = axis * 2 * np.pi * n / n_symmetries_continuous
            cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
            Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
            Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
            Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
            M = np.eye(4)
            M[:3, :3] = Rz @ Ry @ Rx
            continuous.append(M)
    if continuous:
        return np.array([sym_c @ sym_d for sym_d in discrete for sym_c in continuous])
    return np.array(discrete)


def mip_chain(tex: np.ndarray):
    """Levels 1.. of an RGBA8 texture ``[h,w,4]`` as ``glGenerateMipmap`` builds them: each level halves the previous one
    (``max(1, floor(n / 2))`` per side) with a 2 x 2 box filter, rounded to nearest in 8 bit; a side that is already 1
    averages 2 x 1.  Returned without level 0."""
    levels, cur = [], np.ascontiguousarray(tex, np.uint8)
    while cur.shape[0] > 1 or cur.shape[1] > 1:
        h, w = cur.shape[0], cur.shape[1]
        nh, nw = max(1, h // 2), max(1, w // 2)
        c = cur.astype(np.uint16)
        r0 = c[0:2 * nh:2] if h > 1 else c
        r1 = c[1:2 * nh:2] if h > 1 else c
        a = r0[:, 0:2 * nw:2] if w > 1 else r0
        b = r0[:, 1:2 * nw:2] if w > 1 else r0
        cc = r1[:, 0:2 * nw:2] if w > 1 else r1
        d = r1[:, 1:2 * nw:2] if w > 1 else r1
        cur = ((a + b + cc + d + 2) >> 2).astype(np.uint8)
        levels.append(cur)
    return levels


def hpr_to_matrix(ypr_deg) -> np.ndarray:
    """Rotation of Panda3D's ``NodePath.setHpr(h, p, r)`` (degrees; Z-up, Y-forward frame): heading about +Z, pitch
    about +X, roll about +Y, applied roll first, then pitch, then heading -- ``R = Rz(h) @ Rx(p) @ Ry(r)`` on column
    vectors.  **[unverified]**: Panda3D's documented convention; Panda3D is absent here."""
    h, p, r = (np.deg2rad(float(a)) for a in ypr_deg)
    ch, sh, cp, sp, cr, sr = np.cos(h), np.sin(h), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    Rz = np.array([[ch, -sh, 0.0], [sh, ch, 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    Ry = np.array([[cr, 0.0, sr], [0.0, 1.0, 0.0], [-sr, 0.0, cr]])
    return Rz @ Rx @ Ry


class PackedMeshes:
    """Flat layout consumed by the rasteriser (HIP and oracle).

    ``verts [Vtot,3] f32`` (metres), ``normals [Vtot,3] f32``, ``uvs [Vtot,2] f32``,
    ``colors [Vtot,4] u8``, ``faces [Ftot,3] i32`` (ids local to the object),
    ``tex`` RGBA8 pool, ``obj [n_obj,8] i64`` = (vert_off, n_verts, face_off, n_faces,
    tex_off | -1, tex_w, tex_h, n_mip_levels), ``radius [n_obj] f32`` = largest vertex norm (m), ``bounds_center`` / ``bounds_radius`` = the bounding sphere light-positioning functions see.  A texture is stored as its
    level 0 followed by its mip chain (:func:`mip_chain`; level ``k`` is ``max(1, w >> k) x max(1, h >> k)``): the
    bilinear level-0 fetch ignores the chain, ``HP_RASTER_TEX_ANISO`` (the reference's ``texture-minfilter mipmap`` +
    ``texture-anisotropic-degree 16``) walks it."""

    def __init__(self, object_ds: RigidObjectDataset):
        self.labels = [o.label for o in object_ds.list_objects]
        self.label_to_id = {l: i for i, l in enumerate(self.labels)}
        verts, normals, uvs, colors, faces, tex, rows, radius = [], [], [], [], [], [], [], []
        centers, bradius = [], []
        voff = foff = toff = 0
        for obj in object_ds.list_objects:
            m = obj.load()
            v64 = np.asarray(m.vertices, dtype=np.float64) * obj.scale
            n64 = np.asarray(m.normals, np.float64)
            if tuple(float(a) for a in obj.ypr_offset_deg) != (0.0, 0.0, 0.0):
                # the RENDER mesh only is rotated (get_object_node: setScale, setHpr --
                # TB/renderer/panda3d_scene_renderer.py:206-219); the point table of MeshDataBase is not
                # (TB/lib3d/rigid_mesh_database.py:109-111)
                R = hpr_to_matrix(obj.ypr_offset_deg)
                v64, n64 = v64 @ R.T, n64 @ R.T
            v = v64.astype(np.float32)
            nv, nf = len(v), len(m.faces)
            verts.append(v)
            normals.append(n64.astype(np.float32))
            uvs.append(np.zeros((nv, 2), np.float32) if m.uvs is None else np.asarray(m.uvs, np.float32))
            if m.colors is not None:
                colors.append(np.asarray(m.colors, np.uint8).reshape(nv, 4))
            else:
                colors.append(np.full((nv, 4), 255, np.uint8))
            faces.append(np.asarray(m.faces, np.int32))
            if m.texture is not None and m.uvs is not None:
                t = np.ascontiguousarray(m.texture, np.uint8)
                chain = mip_chain(t)
                rows.append((voff, nv, foff, nf, toff, t.shape[1], t.shape[0], 1 + len(chain)))
                for lvl in [t] + chain:
                    tex.append(lvl.reshape(-1))
                    toff += lvl.size
            else:
                rows.append((voff, nv, foff, nf, -1, 0, 0, 0))
            radius.append(float(np.linalg.norm(v, axis=1).max()) if nv else 0.0)
            # bounding sphere as Panda3D builds it for a Geom (centre of the vertices' bounding box, radius = the farthest
            # vertex from it): what ``root_node.getBounds()`` answers to a light-positioning function  [unverified]
            c = (v.min(0).astype(np.float64) + v.max(0).astype(np.float64)) / 2 if nv else np.zeros(3)
            centers.append(c)
            bradius.append(float(np.linalg.norm(v.astype(np.float64) - c, axis=1).max()) if nv else 0.0)
            voff += nv
            foff += nf
        self.verts = np.concatenate(verts)
        self.normals = np.concatenate(normals)
        self.uvs = np.concatenate(uvs)
        self.colors = np.concatenate(colors)
        self.faces = np.concatenate(faces)
        self.tex = np.concatenate(tex) if tex else np.zeros(4, np.uint8)
        self.obj = np.asarray(rows, dtype=np.int64)
        self.radius = np.asarray(radius, dtype=np.float32)
        self.bounds_center = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
        self.bounds_radius = np.asarray(bradius, dtype=np.float32)

    def ids_of(self, labels) -> np.ndarray:
        return np.asarray([self.label_to_id[l] for l in labels], dtype=np.int32)
