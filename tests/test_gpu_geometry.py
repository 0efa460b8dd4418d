"""The pose geometry kernels (csrc/geometry.hip: hp_pose_prep, hp_pose_prep_views, hp_pose_update, hp_tco_init_autodepth) case by case
against the float64 reference (tests/geometry_ref.py), on the case tables of geometry_ref.  Needs a real MI355X: ``pytest -m gpu``.

The entry points are called through the C ABI, because every output is pre-filled with 7 (``happypose_amd.ops`` allocates its own),
some outputs are null and some ids lie outside their tables on the device; ``ops`` is run next to it and must return the same bits.

Stated tolerances (none is a literal here):
* continuous outputs: ``|got - ref| <= 4 x e x S``, ``e`` = geometry_yardstick.MEASURED_F32_ERROR, the error of a float32 evaluation of
  the definition in the kernel's order of operations (re-measured on the CPU by tests/test_geometry_reference.py), ``S`` the scale
  stated in geometry_yardstick's docstring; copies are compared exactly;
* the finiteness mask of every output equals the reference's (non-finite poses, the degenerate look-at, ids outside their tables);
* the identities (a permutation of all points, the K stride, view 0 against the single-view launch, 65 launches of 1, a launch with
  and without an odd hypothesis, null outputs) are bit for bit.
Every case proves on the CPU (tests/test_geometry_reference.py) that it reaches the path it is named after."""

import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import geometry_ref as R  # noqa: E402
import geometry_yardstick as Y  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
WORST = Y.Worst()  # (kernel, quantity) -> worst |got - ref| / (e x S) seen, printed by the tests
PREP_OUT = ("TCO", "tCR", "TCV_O", "boxes_rend", "boxes_crop", "K_crop", "K_crop_main")
_STORES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _d(a, dev):
    return None if a is None else torch.as_tensor(np.array(a), device=dev)  # a copy: the shared tables are read-only


def _store(case, dev):
    """The mesh store of a case's point table: the three objects of 300, 257 and 40 vertices, padded by the store itself, or the
    300-vertex objects of a planted case."""
    from test_gpu_kernels import _store_from_points

    key = case.table.tobytes()
    if key not in _STORES:
        base = R.table_of(R.base_objects())
        objs = list(R.base_objects()) if np.array_equal(case.table, base) else list(case.table)
        st = _store_from_points(objs, dev)
        assert st.n_pad == R.N_PAD and np.array_equal(np.asarray(st.mesh_db.points, np.float32), case.table)
        _STORES[key] = st
    return _STORES[key]


def _report(kernel):
    print("WORST", {k: round(v, 3) for k, v in WORST.items() if k[0] == kernel})


def _bits(a, b):
    return Y._same_bits(a, b)


# ---------------------------------------------------------------------------------------------------------------- hp_pose_prep
def _prep(case, dev, null=(), b=None, first=0, ids_main=None):
    """One launch on hypotheses ``first .. first + b`` of the case -> dict of numpy outputs, None for the null ones (``null``)."""
    from happypose_amd._ffi import check, lib, ptr, stream_ptr

    st = _store(case, dev)
    b = case.b if b is None else b
    sl = slice(first, first + b)
    nvt = 1 + len(R.VIEW_OFFSETS[case.mv])
    V = nvt - case.skip
    T, K, im, ob = _d(case.TCO[sl], dev), _d(case.K, dev), _d(case.im_ids[sl], dev), _d(case.obj_ids[sl], dev)
    i_main, i_extra = _d(case.ids_main if ids_main is None else ids_main, dev), (_d(case.ids_extra, dev) if nvt > 1 else None)
    shapes = dict(TCO=(b, 4, 4), tCR=(b, 3), TCV_O=(b, V, 4, 4), boxes_rend=(b, 4), boxes_crop=(b, 4), K_crop=(b, V, 3, 3), K_crop_main=(b, 3, 3))
    o = {k: None if k in null else torch.full(s, SENTINEL, device=dev) for k, s in shapes.items()}
    args = [C.c_int(case.normalize), ptr(T), ptr(K), len(case.K), ptr(im), ptr(ob), ptr(i_main), len(i_main), ptr(i_extra),
            case.n_extra if nvt > 1 else 0, case.im_size[0], case.im_size[1], case.crop_size[0], case.crop_size[1], C.c_float(case.lamb),
            ptr(o["TCO"]), ptr(o["tCR"]), ptr(o["TCV_O"]), ptr(o["boxes_rend"]), ptr(o["boxes_crop"]), ptr(o["K_crop"])]
    with torch.cuda.device(dev):
        if case.skip:
            check(lib().hp_pose_prep_views(st.handle, b, V, case.mv, 1, *args, ptr(o["K_crop_main"]), stream_ptr(dev)), "hp_pose_prep_views")
        else:
            check(lib().hp_pose_prep(st.handle, b, V, case.mv, *args, stream_ptr(dev)), "hp_pose_prep")
    out = {k: None if v is None else v.cpu().numpy() for k, v in o.items()}
    if not case.skip:
        assert (out["K_crop_main"] == SENTINEL).all()  # no argument of hp_pose_prep: never written
        out["K_crop_main"] = out["K_crop"][:, 0]
    for k, v in out.items():  # everything handed over is overwritten
        assert v is None or not (v == SENTINEL).any(), (case.name, k, "an element was not written")
    return out


def _same_prep(a, b, keys=PREP_OUT, rows=None):
    for k in keys:
        if a[k] is not None and b[k] is not None:
            x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
            assert _bits(x, y), k


def _ops_prep(case, dev):
    from happypose_amd import ops

    out = ops.pose_prep(_store(case, dev), torch.as_tensor(np.array(case.TCO)), torch.as_tensor(np.array(case.K)), _d(case.im_ids, dev),
                        _d(case.obj_ids, dev), case.im_size, case.crop_size, multiview_type=R.MV_NAME[case.mv], normalize=bool(case.normalize),
                        n_points=case.n_main, n_points_extra=case.n_extra, lamb=case.lamb, remove_TCO_rendering=bool(case.skip))
    return {k: out[k].cpu().numpy() for k in PREP_OUT}


@pytest.mark.parametrize("name", R.PREP_REGULAR)
def test_pose_prep(dev, name):
    case, ref = R.prep_case(name), R.prep_ref(name)
    got = _prep(case, dev)
    Y.check_prep(got, ref, case, WORST)
    _same_prep(got, _ops_prep(case, dev))  # happypose_amd.ops makes the same launch
    if case.mv:  # view 0 of a multi-view launch is the single-view launch
        single = _prep(case.replace(mv=0, skip=0), dev)
        _same_prep(got, single, ("TCO", "tCR", "boxes_rend", "boxes_crop", "K_crop_main"))
        if not case.skip:
            assert _bits(got["TCV_O"][:, 0], single["TCV_O"][:, 0]) and _bits(got["K_crop"][:, 0], single["K_crop"][:, 0])
    if case.n_main == R.N_PAD:  # all points: any order of the ids gives the same boxes
        perm = np.random.RandomState(3).permutation(R.N_PAD).astype(np.int32)
        _same_prep(got, _prep(case, dev, ids_main=perm))
    _report("pose_prep")


@pytest.mark.parametrize("name", ["front3_b65_portrait", "skip5_b65_raw_portrait"])
def test_pose_prep_launch_of_65_is_65_launches_of_1(dev, name):
    case = R.prep_case(name)
    got = _prep(case, dev)
    for i in range(case.b):
        one = _prep(case, dev, b=1, first=i)
        _same_prep({k: v[i:i + 1] for k, v in got.items()}, one)


@pytest.mark.parametrize("name", ["front3_b65_portrait", "skip3_b3", "tco_b1"])
def test_pose_prep_null_outputs(dev, name):
    """Each optional output null in turn, then all of them: the others do not change (and _prep finds no unwritten element)."""
    case = R.prep_case(name)
    full = _prep(case, dev)
    optional = ("TCO", "tCR", "TCV_O", "boxes_rend", "boxes_crop")
    for null in [(k,) for k in optional] + [optional]:
        got = _prep(case, dev, null=null)
        assert all(got[k] is None for k in null)
        _same_prep(full, got)


@pytest.mark.parametrize("name", R.PREP_ODD)
def test_pose_prep_non_finite_and_degenerate(dev, name):
    case, ref = R.prep_case(name), R.prep_ref(name)
    i, _, plain = case.odd
    got = _prep(case, dev)
    Y.check_prep(got, ref, case, WORST)  # the finiteness mask is the reference's, the finite values within the bounds
    others = [k for k in range(case.b) if k != i]
    _same_prep(got, _prep(case.replace(TCO=plain), dev), rows=others)
    _same_prep(got, _ops_prep(case, dev))
    _report("pose_prep")


@pytest.mark.parametrize("field,value", R.PREP_BAD_IDS)
def test_pose_prep_bad_device_ids(dev, field, value):
    case, base = R.prep_bad_id_case(field, value)
    got, good = _prep(case, dev), _prep(base, dev)
    for k in PREP_OUT:
        assert np.isnan(got[k][1]).all(), k
    _same_prep(got, good, rows=[0, 2])
    Y.check_prep(got, R.ref_pose_prep(case), case, WORST)


# -------------------------------------------------------------------------------------------------------------- hp_pose_update
def _update(case, dev, K_crop=None, b=None, first=0):
    from happypose_amd._ffi import check, lib, ptr, stream_ptr

    b = case.b if b is None else b
    sl = slice(first, first + b)
    Kc = np.ascontiguousarray((case.K_crop if K_crop is None else K_crop)[sl])
    T, K, p, tcr = _d(case.TCO[sl], dev), _d(Kc, dev), _d(case.pose9[sl], dev), _d(None if case.tCR is None else case.tCR[sl], dev)
    out = torch.full((b, 4, 4), SENTINEL, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_pose_update(b, ptr(T), ptr(K), Kc[0].size, ptr(p), ptr(tcr), ptr(out), stream_ptr(dev)), "hp_pose_update")
    return out.cpu().numpy()


@pytest.mark.parametrize("name", R.UPDATE_CASES)
def test_pose_update(dev, name):
    from happypose_amd import ops

    case = R.update_case(name)
    got = _update(case, dev)
    Y.check_update(got, R.ref_pose_update(case), case, WORST)
    via_ops = ops.pose_update(_d(case.TCO, dev), _d(case.K_crop, dev), _d(case.pose9, dev), _d(case.tCR, dev))
    assert _bits(got, via_ops.cpu().numpy())
    if case.views:  # [b,3,3] and view 0 of [b,4,3,3]
        assert _bits(got, _update(case, dev, K_crop=case.K_crop[:, 0]))
    if case.b == 65:
        for i in (0, 1, 63, 64):
            assert _bits(got[i:i + 1], _update(case, dev, b=1, first=i))
    _report("pose_update")


# -------------------------------------------------------------------------------------------------------- hp_tco_init_autodepth
def _init(case, dev, n=None, first=0):
    from happypose_amd._ffi import check, lib, ptr, stream_ptr

    st = _store(case, dev)
    n = case.n if n is None else n
    sl = slice(first, first + n)
    own = lambda a: a if a is None or len(a) != case.n else a[sl]  # noqa: E731  per-hypothesis tables follow the slice
    boxes, R_ = _d(case.boxes if case.box_ids is not None else own(case.boxes), dev), _d(case.R if case.rot_ids is not None else own(case.R), dev)
    K, im, ob = _d(case.K, dev), _d(case.im_ids[sl], dev), _d(case.obj_ids[sl], dev)
    bid, rid, pid = _d(None if case.box_ids is None else case.box_ids[sl], dev), _d(None if case.rot_ids is None else case.rot_ids[sl], dev), _d(case.point_ids, dev)
    out = torch.full((n, 4, 4), SENTINEL, device=dev)
    with torch.cuda.device(dev):
        check(lib().hp_tco_init_autodepth(st.handle, n, ptr(boxes), len(boxes), ptr(bid), ptr(K), len(case.K), ptr(im), ptr(ob), ptr(R_),
                                          0 if R_ is None else len(R_), ptr(rid), ptr(pid), case.n_points or 0, ptr(out), stream_ptr(dev)),
              "hp_tco_init_autodepth")
    got = out.cpu().numpy()
    assert not (got == SENTINEL).any()
    return got


@pytest.mark.parametrize("name", R.INIT_CASES)
def test_tco_init_autodepth(dev, name):
    from happypose_amd import ops

    case = R.init_case(name)
    got = _init(case, dev)
    Y.check_init(got, R.ref_tco_init(case), case, WORST)
    via_ops = ops.tco_init_autodepth(_store(case, dev), torch.as_tensor(np.array(case.boxes)), torch.as_tensor(np.array(case.K)), _d(case.im_ids, dev),
                                     _d(case.obj_ids, dev), R=None if case.R is None else torch.as_tensor(np.array(case.R)),
                                     box_ids=_d(case.box_ids, dev), rot_ids=_d(case.rot_ids, dev), n_points=case.n_points)
    assert _bits(got, via_ops.cpu().numpy())
    if case.n == 65:
        for i in (0, 1, 63, 64):
            assert _bits(got[i:i + 1], _init(case, dev, n=1, first=i))
    if case.point_ids is not None and case.n_points == R.N_PAD:  # all points: with and without the id list, and in any order
        assert _bits(got, _init(case.replace(point_ids=None, n_points=None), dev))
    _report("tco_init")


@pytest.mark.parametrize("field,value", R.INIT_BAD_IDS)
def test_tco_init_bad_device_ids(dev, field, value):
    case, base = R.init_bad_id_case(field, value)
    got, good = _init(case, dev), _init(base, dev)
    keep = np.arange(case.n) != 1
    assert np.isnan(got[1]).all() and _bits(got[keep], good[keep])
    Y.check_init(got, R.ref_tco_init(case), case, WORST)
