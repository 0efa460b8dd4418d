"""CPU tests of the pose geometry reference (tests/geometry_ref.py), of the case tables it shares with tests/test_gpu_geometry.py and
of the float32 yardstick and comparison functions (tests/geometry_yardstick.py).

* The float64 reference reproduces the reference project's own recorded outputs (goldens G4 and G7) within 4x the float32 yardstick:
  the goldens are float32 results of another order of operations, what the GPU tests allow a kernel.
* It agrees with the float32 restatement ``oracle.geometry`` on every regular case, within the same bound.
* Every case reaches the path it is named after.
* The yardstick's figures are re-measured.
* Teeth: the comparison functions fail on a reference with one deliberate mistake per failure class."""

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import geometry_ref as R  # noqa: E402
import geometry_yardstick as Y  # noqa: E402

F = np.float32
GOLDEN = Path(__file__).resolve().parent / "golden"
KEYS = ("TCO", "tCR", "TCV_O", "boxes_rend", "boxes_crop", "K_crop", "K_crop_main")


def _as_got(ref):
    """A reference rounded to float32: what a perfect kernel would return."""
    with np.errstate(all="ignore"):
        return {k: np.asarray(ref[k]).astype(F) for k in KEYS}


# ------------------------------------------------------------------------------------------------------------------- goldens
def test_reference_reproduces_golden_g7():
    g = np.load(GOLDEN / "g7_iteration.npz")
    b, n = g["pts"].shape[:2]
    ar = np.arange(b, dtype=np.int32)
    case = R.Case("g7", "the reference project's recorded refiner iteration", b=b, mv=0, skip=0, normalize=1, im_size=(480, 640), crop_size=(240, 320),
                  lamb=1.4, K=g["K"], im_ids=ar, obj_ids=ar, TCO=g["T"], table=g["pts"], ids_main=np.arange(n), ids_extra=np.arange(1), n_main=n,
                  n_extra=1)
    ref = R.ref_pose_prep(case)
    got = dict(TCO=g["T_norm"], tCR=g["T_norm"][:, :3, 3], TCV_O=g["T_norm"][:, None], boxes_rend=g["boxes_rend"], boxes_crop=g["boxes_crop"],
               K_crop=g["K_crop"][:, None], K_crop_main=g["K_crop"])
    worst = Y.Worst()
    Y.check_prep(got, ref, case, worst)
    up = R.Case("g7_update", "", b=b, TCO=g["T_norm"], K_crop=g["K_crop"], pose9=g["pose9"], tCR=np.ascontiguousarray(g["T_norm"][:, :3, 3]), views=0)
    Y.check_update(g["T_out"], R.ref_pose_update(up), up, worst)
    print("WORST", {k: round(v, 3) for k, v in worst.items()})


def test_reference_reproduces_golden_g4():
    g = np.load(GOLDEN / "g4_pose_update.npz")
    b = len(g["T"])
    worst = Y.Worst()
    for tcr, key in ((g["tCR"], "upd_ref"), (None, "upd_cosy")):
        case = R.Case("g4", "", b=b, TCO=g["T"], K_crop=g["K_crop"], pose9=g["pose9"], tCR=tcr, views=0)
        Y.check_update(g[key], R.ref_pose_update(case), case, worst)
    ar = np.arange(b, dtype=np.int32)
    for Rg, key in ((g["Rg"], "init_R"), (None, "init_zup")):
        case = R.Case("g4_init", "", n=b, boxes=g["det_boxes"], K=g["K"], im_ids=ar, obj_ids=ar, R=Rg, box_ids=None, rot_ids=None, point_ids=None,
                      n_points=None, table=g["mpts"])
        Y.check_init(g[key], R.ref_tco_init(case), case, worst)
    print("WORST", {k: round(v, 3) for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------------ the float32 restatement
def _oracle_prep(case):
    from oracle import geometry as G

    b, skip = case.b, case.skip
    nvt = 1 + len(R.VIEW_OFFSETS[case.mv])
    Tn = G.normalize_T(case.TCO) if case.normalize else np.array(case.TCO)
    tCR = Tn[:, :3, 3]
    views = [Tn[:, None]]
    if nvt > 1:
        views.append(G.make_TCO_multiview(Tn, tCR, R.MV_NAME[case.mv], nvt, remove_TCO_rendering=True))
        if not skip:  # and the call the estimators make: the identity view first
            np.testing.assert_array_equal(G.make_TCO_multiview(Tn, tCR, R.MV_NAME[case.mv], nvt), np.concatenate(views, 1))
    TV = np.concatenate(views, 1)
    Kb = case.K[case.im_ids]
    pts = case.table[case.obj_ids]
    Kc, boxes = [], []
    for v in range(nvt):
        ids = case.ids_main if v == 0 else case.ids_extra
        br, bc = G.crop_boxes_from_pose(pts[:, ids], Kb, TV[:, v], TV[:, v, :3, 3], case.im_size, lamb=case.lamb)
        Kc.append(G.get_K_crop_resize(Kb, bc, case.im_size, case.crop_size))
        boxes.append((br, bc))
    Kc = np.stack(Kc, 1)
    return dict(TCO=Tn, tCR=tCR, TCV_O=TV[:, skip:], boxes_rend=boxes[0][0], boxes_crop=boxes[0][1], K_crop=Kc[:, skip:], K_crop_main=Kc[:, 0])


@pytest.mark.parametrize("name", R.PREP_REGULAR)
def test_prep_reference_agrees_with_the_float32_restatement(name):
    case = R.prep_case(name)
    Y.check_prep(_oracle_prep(case), R.prep_ref(name), case, Y.Worst())


@pytest.mark.parametrize("name", R.UPDATE_CASES)
def test_update_reference_agrees_with_the_float32_restatement(name):
    from oracle import geometry as G

    case = R.update_case(name)
    K0 = case.K_crop.reshape(case.b, -1)[:, :9].reshape(case.b, 3, 3)
    got = G.update_pose(case.TCO, K0, case.pose9, case.TCO[:, :3, 3] if case.tCR is None else case.tCR)
    Y.check_update(got, R.ref_pose_update(case), case, Y.Worst())


@pytest.mark.parametrize("name", R.INIT_CASES)
def test_init_reference_agrees_with_the_float32_restatement(name):
    from oracle import geometry as G

    case = R.init_case(name)
    n = case.n
    boxes = case.boxes[np.arange(n) if case.box_ids is None else case.box_ids]
    K = case.K[case.im_ids]
    pid = np.arange(R.N_PAD) if case.point_ids is None else case.point_ids
    pts = case.table[case.obj_ids][:, pid]
    if case.R is None:
        got = G.TCO_init_from_boxes_zup_autodepth(boxes, pts, K)
    else:
        got = G.TCO_init_from_boxes_autodepth_with_R(boxes, pts, K, case.R[np.arange(n) if case.rot_ids is None else case.rot_ids])
    Y.check_init(got, R.ref_tco_init(case), case, Y.Worst())


# ------------------------------------------------------------------------------------------------------ every case reaches its path
def test_the_tables_cover_the_listed_paths():
    cases = [R.prep_case(n) for n in R.PREP_CASES]
    assert {c.mv for c in cases} == {0, 1, 3, 5}
    assert {(c.mv, c.skip) for c in cases if c.skip} == {(3, 1), (5, 1)}
    assert {c.normalize for c in cases} == {0, 1} and {c.lamb for c in cases} == {1.4, 1.0}
    assert {c.b for c in cases} >= {1, 3, 65}
    assert {c.n_main for c in cases} >= set(R.MAIN_EDGES) and {c.n_extra for c in cases if c.mv} >= set(R.EXTRA_EDGES)
    assert any(c.n_main != c.n_extra for c in cases if c.mv)
    assert {(c.im_size, c.crop_size) for c in cases} == {((480, 640), (240, 320)), ((640, 480), (320, 240)), ((37, 53), (16, 24))}
    assert any(c.im_size[0] > c.im_size[1] and c.crop_size[0] > c.crop_size[1] for c in cases)  # portrait image and portrait crop
    t = cases[0].table
    assert t.shape == (3, 300, 3) and R.N_PAD % 256 != 0
    for o, n in enumerate(R.OBJECT_SIZES):  # the padded rows repeat vertices of the object
        assert np.array_equal(t[o, :n], R.base_objects()[o]) and all((t[o, j] == t[o, :n]).all(1).any() for j in range(n, 300))
    for c in cases:
        K = c.K
        assert len(K) == 2 and (K[:, 0, 0] != K[:, 1, 1]).all() and (K[0] != K[1]).any()
        assert (abs(K[:, 0, 2] - (c.im_size[1] - 1) / 2) > 0.005 * c.im_size[1]).all()  # off-centre principal points
        if c.b >= 3 and not c.planted:
            assert list(c.im_ids[:3]) == [1, 0, 1] and list(c.obj_ids) != sorted(c.obj_ids)  # permuted ...
            assert c.b == 3 or len(set(c.obj_ids.tolist())) < c.b                            # ... and repeating
    ups = [R.update_case(n) for n in R.UPDATE_CASES]
    assert {u.views for u in ups} == {0, 4} and {u.b for u in ups} == {1, 3, 65}
    assert any(u.tCR is None for u in ups)
    assert any(u.tCR is not None and np.array_equal(u.tCR, u.TCO[:, :3, 3]) for u in ups)
    assert any(u.tCR is not None and not np.array_equal(u.tCR, u.TCO[:, :3, 3]) for u in ups)
    assert any((u.TCO[:, 3] != (0, 0, 0, 1)).any() for u in ups)
    for u in ups:
        if u.views:
            assert (u.K_crop[:, 1:] == 7).all()
    inits = [R.init_case(n) for n in R.INIT_CASES]
    for attr in ("R", "box_ids", "rot_ids", "point_ids"):
        assert {getattr(c, attr) is None for c in inits} == {True, False}, attr
    big = R.init_case("tables_b65")
    assert big.n == 65 and len(big.boxes) == 2 and len(big.R) == 3 and set(big.box_ids) == {0, 1} and set(big.rot_ids) == {0, 1, 2}
    assert {c.n_points for c in inits} >= set(R.MAIN_EDGES)


@pytest.mark.parametrize("name", R.PREP_CASES)
def test_prep_case_reaches_its_path(name):
    case, ref = R.prep_case(name), R.prep_ref(name)
    nvt = 1 + len(R.VIEW_OFFSETS[case.mv])
    for k, v, coord, j in case.planted:  # the planted point defines the box, by pixels
        col = ref["uv"][k][v][:, coord % 2]
        order = np.sort(col)
        assert (col.argmin() if coord < 2 else col.argmax()) == j, (k, v, coord, j)
        if len(col) > 1:
            assert (order[1] - order[0] if coord < 2 else order[-1] - order[-2]) > 5.0
    if case.planted:
        want = set(R.plant_positions(case.n_extra if name.startswith("plant_extra") else case.n_main))
        assert {j for *_, j in case.planted} == want
    if name.startswith("plant_main"):
        assert {(c, j) for _, _, c, j in case.planted} == {(c, j) for c in range(4) for j in R.plant_positions(case.n_main)}
    if name == "behind_b3":
        assert (ref["z_min"] < R.Z_MIN).any() and (ref["cz"] > R.Z_MIN).all()
    if name == "ref_behind_b3":
        assert (ref["cz"][:, 0] < R.Z_MIN).all() and (ref["cz"][:, 1:] < R.Z_MIN).any() and (ref["cz"] < 0).any()
    if "portrait" in name:
        assert case.im_size[0] > case.im_size[1]
    if case.regular:
        assert np.isfinite(ref["cross"]).all() and (ref["cross"] >= 1e-5).all()
        for k in KEYS:
            assert np.isfinite(ref[k]).all(), k
        if nvt > 1:  # the look-at views look at the reference point, from one radius (view 1) or sqrt(2) radii away
            tv = ref["TCV_O"][:, 1 - case.skip:, :3, 3]
            rad = np.linalg.norm(ref["tCR"], axis=1)
            assert np.abs(tv[..., :2]).max() <= 1e-12
            assert np.allclose(tv[:, 0, 2], rad, rtol=1e-12) and np.allclose(tv[:, 1:, 2], np.sqrt(2) * rad[:, None], rtol=1e-12)
    else:
        i, kind, plain = case.odd
        others = [k for k in range(case.b) if k != i]
        for k in KEYS:
            assert np.isfinite(ref[k][others]).all(), k
        if kind.startswith("deg"):
            assert ref["cross"][i] == 0.0 and np.isfinite(case.TCO[i]).all()
            assert np.isnan(ref["TCV_O"][i, 1 - case.skip:, :3]).all() and np.isfinite(ref["TCV_O"][i, :, 3]).all()
            assert np.isfinite(ref["boxes_crop"][i]).all() and np.isfinite(ref["K_crop_main"][i]).all()  # the identity view is regular
            assert np.isnan(ref["K_crop"][i, 1 - case.skip:, 0, 0]).all()
        else:
            assert not np.isfinite(case.TCO[i]).all() and np.isfinite(plain).all()
            assert np.array_equal(ref["TC0_CV"][i], np.tile(np.eye(4), (nvt, 1, 1)))  # the identity as every look-at camera
            assert np.isnan(ref["boxes_rend"][i]).all() and np.isnan(ref["boxes_crop"][i]).all() and np.isnan(ref["K_crop"][i, :, 0, 0]).all()
            if kind == "nan_bottom":  # non-finite among entries 12..15 only
                assert np.isfinite(case.TCO[i, :3]).all() and not case.normalize
                assert np.isnan(ref["TCV_O"][i, :, :, 2]).all() and np.isfinite(ref["TCV_O"][i, :, :, [0, 1, 3]]).all()


@pytest.mark.parametrize("field,value", R.PREP_BAD_IDS)
def test_prep_bad_id_case(field, value):
    case, base = R.prep_bad_id_case(field, value)
    ref, good = R.ref_pose_prep(case), R.prep_ref(base.name)
    for k in KEYS:
        assert np.isnan(ref[k][1]).all() and np.array_equal(ref[k][[0, 2]], good[k][[0, 2]])


@pytest.mark.parametrize("name", R.UPDATE_CASES)
def test_update_case_reaches_its_path(name):
    case = R.update_case(name)
    ref = R.ref_pose_update(case)
    assert np.isfinite(ref).all()
    x, y = case.pose9[:, :3].astype(np.float64), case.pose9[:, 3:6].astype(np.float64)
    sin = np.linalg.norm(np.cross(x, y), axis=1) / (np.linalg.norm(x, axis=1) * np.linalg.norm(y, axis=1))
    assert (abs(np.linalg.norm(x, axis=1) - 1) > 1e-3).any()
    if name == "collinear_b65":
        assert (sin < 0.21).all() and (sin > 0.19).all()
    else:
        assert (sin > 0.02).all()
    np.testing.assert_array_equal(ref[:, 3], case.TCO[:, 3])
    Rm = ref[:, :3, :3] @ np.linalg.inv(case.TCO[:, :3, :3].astype(np.float64))  # dR is a rotation
    assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and (np.linalg.det(Rm) > 0).all()


@pytest.mark.parametrize("name", R.INIT_CASES)
def test_init_case_reaches_its_path(name):
    case = R.init_case(name)
    ref = R.ref_tco_init(case)
    assert np.isfinite(ref["TCO"]).all()
    for k, coord, j in case.planted:
        col = ref["X"][k][:, coord % 2]
        assert (col.argmin() if coord < 2 else col.argmax()) == j
        order = np.sort(col)
        if len(col) > 1:
            assert (order[1] - order[0] if coord < 2 else order[-1] - order[-2]) > 0.1
    if case.planted:
        assert {(c, j) for _, c, j in case.planted} == {(c, j) for c in range(4) for j in R.plant_positions(case.n_points)}


@pytest.mark.parametrize("field,value", R.INIT_BAD_IDS)
def test_init_bad_id_case(field, value):
    case, base = R.init_bad_id_case(field, value)
    ref, good = R.ref_tco_init(case)["TCO"], R.ref_tco_init(base)["TCO"]
    keep = np.arange(case.n) != 1
    assert np.isnan(ref[1]).all() and np.array_equal(ref[keep], good[keep])


# ------------------------------------------------------------------------------------------------------------------- yardstick
def test_yardstick_figures_are_the_measured_ones():
    measured = Y.measure()
    print({k: float(f"{v:.3g}") for k, v in measured.items()})
    assert set(measured) == set(Y.MEASURED_F32_ERROR)
    for k, v in measured.items():
        assert v == pytest.approx(Y.MEASURED_F32_ERROR[k], rel=6e-3), k  # recorded to three digits
        assert f"{k} {Y.MEASURED_F32_ERROR[k]:.3g}".replace("e-07", "e-7").replace("e-08", "e-8").replace("e-06", "e-6") in " ".join(Y.__doc__.split())


def test_a_float32_evaluation_passes_the_gpu_comparison():
    """What the bound is made for: the float32 evaluation itself is within 1x, so within the 4x a kernel is allowed."""
    worst = Y.Worst()
    for name in R.PREP_REGULAR:
        case, ref = R.prep_case(name), R.prep_ref(name)
        Y.check_prep(Y.prep_f32(case, ref), ref, case, worst)
    for name in R.UPDATE_CASES:
        case = R.update_case(name)
        Y.check_update(Y.update_f32(case), R.ref_pose_update(case), case, worst)
    for name in R.INIT_CASES:
        case = R.init_case(name)
        Y.check_init(Y.init_f32(case), R.ref_tco_init(case), case, worst)
    assert max(worst.values()) <= 1.0 + 6e-3


# ----------------------------------------------------------------------------------------------------------------------- teeth
@pytest.mark.parametrize("name,mutation", [
    ("plant_main_300", "drop_last_point"), ("plant_main_257", "drop_last_point"), ("plant_main_65", "drop_last_point"),
    ("plant_main_255", "drop_wave"), ("plant_main_300", "drop_wave"),
    ("front3_b65_portrait", "swap_views_2_3"), ("skip5_b65_raw_portrait", "swap_views_2_3"),
    ("skip3_b3", "kcrop_main_slot0"), ("skip5_b65_raw_portrait", "kcrop_main_slot0"),
    ("front3_b65_portrait", "r_inverted"), ("skip5_b65_raw_portrait", "r_inverted"),
])
def test_teeth_pose_prep(name, mutation):
    case, ref = R.prep_case(name), R.prep_ref(name)
    Y.check_prep(_as_got(ref), ref, case, Y.Worst())  # the unmutated reference passes
    with pytest.raises(AssertionError):
        Y.check_prep(_as_got(R.ref_pose_prep(case, mutate=mutation)), ref, case, Y.Worst())


def test_teeth_pose_update_k_stride():
    case = R.update_case("k4x33_offset_b65")
    ref = R.ref_pose_update(case)
    Y.check_update(ref.astype(F), ref, case, Y.Worst())
    with pytest.raises(AssertionError):
        Y.check_update(R.ref_pose_update(case, mutate="k_stride_9").astype(F), ref, case, Y.Worst())


@pytest.mark.parametrize("name", ["tables_b65", "box_ids_only_b3", "zup_box_ids_b65"])
def test_teeth_tco_init_box_ids(name):
    case = R.init_case(name)
    ref = R.ref_tco_init(case)
    Y.check_init(ref["TCO"].astype(F), ref, case, Y.Worst())
    with pytest.raises(AssertionError):
        Y.check_init(R.ref_tco_init(case, mutate="box_ids_ignored")["TCO"].astype(F), ref, case, Y.Worst())


def test_teeth_finiteness_and_copies():
    """A NaN answered with a number (what fminf / fmaxf make of a non-finite pose), and a changed copy."""
    case, ref = R.prep_case("nan_rot"), R.prep_ref("nan_rot")
    got = _as_got(ref)
    Y.check_prep(got, ref, case, Y.Worst())
    bad = dict(got, boxes_rend=np.where(np.isnan(got["boxes_rend"]), F(np.inf), got["boxes_rend"]), K_crop=np.nan_to_num(got["K_crop"], nan=0.0))
    with pytest.raises(AssertionError):
        Y.check_prep(dict(got, K_crop=bad["K_crop"]), ref, case, Y.Worst())
    bad_tcr = got["tCR"].copy()
    bad_tcr[0, 0] = np.nextafter(bad_tcr[0, 0], F(9))
    with pytest.raises(AssertionError):
        Y.check_prep(dict(got, tCR=bad_tcr), ref, case, Y.Worst())
