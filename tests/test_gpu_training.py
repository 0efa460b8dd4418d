"""The trainers' forward-loss step on the device (csrc/train_hyp.hip, happypose_amd.training) against the float64 restatement
(tests/training_ref.py) and against the same quantities composed by hand from the predictor and happypose_amd.losses.

Bounds.  The kernels' poses and noise values are held to MARGIN = 4 x the distance of a float32 numpy evaluation of the same
formula from the float64 one ON THE INPUTS OF THE CASE (printed next to the error; CHANGELOG carries them), so that the order of
operations and the device's sine / cosine may differ by a few ulp while a wrong axis, sign or convention fails by orders of
magnitude.  Everything about the draw's determinism and the forward-loss composition is compared bit for bit."""

import sys
from collections import defaultdict
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import training_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def dev(a):
    return torch.as_tensor(a).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- hp_pose_add_noise: given noise ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,repeat", R.EXPLICIT_CASES)
def test_explicit_noise_against_the_float64_reference(n, repeat):
    from happypose_amd import ops

    TCO, noise = R.explicit_case(n, repeat)
    ref = R.add_noise(TCO, noise, repeat)
    bound = R.MARGIN * R.yardstick(R.add_noise(TCO, noise, repeat, np.float32), ref)
    out, back = ops.pose_add_noise(dev(TCO), noise=dev(noise), repeat=repeat, return_noise=True)
    got = out.cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"add_noise n = {n}, repeat = {repeat}: error {err:.3g} (bound {bound:.3g} = {R.MARGIN:g} x the float32 evaluation's)")
    assert got.shape == (n, 4, 4) and err <= bound, (err, bound)
    assert np.array_equal(got[:, 3], np.repeat(TCO, repeat, axis=0)[:, 3]) and np.array_equal(back.cpu().numpy(), noise)


def test_the_euler_convention_is_static_xyz():
    from happypose_amd import ops

    TCO = R.random_poses(np.random.RandomState(5), 2)
    noise = np.concatenate([R.BIG_ANGLES, np.zeros((2, 3), np.float32)], axis=1)
    ref = R.add_noise(TCO, noise)
    bound = R.MARGIN * R.yardstick(R.add_noise(TCO, noise, dtype=np.float32), ref)
    got = ops.pose_add_noise(dev(TCO), noise=dev(noise)).cpu().numpy().astype(np.float64)
    err, err_rxyz = np.abs(got - ref).max(), np.abs(got - R.add_noise(TCO, noise, axes="rxyz")).max()
    print(f"add_noise, angles of 0.4 .. 2.5 rad: error {err:.3g} (bound {bound:.3g}); distance from the rotating-axes convention {err_rxyz:.3g}")
    assert err <= bound and err_rxyz > 0.1
    assert np.array_equal(got[:, :3, 3], TCO[:, :3, 3].astype(np.float64))  # zero translation noise: untouched


# ---- hp_pose_add_noise: drawn noise ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drawn():
    from happypose_amd import ops

    TCO = dev(R.random_poses(np.random.RandomState(9), 257))
    out, noise = ops.pose_add_noise(TCO, R.EULER_DEG_STD, R.TRANS_STD, seed=R.SEED, return_noise=True)
    return TCO, out, noise


def test_drawn_noise_repeats_and_rows_depend_on_seed_and_row_alone(drawn):
    from happypose_amd import ops

    TCO, out, noise = drawn
    out2, noise2 = ops.pose_add_noise(TCO, R.EULER_DEG_STD, R.TRANS_STD, seed=R.SEED, return_noise=True)
    assert same_bits(out, out2) and same_bits(noise, noise2)
    sub, sub_noise = ops.pose_add_noise(TCO[100:164].contiguous(), R.EULER_DEG_STD, R.TRANS_STD, seed=R.SEED, row_offset=100, return_noise=True)
    assert same_bits(sub, out[100:164]) and same_bits(sub_noise, noise[100:164])
    other = ops.pose_add_noise(TCO, R.EULER_DEG_STD, R.TRANS_STD, seed=R.SEED + 1)
    assert not torch.equal(other, out)
    # n_hypotheses inside the launch: row i of a repeat = 3 call is pose i // 3 with the noise of row i
    rep, rep_noise = ops.pose_add_noise(TCO[:65].contiguous(), R.EULER_DEG_STD, R.TRANS_STD, seed=R.SEED, repeat=3, return_noise=True)
    assert same_bits(rep_noise, noise[:195])
    assert same_bits(rep, ops.pose_add_noise(TCO[:65].repeat_interleave(3, dim=0), noise=noise[:195].contiguous()))


def test_drawn_noise_against_the_philox_restatement(drawn):
    _, _, noise = drawn
    ref = R.draw_noise(257, R.SEED, 0, R.EULER_DEG_STD, R.TRANS_STD)
    bound = R.MARGIN * R.yardstick(R.draw_noise(257, R.SEED, 0, R.EULER_DEG_STD, R.TRANS_STD, np.float32), ref)
    err = np.abs(noise.cpu().numpy().astype(np.float64) - ref).max()
    print(f"drawn noise, 257 rows: error {err:.3g} (bound {bound:.3g} = {R.MARGIN:g} x the float32 evaluation's)")
    assert err <= bound, (err, bound)


def test_drawn_pose_is_the_explicit_path_fed_with_the_drawn_noise(drawn):
    from happypose_amd import ops

    TCO, out, noise = drawn
    assert same_bits(ops.pose_add_noise(TCO, noise=noise), out)


def test_a_zero_standard_deviation_leaves_that_part_bit_identical(drawn):
    from happypose_amd import ops

    TCO = drawn[0].clone()
    TCO[3, 0, 1] = -0.0  # a product with the identity, or an added zero, would lose the sign
    TCO[4, 1, 3] = -0.0
    t_only = ops.pose_add_noise(TCO, (0, 0, 0), R.TRANS_STD, seed=R.SEED)
    assert same_bits(t_only[:, :3, :3], TCO[:, :3, :3]) and not torch.equal(t_only[:, :3, 3], TCO[:, :3, 3])
    r_only = ops.pose_add_noise(TCO, R.EULER_DEG_STD, (0, 0, 0), seed=R.SEED)
    assert same_bits(r_only[:, :3, 3], TCO[:, :3, 3]) and not torch.equal(r_only[:, :3, :3], TCO[:, :3, :3])
    z_only = ops.pose_add_noise(TCO, (0, 0, 0), (0, 0, 0.05), seed=R.SEED)
    assert same_bits(z_only[:, :2, 3], TCO[:, :2, 3]) and same_bits(z_only[:, :3, :3], TCO[:, :3, :3])
    assert same_bits(ops.pose_add_noise(TCO, (0, 0, 0), (0, 0, 0), seed=R.SEED), TCO)


def test_in_place_gives_the_out_of_place_result(drawn):
    from happypose_amd import ops

    TCO, out, _ = drawn
    work = TCO.clone()
    res = ops.pose_add_noise(work, R.EULER_DEG_STD, R.TRANS_STD, seed=R.SEED, out=work)
    assert res.data_ptr() == work.data_ptr() and same_bits(work, out)


def test_argument_errors():
    from happypose_amd import ops

    TCO = dev(R.random_poses(np.random.RandomState(2), 6))
    with pytest.raises(ValueError):
        ops.pose_add_noise(TCO.cpu(), seed=1)
    with pytest.raises(ValueError):
        ops.pose_add_noise(TCO, noise=torch.zeros(6, 6))
    with pytest.raises(ValueError):
        ops.tco_init_from_boxes(torch.zeros(2, 4), torch.eye(3).expand(2, 3, 3))
    with pytest.raises(AssertionError):  # overlap with repeat > 1 is refused by the library before anything is launched
        ops.pose_add_noise(TCO[:2], seed=1, repeat=3, out=TCO)
    with pytest.raises(AssertionError):
        ops.pose_add_noise(TCO, (-1, 0, 0), seed=1)
    assert ops.pose_add_noise(TCO[:0], seed=1).shape == (0, 4, 4)


# ---- hp_tco_init_from_boxes ------------------------------------------------------------------------------------------------------
def test_tco_init_from_boxes_against_the_reference_golden(golden_dir):
    from happypose_amd import ops, training

    g = np.load(golden_dir / "g4_pose_update.npz")
    boxes, K = g["det_boxes"], g["K"]
    got = training.TCO_init_from_boxes((1.0, 1.0), dev(boxes), dev(K)).cpu().numpy()
    np.testing.assert_allclose(got, g["init_v0"], rtol=1e-6, atol=1e-6)  # the tolerance of tests/test_oracle_golden.py
    for z_range in ((1.0, 1.0), (0.3, 1.5)):
        ref = R.TCO_init_from_boxes(z_range, boxes, K)
        got = ops.tco_init_from_boxes(dev(boxes), dev(K), z_range).cpu().numpy()
        bound = max(R.MARGIN * R.yardstick(R.TCO_init_from_boxes(z_range, boxes, K, np.float32), ref), float(np.spacing(np.float32(np.abs(ref).max()))))
        err = np.abs(got.astype(np.float64) - ref).max()
        print(f"tco_init_from_boxes z_range = {z_range}: error {err:.3g} (bound {bound:.3g})")
        assert err <= bound
    # ids on the device are guarded in the kernel: a row whose id leaves its table is NaN, its neighbours are untouched
    im_ids = torch.tensor([0, 99, -1, 3, 15], dtype=torch.int32, device=DEV)
    box_ids = torch.tensor([5, 1, 2, 16, 0], dtype=torch.int32, device=DEV)
    got = ops.tco_init_from_boxes(dev(boxes), dev(K), im_ids=im_ids, box_ids=box_ids).cpu().numpy()
    assert np.isnan(got[[1, 2, 3]]).all()
    ref = R.TCO_init_from_boxes((1.0, 1.0), boxes[[5, 0]], K[[0, 15]], np.float32)
    np.testing.assert_allclose(got[[0, 4]], ref, rtol=1e-6, atol=1e-6)
    with pytest.raises(IndexError):  # ids still on the host are checked there
        ops.tco_init_from_boxes(dev(boxes), dev(K), im_ids=[0, 16], box_ids=[0, 1])


# ---- h_pose and megapose_forward_loss -----------------------------------------------------------------------------------------------
N_POINTS_LOSS = 64  # of the 8249 padded points per object
N_ITERATIONS = 2


@pytest.fixture(scope="module")
def world():
    from happypose_amd.mesh_store import MeshDataBase
    from happypose_amd.renderer import BatchRenderer
    from happypose_amd.synthetic import make_object_dataset, make_scene

    ds = make_object_dataset(2, seed=1, tex_size=256)
    renderer = BatchRenderer(ds, device=torch.device("cuda:0"))
    mesh_db = MeshDataBase.from_object_ds(ds).batched()
    sc = make_scene(n_detections=2, n_hypotheses=1, n_objects=2, seed=2)
    pts, K = np.asarray(mesh_db.points, np.float64), sc["K"][0].astype(np.float64)
    labels = [str(mesh_db.labels[i]) for i in sc["det_obj_ids"]]
    boxes = []
    for T, o in zip(sc["TCO_det"].astype(np.float64), sc["det_obj_ids"]):
        uv = (pts[o] @ T[:3, :3].T + T[:3, 3]) @ K.T
        uv = uv[:, :2] / uv[:, 2:]
        boxes.append([uv[:, 0].min(), uv[:, 1].min(), uv[:, 0].max(), uv[:, 1].max()])
    rgb = (sc["images"][0] * 255).astype(np.uint8)
    data = SimpleNamespace(rgbs=dev(np.stack([rgb, rgb[:, ::-1].copy()])), depths=None, K=dev(np.repeat(sc["K"], 2, axis=0)),
                           TCO=dev(sc["TCO_det"]), bboxes=dev(np.asarray(boxes, np.float32)),
                           object_datas=[SimpleNamespace(label=l) for l in labels])
    return SimpleNamespace(renderer=renderer, mesh_db=mesh_db.to(DEV), data=data, labels=labels)


def _weights(arch, n_in, seed):
    from happypose_amd.models import pose_model_param_shapes
    from happypose_amd.synthetic import predictor_weights

    return predictor_weights(pose_model_param_shapes(arch, n_in), seed=seed)


@pytest.fixture(scope="module")
def cosy(world):
    from happypose_amd.models import create_pose_model_cosypose

    return create_pose_model_cosypose(dict(backbone_str="resnet18"), world.renderer, state_dict=_weights("resnet18", 6, 1), max_batch=4)


@pytest.fixture(scope="module")
def mega(world):
    from happypose_amd.models import create_model_pose

    cfg = dict(backbone_str="vanilla_resnet34", n_rendered_views=4, multiview_type="front_3views", render_normals=True, render_depth=False,
               input_depth=False, predict_pose_update=True, depth_augmentation=False, depth_normalization_type="tCR_scale_clamp_center")
    return create_model_pose(cfg, world.renderer, state_dict=_weights("vanilla_resnet34", 27, 2), max_batch=4)


def _meters():
    from happypose_amd.training import AverageValueMeter

    return defaultdict(AverageValueMeter)


def _by_hand(world, model, dbg, n_hyp, megapose, **kw):
    """The predictor on ``debug_dict``'s hypotheses and ``losses.*`` on its outputs: per iteration the loss rows, the parts, and
    the backward of the rows with a given upstream gradient."""
    from happypose_amd import losses, ops

    B = 2
    hyp = dbg["hypotheses_TCO_init"]
    assert hyp.shape == (B, n_hyp, 4, 4)
    images = world.data.rgbs.float() / 255.0
    im_ids = torch.arange(B, dtype=torch.int32, device=DEV).repeat_interleave(n_hyp)
    labels = [l for l in world.labels for _ in range(n_hyp)]
    outputs = model(images=images, K=world.data.K, labels=labels, TCO=hyp.reshape(B * n_hyp, 4, 4), n_iterations=N_ITERATIONS, im_ids=im_ids, **kw)
    rows = []
    for n in range(N_ITERATIONS):
        o = outputs[f"iteration={n + 1}"]
        ran = dbg["outputs"][f"iteration={n + 1}"]
        pose = o.network_outputs["pose"]
        assert same_bits(pose, ran.network_outputs["pose"].detach()) and same_bits(o.TCO_input, ran.TCO_input)
        args = (dbg["TCO_possible_gt"], o.TCO_input, pose, o.K_crop, dbg["points"], o.tCR if megapose else None)
        if megapose:
            loss, data = losses.loss_refiner_CO_disentangled_reference_point(*args)
        else:
            loss, data = losses.loss_refiner_CO_disentangled(*args[:5]), None
        sym_ids = ops.loss_refiner_forward(*args)[2]
        rows.append(SimpleNamespace(loss=loss, data=data, grad=lambda up, a=args, s=sym_ids: ops.loss_refiner_backward(*a, s, up), ran=ran))
    return rows


@pytest.mark.parametrize("method,n_hyp", [("refiner_gt+noise", 1), ("refiner_gt+noise", 2), ("coarse_z_up+auto-depth", 1)])
def test_megapose_forward_loss_is_the_hand_composition(world, mega, method, n_hyp):
    from happypose_amd import training

    B, alpha = 2, 0.5
    cfg = training.TrainingConfig(hypotheses_init_method=method, n_hypotheses=n_hyp, n_points_loss=N_POINTS_LOSS, loss_alpha_pose=alpha)
    meters, dbg = _meters(), {}
    loss = training.megapose_forward_loss(mega, cfg, world.data, meters, world.mesh_db, N_ITERATIONS, dbg, seed=7)
    assert loss.is_cuda and loss.shape == () and loss.requires_grad
    assert set(meters) == R.megapose_meter_keys(N_ITERATIONS) and all(m.n == 1 for m in meters.values())
    assert dbg["points"].shape == (B * n_hyp, N_POINTS_LOSS, 3) and dbg["time_render"] == meters["time_render"].mean

    rows = _by_hand(world, mega, dbg, n_hyp, True, random_ambient_light=False)
    want = {}
    for n, r in enumerate(rows):
        want[f"loss_TCO-iter={n + 1}"] = r.loss.view(B, n_hyp).mean()
        for key in ("loss_orn", "loss_xy", "loss_z"):
            want[f"loss_TCO-iter={n + 1}-{key}"] = r.data[key].view(B, n_hyp).mean()
    losses_pose = torch.stack([r.loss.view(B, n_hyp) for r in rows]).permute(1, 2, 0)
    want["loss_TCO"] = losses_pose.mean(dim=(-1, -2)).mean()
    want["loss_total"] = (torch.zeros(B, n_hyp, N_ITERATIONS, device=DEV) + alpha * losses_pose).mean()
    for key, v in want.items():
        assert meters[key].mean == v.item(), (key, meters[key].mean, v.item())
    assert same_bits(loss.detach(), want["loss_total"])
    ref, _ = R.megapose_meters([r.loss.cpu().numpy() for r in rows], [{k: v.cpu().numpy() for k, v in r.data.items()} for r in rows], B, n_hyp, alpha)
    for key, v in ref.items():  # the float64 restatement of the formulas: float32 means of a few O(0.01 .. 1) values
        assert abs(meters[key].mean - v) <= 1e-6 * max(abs(v), 1.0), (key, meters[key].mean, v)
    assert np.isfinite(list(ref.values())).all() and ref["loss_total"] > 0

    loss.backward()
    up = torch.full((B * n_hyp,), alpha / (B * n_hyp * N_ITERATIONS), device=DEV)
    for r in rows:
        grad = r.ran.network_outputs["pose"].grad
        assert grad is not None and same_bits(grad, r.grad(up)) and bool((grad != 0).any())

    again = training.megapose_forward_loss(mega, cfg, world.data, _meters(), world.mesh_db, N_ITERATIONS, None, seed=7)
    assert same_bits(again.detach(), loss.detach())
    other = training.megapose_forward_loss(mega, cfg, world.data, _meters(), world.mesh_db, N_ITERATIONS, None, seed=8)
    assert not torch.equal(other.detach(), loss.detach())


@pytest.mark.parametrize("input_generator", ["fixed", "gt+noise", "fixed+trans_noise"])
def test_h_pose_is_the_hand_composition(world, cosy, input_generator):
    from happypose_amd import training

    B = 2
    cfg = training.CosyPoseTrainingConfig(n_points_loss=N_POINTS_LOSS, init_method="z-up+auto-depth")
    meters, dbg = _meters(), {}
    loss = training.h_pose(cosy, world.mesh_db, world.data, meters, cfg, n_iterations=N_ITERATIONS, input_generator=input_generator, seed=7,
                           debug_dict=dbg)
    assert loss.is_cuda and loss.shape == () and loss.requires_grad
    assert set(meters) == R.h_pose_meter_keys(N_ITERATIONS) and all(m.n == 1 for m in meters.values())

    rows = _by_hand(world, cosy, dbg, 1, False)
    want = {f"loss_TCO-iter={n + 1}": r.loss.mean() for n, r in enumerate(rows)}
    want["loss_TCO"] = want["loss_total"] = torch.cat([r.loss for r in rows]).mean()
    for key, v in want.items():
        assert meters[key].mean == v.item(), (key, meters[key].mean, v.item())
    assert same_bits(loss.detach(), want["loss_total"])
    ref, _ = R.h_pose_meters([r.loss.cpu().numpy() for r in rows])
    for key, v in ref.items():
        assert abs(meters[key].mean - v) <= 1e-6 * max(abs(v), 1.0), (key, meters[key].mean, v)
    assert np.isfinite(list(ref.values())).all() and ref["loss_total"] > 0

    loss.backward()
    up = torch.full((B,), 1.0 / (B * N_ITERATIONS), device=DEV)
    for r in rows:
        grad = r.ran.network_outputs["pose"].grad
        assert grad is not None and same_bits(grad, r.grad(up)) and bool((grad != 0).any())

    again = training.h_pose(cosy, world.mesh_db, world.data, _meters(), cfg, n_iterations=N_ITERATIONS, input_generator=input_generator, seed=7)
    assert same_bits(again.detach(), loss.detach())
    if input_generator == "fixed":  # what the reference's fixed generator is: the box initialisation at z = 1
        want_init = training.TCO_init_from_boxes((1.0, 1.0), world.data.bboxes, world.data.K)
        assert same_bits(dbg["hypotheses_TCO_init"][:, 0], want_init)
    else:
        other = training.h_pose(cosy, world.mesh_db, world.data, _meters(), cfg, n_iterations=N_ITERATIONS, input_generator=input_generator, seed=8)
        assert not torch.equal(other.detach(), loss.detach())


def test_hypotheses_of_every_method(world, cosy):
    from happypose_amd import ops, training

    store, B = cosy.store, 2
    gt = world.data.TCO
    cfg = training.TrainingConfig(n_hypotheses=3, n_points_loss=N_POINTS_LOSS)
    hyp = training.make_hypotheses("refiner_gt+noise", world.data, world.mesh_db, cfg, 5)
    assert hyp.shape == (B, 3, 4, 4) and same_bits(hyp, training.make_hypotheses("refiner_gt+noise", world.data, world.mesh_db, cfg, 5))
    # noisy copies of the ground truth at the reference's magnitudes: 15 degrees, centimetres
    dt = (hyp[:, :, :3, 3] - gt[:, None, :3, 3]).abs().max().item()
    dR = (hyp[:, :, :3, :3] - gt[:, None, :3, :3]).abs().max().item()
    assert 0 < dt < 0.5 and 0 < dR < 1.5
    cfg1 = training.TrainingConfig(hypotheses_init_method="coarse_z_up+auto-depth", n_hypotheses=1)
    zup = training.make_hypotheses("coarse_z_up+auto-depth", world.data, world.mesh_db, cfg1, 5, store=store)
    base = training.TCO_init_from_boxes_zup_autodepth(world.data.bboxes, store, world.data.K, labels=world.labels, n_points=200)
    assert zup.shape == (B, 1, 4, 4) and same_bits(zup[:, 0, :3, :3], base[:, :3, :3]) and not torch.equal(zup[:, 0, :3, 3], base[:, :3, 3])
    assert same_bits(zup[:, 0], ops.pose_add_noise(base, (0, 0, 0), (0.01, 0.01, 0.05), seed=training._seed(5, 1)))
    # the boxes are the ground truth's own: the z-up guess of another orientation still lands at the depth's order of magnitude
    ratio = base[:, 2, 3] / gt[:, 2, 3]
    assert bool(((ratio > 1 / 3) & (ratio < 3)).all()), ratio
    with pytest.raises(ValueError):
        training.make_hypotheses("coarse_z_up+auto-depth", world.data, world.mesh_db, cfg1, 5)
    with pytest.raises(TypeError):
        training.TCO_init_from_boxes_zup_autodepth(world.data.bboxes, world.mesh_db.points[:2], world.data.K, labels=world.labels)


def test_what_is_not_built_raises(world, cosy, mega):
    from happypose_amd import training

    for method in ("coarse_classif_multiview_paper", "coarse_classif_multiview_SO3_grid"):
        with pytest.raises(NotImplementedError):
            training.make_hypotheses(method, world.data, world.mesh_db, training.TrainingConfig(), 0)
        with pytest.raises(NotImplementedError):
            training.megapose_forward_loss(mega, training.TrainingConfig(hypotheses_init_method=method), world.data, _meters(), world.mesh_db, 1, None)
    with pytest.raises(ValueError):
        training.megapose_forward_loss(mega, training.TrainingConfig(hypotheses_init_method="fixed"), world.data, _meters(), world.mesh_db, 1, None)
    with pytest.raises(ValueError):
        training.h_pose(cosy, world.mesh_db, world.data, _meters(), training.CosyPoseTrainingConfig(n_points_loss=N_POINTS_LOSS), input_generator="nope")
    with pytest.raises(NotImplementedError):
        training.h_pose(cosy, world.mesh_db, world.data, _meters(), training.CosyPoseTrainingConfig(n_pose_dims=7))
    with pytest.raises(NotImplementedError):
        training.megapose_forward_loss(mega, training.TrainingConfig(), world.data, _meters(), world.mesh_db, 1, None, make_visualization=True)
    with pytest.raises(NotImplementedError):
        training.megapose_forward_loss(mega, training.TrainingConfig(random_ambient_light=True), world.data, _meters(), world.mesh_db, 1, None)
    cpu = SimpleNamespace(**{**vars(world.data), "TCO": world.data.TCO.cpu()})
    with pytest.raises(ValueError):
        training.h_pose(cosy, world.mesh_db, cpu, _meters(), training.CosyPoseTrainingConfig(n_points_loss=N_POINTS_LOSS))
