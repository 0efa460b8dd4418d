"""Training MegaPose's coarse classifier on the device: ``megapose_forward_loss`` with ``coarse_classif_multiview_paper`` and the
rendered-views-logits loss, and ``HeadTrainer`` on a network with a logits head and no pose head.

The step is compared bit for bit with its hand composition (``ops.coarse_hypotheses``, the model's forward,
``losses.renderings_confidence_loss``, the mean) and its gradient with float64.  The trainer is held to a float64 replay of head
backward + Adam with the bounds of tests/test_gpu_head_train.py (its module docstring derives them; ``_update_bound`` is
imported from there)."""

import math
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import coarse_hyp_ref as C  # noqa: E402
import head_train_ref as R  # noqa: E402
import test_gpu_head_train as H  # noqa: E402
import training_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = R.U
B, N_HYP, N_POINTS_LOSS, SEED, N_STEPS = 2, 3, 64, 7, 3
TEMPERATURE, ALPHA = 0.5, 0.75

dev, f64, same_bits, _meters = H.dev, H.f64, H.same_bits, H._meters
world = H.world  # 2 images and 2 objects from happypose_amd.synthetic, as in tests/test_gpu_training.py


def _model(world, arch, pose):
    from happypose_amd.models import create_model_pose, pose_model_param_shapes
    from happypose_amd.synthetic import predictor_weights

    mcfg = dict(backbone_str=arch, n_rendered_views=1, multiview_type="TCO", render_normals=True, render_depth=False, input_depth=False,
                predict_pose_update=pose, predict_rendered_views_logits=True, depth_augmentation=False,
                depth_normalization_type="tCR_scale_clamp_center")
    sd = predictor_weights(pose_model_param_shapes(arch, 9, pose_dim=9 if pose else 0, n_views_logits=1), seed=3)
    return create_model_pose(mcfg, world.renderer, state_dict=sd, max_batch=B * N_HYP)


@pytest.fixture(scope="module")
def coarse(world):
    return _model(world, "vanilla_resnet34", pose=False)  # the fc in front of the logits row is trained too


def _cfg(pose=False):
    from happypose_amd import training

    return training.TrainingConfig(hypotheses_init_method="coarse_classif_multiview_paper", n_hypotheses=N_HYP, n_points_loss=N_POINTS_LOSS,
                                   predict_pose_update=pose, predict_rendered_views_logits=True, n_rendered_views=1,
                                   renderings_logits_temperature=TEMPERATURE, loss_alpha_renderings_confidence=ALPHA)


def test_config_defaults_are_the_reference():
    from happypose_amd import training

    cfg = training.TrainingConfig()
    assert (cfg.n_rendered_views, cfg.renderings_logits_temperature, cfg.loss_alpha_renderings_confidence) == (1, 1.0, 1.0)


def test_coarse_step_is_the_hand_composition(world, coarse):
    from happypose_amd import losses, ops, training

    cfg = _cfg()
    meters, dbg = _meters(), {}
    loss = training.megapose_forward_loss(coarse, cfg, world.data, meters, world.mesh_db, 1, dbg, seed=SEED)
    assert loss.is_cuda and loss.shape == () and loss.requires_grad
    assert set(meters) == {"time_render", "loss_renderings_confidence", "loss_total"} and all(m.n == 1 for m in meters.values())
    assert list(meters) == ["time_render", "loss_renderings_confidence", "loss_total"]  # the reference's order of .add()

    # the hypotheses: one noisy ground truth per image, then the draw
    noisy = training.add_noise(world.data.TCO, cfg.init_euler_deg_std, cfg.init_trans_std, seed=training._seed(SEED, 1))
    hyp, ids, pos = ops.coarse_hypotheses(noisy, N_HYP, seed=training._seed(SEED, 4), n_rendered_views=1)
    assert same_bits(dbg["hypotheses_TCO_init"], hyp) and torch.equal(dbg["views_permutation"], ids) and same_bits(dbg["is_hypothesis_positive"], pos)
    ref_ids, ref_pos = C.draw(B, N_HYP, training._seed(SEED, 4))
    assert np.array_equal(ids.cpu().numpy(), ref_ids) and np.array_equal(pos.cpu().numpy(), ref_pos)
    got = training.make_hypotheses("coarse_classif_multiview_paper", world.data, world.mesh_db, cfg, SEED, return_labels=True)
    assert same_bits(got[0], hyp) and same_bits(got[1], pos) and torch.equal(got[2], ids)
    assert same_bits(training.make_hypotheses("coarse_classif_multiview_paper", world.data, world.mesh_db, cfg, SEED), hyp)

    # the model's forward and the loss
    images = world.data.rgbs.float() / 255.0
    im_ids = torch.arange(B, dtype=torch.int32, device=DEV).repeat_interleave(N_HYP)
    labels = [l for l in world.labels for _ in range(N_HYP)]
    out = coarse(images=images, K=world.data.K, labels=labels, TCO=hyp.reshape(B * N_HYP, 4, 4), n_iterations=1, im_ids=im_ids,
                 random_ambient_light=False)["iteration=1"]
    ran = dbg["outputs"]["iteration=1"].network_outputs
    assert set(ran) == {"renderings_logits"} and ran["renderings_logits"].shape == (B * N_HYP, 1)
    logits = out.network_outputs["renderings_logits"]
    assert same_bits(logits, ran["renderings_logits"].detach())
    rows = losses.renderings_confidence_loss(logits.view(B, N_HYP), pos, TEMPERATURE)
    want_rc = rows.mean()
    want_total = (torch.zeros(B, N_HYP, 1, device=DEV) + ALPHA * rows[..., None]).mean()
    assert meters["loss_renderings_confidence"].mean == want_rc.item() and meters["loss_total"].mean == want_total.item()
    assert same_bits(loss.detach(), want_total) and math.isfinite(want_total.item()) and want_total.item() > 0

    # the gradient at the network's output: alpha (sigmoid(x / T) - y) / (T B n_hyp).  Three float32 roundings lie between the
    # float64 value and the result (1 / (B n_hyp), the product with alpha, the kernel's one rounding): 4 u relative
    loss.backward()
    grad = ran["renderings_logits"].grad
    assert grad is not None and grad.shape == (B * N_HYP, 1)
    ref = ALPHA * C.bce_logits(f64(logits).reshape(B, N_HYP), f64(pos), TEMPERATURE)[1] / (B * N_HYP)
    err = np.abs(f64(grad).reshape(B, N_HYP) - ref)
    print(f"d loss / d logits: worst relative error {(err / np.abs(ref)).max():.3g} (bound {4 * U:.3g})")
    assert (err <= 4 * U * np.abs(ref)).all() and (ref != 0).all()

    again = training.megapose_forward_loss(coarse, cfg, world.data, _meters(), world.mesh_db, 1, None, seed=SEED)
    assert same_bits(again.detach(), loss.detach())
    other = {}
    training.megapose_forward_loss(coarse, cfg, world.data, _meters(), world.mesh_db, 1, other, seed=SEED + 1)
    assert not torch.equal(other["hypotheses_TCO_init"], hyp)


def test_both_heads_fill_both_groups_of_meters(world):
    from happypose_amd import training

    model = _model(world, "resnet18", pose=True)
    meters, dbg = _meters(), {}
    loss = training.megapose_forward_loss(model, _cfg(pose=True), world.data, meters, world.mesh_db, 1, dbg, seed=SEED)
    assert set(meters) == TR.megapose_meter_keys(1) | {"loss_renderings_confidence"} and all(m.n == 1 for m in meters.values())
    keys = list(meters)
    assert keys.index("time_render") < keys.index("loss_TCO") < keys.index("loss_renderings_confidence") < keys.index("loss_total")
    assert all(math.isfinite(m.mean) for m in meters.values()) and meters["loss_TCO"].mean > 0 and meters["loss_renderings_confidence"].mean > 0
    want = 1.0 * meters["loss_TCO"].mean + ALPHA * meters["loss_renderings_confidence"].mean
    assert abs(meters["loss_total"].mean - want) <= 1e-6 * max(want, 1.0)  # float32 means of a few O(0.01 .. 10) values
    loss.backward()
    out = dbg["outputs"]["iteration=1"].network_outputs
    assert bool((out["pose"].grad != 0).any()) and bool((out["renderings_logits"].grad != 0).any())
    # the trainer hands both gradients to one head_backward: every head tensor moves
    trainer = training.HeadTrainer(model, world.mesh_db, _cfg(pose=True), training.HeadOptimConfig(lr=2e-5, n_warmup_steps=0))
    before = trainer.state_dict()
    trainer.step(world.data, _meters(), 1, SEED)
    after = trainer.state_dict()
    assert set(trainer.shapes) == {"pose_fc.weight", "views_logits_head.weight", "pose_fc.bias", "views_logits_head.bias"}
    assert all(not same_bits(after[n], before[n]) for n in trainer.shapes)


def test_what_still_raises(world, coarse):
    from happypose_amd import training

    with pytest.raises(NotImplementedError, match="predict_rendered_views_logits"):
        training.make_hypotheses("coarse_classif_multiview_paper", world.data, world.mesh_db, training.TrainingConfig(), 0)
    with pytest.raises(AssertionError):  # the reference's assert: one iteration
        training.megapose_forward_loss(coarse, _cfg(), world.data, _meters(), world.mesh_db, 2, None)
    with pytest.raises(ValueError):  # the logits loss has no labels without the classifier's draw
        cfg = training.TrainingConfig(predict_rendered_views_logits=True)
        training.megapose_forward_loss(coarse, cfg, world.data, _meters(), world.mesh_db, 1, None)


def _run_three_steps(trainer, world, record=None):
    meters, losses = _meters(), []
    for _ in range(N_STEPS):
        dbg = {}
        W_now = f64(trainer._W)
        losses.append(float(trainer.step(world.data, meters, 1, SEED, debug_dict=dbg)))
        if record is not None:
            record(W_now, dbg["outputs"]["iteration=1"].network_outputs)
    return meters, losses


def test_three_steps_lower_the_loss_and_match_the_float64_replay(world, coarse):
    from happypose_amd import training

    net, cfg = coarse.backbone, _cfg()
    assert net.pose_dim == 0 and net.n_logits == 1
    rows = B * N_HYP
    oc = training.HeadOptimConfig(lr=2e-5, n_warmup_steps=2, clip_grad_norm=1000.0)
    trainer = training.HeadTrainer(coarse, world.mesh_db, cfg, oc)
    before = trainer.state_dict()
    names = list(trainer.shapes)
    assert names == ["views_logits_head.weight", "views_logits_head.bias", "backbone.fc.weight", "backbone.fc.bias"]
    assert before["optimizer"]["step"] == 0 and set(before) - {"optimizer"} == set(net.head_param_shapes())
    assert trainer._W.shape == (1, 512) and trainer._gb.shape == (1,)
    dbg0 = {}
    loss_first = float(training.megapose_forward_loss(coarse, cfg, world.data, _meters(), world.mesh_db, 1, dbg0, seed=SEED).detach())
    logits_first = dbg0["outputs"]["iteration=1"].network_outputs["renderings_logits"].detach().clone()

    O, N = 1, trainer.p.numel()
    flat = lambda d: np.concatenate([np.asarray(d[n], np.float64).reshape(-1) for n in names])  # noqa: E731
    p = flat({n: f64(before[n]) for n in names})
    state = SimpleNamespace(p=p, m=np.zeros(N), v=np.zeros(N), dm=np.zeros(N), dv=np.zeros(N), tol=np.zeros(N), step=0, norms=[])
    t32 = torch.from_numpy(p.astype(np.float32)).requires_grad_()
    opt32 = torch.optim.Adam([t32], lr=oc.lr, betas=oc.betas, eps=oc.eps, weight_decay=oc.weight_decay, foreach=False)
    b1, b2 = oc.betas

    def replay(W_now, out):
        state.step += 1
        assert set(out) == {"renderings_logits", "features", "pooled"}
        d_logits = out["renderings_logits"].grad
        assert d_logits is not None and bool((d_logits != 0).any())
        h = R.head_backward(f64(out["features"]), np.zeros((rows, 0)), f64(d_logits), 1, None, W_now)
        f = R.fc_backward(h["d_feat"], f64(out["pooled"]))
        d_feat_err = (O + 2) * U * h["d_feat_abs"]
        pooled_abs = np.abs(f64(out["pooled"]))
        g = dict(zip(names, (h["dW"], h["db"], f["dW"], f["db"])))
        dg = dict(zip(names, ((rows + 2) * U * h["dW_abs"], (rows + 2) * U * h["db_abs"],
                              (rows + 2) * U * f["dW_abs"] + (1 + (rows + 2) * U) * d_feat_err.T @ pooled_abs,
                              (rows + 2) * U * f["db_abs"] + (1 + (rows + 2) * U) * d_feat_err.sum(0))))
        g, dg = flat(g), flat(dg)
        assert (np.abs(f64(trainer.g) - g) <= dg).all(), "the gradient"
        sq = R.grad_sq_norm(g)
        state.norms.append(math.sqrt(sq))
        lr = oc.lr_at(state.step)
        coef = R.clip_coef(sq, oc.clip_grad_norm)
        if coef < 1:  # the factor comes from the device's norm of the device's gradient, and multiplies with one rounding
            dg = coef * dg + np.abs(coef * g) * ((math.log2(N) + 4) * U / 2 + np.linalg.norm(dg) / math.sqrt(sq) + 2 * U)
        state.p, state.m, state.v = R.adam_step(state.p, g, state.m, state.v, lr=lr, betas=oc.betas, eps=oc.eps, weight_decay=oc.weight_decay,
                                                step=state.step, sq_norm=sq, max_norm=oc.clip_grad_norm)
        state.dm = b1 * state.dm + (1 - b1) * dg
        state.dv = b2 * state.dv + (1 - b2) * (2 * np.abs(coef * g) * dg + dg * dg)
        state.tol += H._update_bound(lr / (1 - b1 ** state.step), math.sqrt(1 - b2 ** state.step), oc.eps, b1, b2, state.m, state.v,
                                     state.dm, state.dv)
        for gr in opt32.param_groups:
            gr["lr"] = lr
        t32.grad = torch.from_numpy((coef * g).astype(np.float32))
        opt32.step()

    meters, losses = _run_three_steps(trainer, world, replay)
    assert losses[0] == loss_first, "the first step's forward is the untrained network's"
    assert meters["loss_renderings_confidence"].n == N_STEPS and meters["grad_norm"].sum == pytest.approx(sum(state.norms), rel=1e-5)
    after = trainer.state_dict()
    got = flat({n: f64(after[n]) for n in names})
    assert all(not same_bits(after[n], before[n]) for n in names)
    err_torch = np.abs(t32.detach().numpy().astype(np.float64) - state.p).max()
    tol = 4 * err_torch + state.tol
    err = np.abs(got - state.p)
    update = np.abs(got - p)
    print(f"coarse: losses {losses}, |trained - replay| max {err.max():.3g}, torch float32 {err_torch:.3g}, worst error / tolerance "
          f"{(err / tol).max():.3g}, median tolerance {np.median(tol):.3g}, median update {np.median(update):.3g}")
    assert (err <= tol).all(), f"{int((err > tol).sum())} of {N} parameters outside the compounded tolerance"
    assert np.median(tol) < 0.1 * np.median(update[update > 0]), "the tolerance is far below what training changed"
    for n in names:  # the network holds the master copy
        assert same_bits(net.get_param_device(n), after[n]), n

    # the logits rows written into the network change the next forward's logits, and the loss went down
    dbg4 = {}
    m4 = _meters()
    training.megapose_forward_loss(coarse, cfg, world.data, m4, world.mesh_db, 1, dbg4, seed=SEED)
    logits_fourth = dbg4["outputs"]["iteration=1"].network_outputs["renderings_logits"].detach()
    assert not torch.equal(logits_fourth, logits_first)
    print(f"coarse: loss_renderings_confidence {loss_first / ALPHA:.6g} -> {m4['loss_renderings_confidence'].mean:.6g} after {N_STEPS} steps")
    assert m4["loss_renderings_confidence"].mean < loss_first / ALPHA * (1 - 1e-6) and m4["loss_total"].mean < loss_first

    # a second trainer from the same state: the same bits
    fresh = training.HeadTrainer(coarse, world.mesh_db, cfg, oc)
    fresh.load_state_dict(before)
    assert fresh.n_steps == 0 and all(same_bits(net.get_param_device(n), before[n]) for n in names)
    _, losses2 = _run_three_steps(fresh, world)
    again = fresh.state_dict()
    assert losses2 == losses and again["optimizer"]["step"] == N_STEPS
    for n in names:
        assert same_bits(again[n], after[n])
        assert same_bits(again["optimizer"]["exp_avg"][n], after["optimizer"]["exp_avg"][n])
        assert same_bits(again["optimizer"]["exp_avg_sq"][n], after["optimizer"]["exp_avg_sq"][n])
