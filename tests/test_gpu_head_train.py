"""Head training on the device (csrc/head_train.hip, happypose_amd.training.HeadTrainer) against the float64 restatement
tests/head_train_ref.py (itself held against torch.autograd / torch.optim by tests/test_head_train_reference.py).

Bounds, u = 2^-24, all evaluated in float64 from the inputs of the case:

* backward: ``|dW - ref| <= (B + 2) u sum_b |w_b d_out[b, o] feat[b, c]|`` per element, the same form for ``db``, and
  ``(O + 2) u sum_o |.|`` for ``d_feat``.  A term meets one rounding in ``w_b d_out``, at most 64 in its chunk's fma chain,
  ``ceil(B / 64) - 1`` when the chunks are added and one more under ``accumulate``: never more than ``B + 2``.
* the chunk length is a constant of the kernel, not a launch parameter: there is no chunk count to vary, the order of the sum is
  a function of ``B`` alone.  What is checked is that two launches give the same bits.
* ``grad_sq_norm``: ``(log2(N) + 4) u`` relative (all terms are positive).  The tree: a lane squares four elements and adds them
  pairwise (3 roundings), 6 butterfly levels over the wavefront, 2 over the four wavefronts -- 11 for a workgroup's 1024
  elements; the second level adds ``ceil(P / 256) - 1`` partials per lane in sequence (``P = ceil(N / 1024)``), then again 6 + 2.
  Additions of the zeros that pad a short tree are exact, so ``depth(N)`` below counts the levels that can round, and the test
  asserts ``depth(N) <= log2(N) + 4`` for its sizes before it uses the bound.
* ``adamw_step``: not fixed in advance.  The kernel and torch's own float32 CPU optimiser run on the same inputs; the error of
  each is its distance from the float64 reference, per case the largest over the three steps and over ``p``, ``m``, ``v`` of
  ``max |x - ref| / max |ref|``.  The kernel's limit is 4 x torch's measured error (the margin covers another order of fused
  multiply-adds and the reduction order of the clipping norm).  Measured values: DESIGN.md 4.10d.
* end to end: the trained heads against a float64 replay of the three steps from the features, ``dL/dpose`` and head matrix read
  back from the device.  The limits above are compounded per element as  4 x (distance of torch's float32 CPU Adam from the
  float64 replay over the same three steps, on the replay's gradients rounded to float32)  +  the first-order effect of the
  gradient bounds on every step's update: with ``dg`` the backward bound (``(B + 2) u`` x the absolute sums, through the fc with
  ``d_feat``'s own bound, plus ``|g|`` x half the norm's bound when the step clips), ``dm = sum_j (1 - b1) b1^(k - j) dg_j``,
  ``dv = sum_j (1 - b2) b2^(k - j) (2 |g_j| dg_j + dg_j^2)``, the update ``s m / denom`` moves by at most
  ``s (dm / denom + |m| dv / (2 sqrt(v) c denom^2))`` (``s`` the step size, ``c = sqrt(1 - b2^k)``), capped at twice Adam's
  largest possible update ``s (1 - b1) / sqrt(1 - b2) / c``; every step's term is added."""

import math
import sys
from collections import defaultdict
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import head_train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = R.U


def dev(a):
    return torch.as_tensor(a).to(DEV)


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def within(got, ref, bound, what):
    err = np.abs(f64(got) - ref)
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the bound, worst error {err.max():.3g} at bound " \
                          f"{bound.reshape(-1)[int(np.argmax(err - bound))]:.3g}"
    return float((err / np.maximum(bound, 1e-300)).max())


# ---- hp_head_backward / hp_fc_backward -------------------------------------------------------------------------------------------
HEADS = [(9, 0), (9, 1), (9, 4)]  # O = 9, 10, 13


@pytest.mark.parametrize("C", [24, 512, 1536])
@pytest.mark.parametrize("B", [1, 3, 64, 65, 257])
def test_head_backward_against_the_float64_reference(B, C):
    from happypose_amd import ops

    rs = np.random.RandomState(B * 4099 + C)
    worst = 0.0
    for pose_dim, n_logits in HEADS:
        O = pose_dim + n_logits
        feat = rs.randn(B, C).astype(np.float32)
        W = (rs.randn(O, C) / math.sqrt(C)).astype(np.float32)
        d_pose = rs.randn(B, pose_dim).astype(np.float32)
        d_logits = rs.randn(B, n_logits).astype(np.float32) if n_logits else None
        w = rs.rand(B).astype(np.float32)
        w[::3] = 0.0  # zero-weight rows (every row when B == 1)
        for use_w, use_logits in [(False, True), (True, False), (True, True)]:
            dl = d_logits if use_logits else None
            ref = R.head_backward(feat, d_pose, dl, n_logits, w if use_w else None, W)
            args = (dev(feat), dev(d_pose), dev(W))
            kw = dict(d_logits=None if dl is None else dev(dl), n_logits=n_logits, w=dev(w) if use_w else None, return_d_feat=True)
            dW, db, d_feat = ops.head_backward(*args, **kw)
            dW2, db2, d_feat2 = ops.head_backward(*args, **kw)
            assert same_bits(dW, dW2) and same_bits(db, db2) and same_bits(d_feat, d_feat2), "a second launch gave other bits"
            tag = f"B={B} C={C} O={O} w={use_w} logits={use_logits}"
            worst = max(worst, within(dW, ref["dW"], (B + 2) * U * ref["dW_abs"], "dW " + tag),
                        within(db, ref["db"], (B + 2) * U * ref["db_abs"], "db " + tag),
                        within(d_feat, ref["d_feat"], (O + 2) * U * ref["d_feat_abs"], "d_feat " + tag))
            if not use_logits and n_logits:
                assert not dW[pose_dim:].any() and not db[pose_dim:].any(), "a NULL logits gradient is zeros"
            if use_w:
                assert not d_feat[::3].any(), "a zero-weight row has no d_feat"
            # accumulate: the rows in two calls against ONE call's reference on all rows, same bound
            h = B // 2  # B == 1: the first call is the empty sum
            cut = lambda t, s: None if t is None else t[s].contiguous()  # noqa: E731
            first = ops.head_backward(args[0][:h].contiguous(), args[1][:h].contiguous(), d_logits=cut(kw["d_logits"], slice(0, h)),
                                      n_logits=n_logits, w=cut(kw["w"], slice(0, h)))
            aW, ab = ops.head_backward(args[0][h:].contiguous(), args[1][h:].contiguous(), d_logits=cut(kw["d_logits"], slice(h, B)),
                                       n_logits=n_logits, w=cut(kw["w"], slice(h, B)), dW=first[0], db=first[1], accumulate=True)
            assert aW.data_ptr() == first[0].data_ptr()
            within(aW, ref["dW"], (B + 2) * U * ref["dW_abs"], "accumulated dW " + tag)
            within(ab, ref["db"], (B + 2) * U * ref["db_abs"], "accumulated db " + tag)
    print(f"head_backward B={B} C={C}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("B,O,C", [(1, 512, 512), (3, 40, 24), (65, 512, 512), (257, 33, 70)])
def test_fc_backward_against_the_float64_reference(B, O, C):
    from happypose_amd import ops

    rs = np.random.RandomState(B + O)
    d_out, x = rs.randn(B, O).astype(np.float32), rs.randn(B, C).astype(np.float32)
    ref = R.fc_backward(d_out, x)
    dW, db = ops.fc_backward(dev(d_out), dev(x))
    dW2, db2 = ops.fc_backward(dev(d_out), dev(x))
    assert same_bits(dW, dW2) and same_bits(db, db2)
    a = within(dW, ref["dW"], (B + 2) * U * ref["dW_abs"], "dW")
    b = within(db, ref["db"], (B + 2) * U * ref["db_abs"], "db")
    h = B // 2
    first = ops.fc_backward(dev(d_out[:h]), dev(x[:h]))
    aW, ab = ops.fc_backward(dev(d_out[h:]), dev(x[h:]), dW=first[0], db=first[1], accumulate=True)
    within(aW, ref["dW"], (B + 2) * U * ref["dW_abs"], "accumulated dW")
    within(ab, ref["db"], (B + 2) * U * ref["db_abs"], "accumulated db")
    print(f"fc_backward B={B} O={O} C={C}: worst error / bound = {max(a, b):.3f}")


def test_argument_errors():
    from happypose_amd import ops

    feat, d_pose = torch.zeros(3, 24, device=DEV), torch.zeros(3, 9, device=DEV)
    with pytest.raises(ValueError):
        ops.head_backward(feat.cpu(), d_pose)
    with pytest.raises(ValueError):
        ops.fc_backward(d_pose.cpu(), feat)
    with pytest.raises(ValueError):
        ops.grad_sq_norm(torch.zeros(4))
    with pytest.raises(ValueError):
        ops.adamw_step(torch.zeros(4), torch.zeros(4, device=DEV), torch.zeros(4, device=DEV), torch.zeros(4, device=DEV), lr=1e-3, step=1)
    with pytest.raises(AssertionError):
        ops.head_backward(feat, d_pose, n_logits=30)  # O > 32
    with pytest.raises(AssertionError):
        ops.head_backward(feat, d_pose, return_d_feat=True)  # no W
    with pytest.raises(AssertionError):
        ops.head_backward(feat, d_pose.double())
    with pytest.raises(AssertionError):
        ops.adamw_step(*[torch.zeros(4, device=DEV)] * 4, lr=1e-3, step=0)
    with pytest.raises(AssertionError):
        ops.adamw_step(*[torch.zeros(4, device=DEV)] * 4, lr=1e-3, step=1, sq_norm=torch.zeros(1, device=DEV))


# ---- hp_grad_sq_norm -------------------------------------------------------------------------------------------------------------
def depth(N: int) -> int:
    """Levels of the reduction tree that can round (module docstring)."""
    in_block = min(N, 1024)
    lanes = min(in_block, 256)
    d = {1: 1, 2: 2}.get(-(-in_block // 256), 3)               # squares and the lane's pairwise additions
    d += min(6, math.ceil(math.log2(min(lanes, 64)))) if lanes > 1 else 0  # butterfly
    d += {1: 0, 2: 1}.get(-(-lanes // 64), 2)                  # wavefronts
    P = -(-N // 1024)
    if P > 1:
        d += -(-P // 256) - 1
        lanes2 = min(P, 256)
        d += min(6, math.ceil(math.log2(min(lanes2, 64))))
        d += {1: 0, 2: 1}.get(-(-lanes2 // 64), 2)
    return d


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4099, 2 ** 20 + 1])
def test_grad_sq_norm(N):
    from happypose_amd import ops

    assert depth(N) <= math.log2(N) + 4, (depth(N), math.log2(N) + 4)
    g = np.random.RandomState(N % 1000).randn(N).astype(np.float32)
    ref = R.grad_sq_norm(g)
    a, b = ops.grad_sq_norm(dev(g)), ops.grad_sq_norm(dev(g))
    assert same_bits(a, b)
    err = abs(float(a) - ref) / ref
    print(f"grad_sq_norm N={N}: relative error {err:.3g}, bound {(math.log2(N) + 4) * U:.3g}, depth {depth(N)}")
    assert err <= (math.log2(N) + 4) * U
    assert float(ops.grad_sq_norm(torch.zeros(0, device=DEV))) == 0.0


# ---- hp_adamw_step ---------------------------------------------------------------------------------------------------------------
def _rel(x, ref):
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4099])
def test_adamw_step_against_float64_within_four_times_torch_float32(N):
    from happypose_amd import ops

    lr, steps = 1e-3, 3
    worst = (0.0, 0.0, 0.0)
    for decoupled in (False, True):
        for weight_decay in (0.0, 0.01):
            for clip in ("clips", "does not clip"):
                rs = np.random.RandomState(N)
                p0 = rs.randn(N).astype(np.float32)
                grads = [(rs.randn(N) * s).astype(np.float32) for s in (1.0, 0.1, 0.01)]
                norms = [math.sqrt(R.grad_sq_norm(g)) for g in grads]
                max_norm = 0.5 * min(norms) if clip == "clips" else 2.0 * max(norms)  # every norm above / every norm below
                # torch's own float32 optimiser on the CPU
                t = torch.from_numpy(p0.copy()).requires_grad_()
                opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([t], lr=lr, weight_decay=weight_decay, foreach=False)
                # the kernel
                p, m, v = dev(p0.copy()), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
                mx = torch.full((1,), max_norm, dtype=torch.float32, device=DEV)
                # the float64 reference
                pr, mr, vr = p0.astype(np.float64), np.zeros(N), np.zeros(N)
                err_k = err_t = 0.0
                for step, g in enumerate(grads, 1):  # step 1: the largest bias correction
                    t.grad = torch.from_numpy(g.copy())
                    torch.nn.utils.clip_grad_norm_([t], max_norm=float(np.float32(max_norm)), norm_type=2)
                    opt.step()
                    gd = dev(g)
                    ops.adamw_step(p, gd, m, v, lr=lr, weight_decay=weight_decay, step=step, decoupled=decoupled,
                                   sq_norm=ops.grad_sq_norm(gd), max_norm=mx)
                    assert torch.equal(gd.cpu(), torch.from_numpy(g)), "the gradient buffer is read-only"
                    pr, mr, vr = R.adam_step(pr, g, mr, vr, lr=lr, weight_decay=weight_decay, step=step, decoupled=decoupled,
                                             max_norm=float(np.float32(max_norm)))
                    st = opt.state[t]
                    err_k = max(err_k, _rel(f64(p), pr), _rel(f64(m), mr), _rel(f64(v), vr))
                    err_t = max(err_t, _rel(t.detach().numpy(), pr), _rel(st["exp_avg"].numpy(), mr), _rel(st["exp_avg_sq"].numpy(), vr))
                print(f"adamw_step N={N} decoupled={decoupled} weight_decay={weight_decay} {clip}: kernel {err_k:.3g}, "
                      f"torch float32 {err_t:.3g}, limit {4 * err_t:.3g}")
                assert err_k <= 4 * err_t, (N, decoupled, weight_decay, clip, err_k, err_t)
                if err_k / max(err_t, 1e-300) > worst[0]:
                    worst = (err_k / err_t, err_k, err_t)
    print(f"adamw_step N={N}: largest kernel / torch ratio {worst[0]:.2f} (kernel {worst[1]:.3g}, torch {worst[2]:.3g})")


def test_adamw_step_without_clipping_and_repeat():
    from happypose_amd import ops

    rs = np.random.RandomState(0)
    p0, g = rs.randn(4099).astype(np.float32), rs.randn(4099).astype(np.float32)
    outs = []
    for _ in range(2):
        p, m, v = dev(p0.copy()), torch.zeros(4099, device=DEV), torch.zeros(4099, device=DEV)
        ops.adamw_step(p, dev(g), m, v, lr=1e-3, step=1)
        outs.append((p, m, v))
    assert all(same_bits(a, b) for a, b in zip(*outs))
    pr, mr, vr = R.adam_step(p0, g, np.zeros(4099), np.zeros(4099), lr=1e-3, step=1)
    assert _rel(f64(outs[0][0]), pr) <= 4 * U and _rel(f64(outs[0][1]), mr) <= 4 * U and _rel(f64(outs[0][2]), vr) <= 4 * U


# ---- end to end ------------------------------------------------------------------------------------------------------------------
N_POINTS_LOSS, N_ITERATIONS, N_STEPS, SEED = 64, 2, 3, 7


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


def _make(kind, world):
    from happypose_amd import training
    from happypose_amd.models import create_model_pose, create_pose_model_cosypose

    if kind == "cosypose":
        model = create_pose_model_cosypose(dict(backbone_str="resnet18"), world.renderer, state_dict=_weights("resnet18", 6, 1), max_batch=4)
        cfg = training.CosyPoseTrainingConfig(n_points_loss=N_POINTS_LOSS)
        loss = lambda meters, dbg=None: training.h_pose(model, world.mesh_db, world.data, meters, cfg, N_ITERATIONS, "gt+noise",  # noqa: E731
                                                        seed=SEED, debug_dict=dbg)
        return model, cfg, loss, dict(input_generator="gt+noise"), 1
    mcfg = dict(backbone_str="vanilla_resnet34", n_rendered_views=4, multiview_type="front_3views", render_normals=True, render_depth=False,
                input_depth=False, predict_pose_update=True, depth_augmentation=False, depth_normalization_type="tCR_scale_clamp_center")
    model = create_model_pose(mcfg, world.renderer, state_dict=_weights("vanilla_resnet34", 27, 2), max_batch=4)
    cfg = training.TrainingConfig(hypotheses_init_method="refiner_gt+noise", n_hypotheses=2, n_points_loss=N_POINTS_LOSS)
    loss = lambda meters, dbg=None: training.megapose_forward_loss(model, cfg, world.data, meters, world.mesh_db, N_ITERATIONS, dbg,  # noqa: E731
                                                                   seed=SEED)
    return model, cfg, loss, {}, 2


def _meters():
    from happypose_amd.training import AverageValueMeter

    return defaultdict(AverageValueMeter)


def _update_bound(s, c, eps, b1, b2, m, v, dm, dv):
    """First-order bound on the change of ``s m / (sqrt(v) / c + eps)`` under ``|dm|``, ``|dv|``, capped (module docstring)."""
    root = np.sqrt(v)
    denom = root / c + eps
    d_denom = np.where(root > 0, dv / np.maximum(2 * root * c, 1e-300), np.sqrt(dv) / c)
    first = s * (dm / denom + np.abs(m) * d_denom / denom ** 2)
    return np.minimum(first, 2 * s * (1 - b1) / math.sqrt(1 - b2) / c)


@pytest.mark.parametrize("kind", ["megapose", "cosypose"])
def test_three_steps_lower_the_loss_and_match_the_float64_replay(world, kind):
    from happypose_amd import training

    model, cfg, forward_loss, step_kw, n_hyp = _make(kind, world)
    net = model.backbone
    B = 2 * n_hyp

    # 1. return_features off: the outputs are the ones the predictor gave before, and the features belong to the pose
    images, hyp = world.data.rgbs.float() / 255.0, None
    dbg0 = {}
    loss_first = forward_loss(_meters(), dbg0).detach()
    hyp = dbg0["hypotheses_TCO_init"].reshape(B, 4, 4)
    call = dict(images=images, K=world.data.K, labels=[l for l in world.labels for _ in range(n_hyp)], TCO=hyp, n_iterations=N_ITERATIONS,
                im_ids=torch.arange(2, dtype=torch.int32, device=DEV).repeat_interleave(n_hyp))
    off, on = model(**call), model(return_features=True, **call)
    for k in range(N_ITERATIONS):
        a, b, ran = off[f"iteration={k + 1}"], on[f"iteration={k + 1}"], dbg0["outputs"][f"iteration={k + 1}"]
        assert set(a.network_outputs) == {"pose"} and set(ran.network_outputs) == {"pose"}
        assert set(b.network_outputs) == {"pose", "features"} | ({"pooled"} if kind == "megapose" else set())
        for name in ("TCO_input", "TCO_output", "K_crop", "tCR", "boxes_crop", "boxes_rend"):
            assert same_bits(getattr(a, name), getattr(b, name)) and same_bits(getattr(a, name), getattr(ran, name)), name
        assert same_bits(a.network_outputs["pose"], b.network_outputs["pose"])
        assert same_bits(a.network_outputs["pose"], ran.network_outputs["pose"].detach())
        W, bias = f64(net.get_param_device("pose_fc.weight")), f64(net.get_param_device("pose_fc.bias"))
        feat, pose = f64(b.network_outputs["features"]), f64(b.network_outputs["pose"])
        assert np.abs(feat @ W.T + bias - pose).max() <= (net.n_features + 2) * U * (np.abs(feat) @ np.abs(W).T + np.abs(bias)).max()
        if kind == "megapose":
            Wf, bf = f64(net.get_param_device("backbone.fc.weight")), f64(net.get_param_device("backbone.fc.bias"))
            pooled = f64(b.network_outputs["pooled"])
            assert np.abs(pooled @ Wf.T + bf - feat).max() <= 514 * U * (np.abs(pooled) @ np.abs(Wf).T + np.abs(bf)).max()

    # 2. three steps on the fixed batch
    oc = training.HeadOptimConfig(lr=LR[kind], n_warmup_steps=2, clip_grad_norm=CLIP[kind])
    trainer = training.HeadTrainer(model, world.mesh_db, cfg, oc, kind=kind)
    before = trainer.state_dict()
    assert before["optimizer"]["step"] == 0 and set(before) - {"optimizer"} == set(net.head_param_shapes())
    O, C, N = trainer.pose_dim + trainer.n_logits, trainer.n_features, trainer.p.numel()
    names = list(trainer.shapes)
    flat = lambda d: np.concatenate([np.asarray(d[n], np.float64).reshape(-1) for n in names])  # noqa: E731
    p = flat({n: f64(before[n]) for n in names})
    m, v, dm, dv = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
    t32 = torch.from_numpy(p.astype(np.float32)).requires_grad_()
    opt32 = torch.optim.Adam([t32], lr=oc.lr, betas=oc.betas, eps=oc.eps, weight_decay=oc.weight_decay, foreach=False)
    tol_grad, meters, losses, norms, b1, b2 = np.zeros(N), _meters(), [], [], *oc.betas
    for step in range(1, N_STEPS + 1):
        W_now = f64(trainer._W)  # the head matrix this step's forward and d_feat use
        dbg = {}
        losses.append(float(trainer.step(world.data, meters, N_ITERATIONS, SEED, debug_dict=dbg, **step_kw)))
        g, dg = {n: 0.0 for n in names}, {n: 0.0 for n in names}
        for k in range(N_ITERATIONS):
            out = dbg["outputs"][f"iteration={k + 1}"].network_outputs
            assert out["pose"].grad is not None and bool((out["pose"].grad != 0).any())
            h = R.head_backward(f64(out["features"]), f64(out["pose"].grad), None, trainer.n_logits, None, W_now)
            hW, hb, hWa, hba = (x.reshape(-1) for x in (h["dW"], h["db"], h["dW_abs"], h["db_abs"]))
            head_names = [n for n in names if not n.startswith("backbone.fc")]
            gw = dict(zip(head_names, np.split(np.concatenate([hW, hb]), np.cumsum([int(np.prod(trainer.shapes[n])) for n in head_names])[:-1])))
            ga = dict(zip(head_names, np.split(np.concatenate([hWa, hba]), np.cumsum([int(np.prod(trainer.shapes[n])) for n in head_names])[:-1])))
            for n in head_names:
                g[n] = g[n] + gw[n]
                dg[n] = dg[n] + (B + 2) * U * ga[n]
            if trainer.has_fc:
                f = R.fc_backward(h["d_feat"], f64(out["pooled"]))
                d_feat_err = (O + 2) * U * h["d_feat_abs"]  # the device's d_feat is within this of the exact one
                pooled_abs = np.abs(f64(out["pooled"]))
                g["backbone.fc.weight"] = g["backbone.fc.weight"] + f["dW"].reshape(-1)
                g["backbone.fc.bias"] = g["backbone.fc.bias"] + f["db"]
                dg["backbone.fc.weight"] = dg["backbone.fc.weight"] + ((B + 2) * U * f["dW_abs"] + (1 + (B + 2) * U) * d_feat_err.T @ pooled_abs).reshape(-1)
                dg["backbone.fc.bias"] = dg["backbone.fc.bias"] + (B + 2) * U * f["db_abs"] + (1 + (B + 2) * U) * d_feat_err.sum(0)
        g, dg = flat(g), flat(dg) + N_ITERATIONS * U * np.abs(flat(g))  # accumulate's own rounding per iteration
        assert (np.abs(f64(trainer.g) - g) <= dg).all(), "the accumulated gradient"
        sq = R.grad_sq_norm(g)
        norms.append(math.sqrt(sq))
        assert meters["grad_norm"].n == step and meters["grad_norm"].sum == pytest.approx(sum(norms), rel=1e-5)
        lr = oc.lr_at(step)
        coef = R.clip_coef(sq, oc.clip_grad_norm)
        if coef < 1:  # the factor comes from the device's norm of the device's gradient, and multiplies with one rounding
            dg = coef * dg + np.abs(coef * g) * ((math.log2(N) + 4) * U / 2 + np.linalg.norm(dg) / math.sqrt(sq) + 2 * U)
        p, m, v = R.adam_step(p, g, m, v, lr=lr, betas=oc.betas, eps=oc.eps, weight_decay=oc.weight_decay, step=step, sq_norm=sq,
                              max_norm=oc.clip_grad_norm)
        dm = b1 * dm + (1 - b1) * dg
        dv = b2 * dv + (1 - b2) * (2 * np.abs(coef * g) * dg + dg * dg)
        tol_grad += _update_bound(lr / (1 - b1 ** step), math.sqrt(1 - b2 ** step), oc.eps, b1, b2, m, v, dm, dv)
        # torch's float32 CPU Adam on the replay's gradient (clipped in float64, rounded to float32)
        for gr in opt32.param_groups:
            gr["lr"] = lr
        t32.grad = torch.from_numpy((coef * g).astype(np.float32))
        opt32.step()
    assert meters["lr"].n == N_STEPS and meters["lr"].sum == pytest.approx(sum(oc.lr_at(s) for s in (1, 2, 3)), rel=1e-12)
    assert meters["loss_total"].n == N_STEPS and losses[0] == float(loss_first), "the first step's forward is the untrained network's"

    after = trainer.state_dict()
    got = flat({n: f64(after[n]) for n in names})
    moved = {n: not same_bits(after[n], before[n]) for n in names}
    assert all(moved[n] for n in names if not n.startswith("views_logits_head")), moved
    err_torch = np.abs(t32.detach().numpy().astype(np.float64) - p).max()
    tol = 4 * err_torch + tol_grad
    err = np.abs(got - p)
    print(f"{kind}: losses {losses}, |trained - replay| max {err.max():.3g}, torch float32 {err_torch:.3g}, largest tolerance {tol.max():.3g}, "
          f"worst error / tolerance {(err / tol).max():.3g}, largest update {np.abs(p - flat({n: f64(before[n]) for n in names})).max():.3g}")
    assert (err <= tol).all(), f"{int((err > tol).sum())} of {N} parameters outside the compounded tolerance"
    update = np.abs(got - flat({n: f64(before[n]) for n in names}))
    print(f"{kind}: median tolerance {np.median(tol):.3g}, median update {np.median(update):.3g}")
    assert np.median(tol) < 0.1 * np.median(update[update > 0]), "the tolerance is far below what training changed"
    for n in names:  # the network holds the master copy
        assert same_bits(net.get_param_device(n), after[n]), n

    # 3. a fourth forward on the same batch and seed
    loss_fourth = float(forward_loss(_meters()).detach())
    print(f"{kind}: loss_total {float(loss_first):.6g} -> {loss_fourth:.6g} after {N_STEPS} steps")
    assert loss_fourth < float(loss_first)

    # 4. the state dict round-trips into a fresh trainer, through other contents, bit for bit
    fresh = training.HeadTrainer(model, world.mesh_db, cfg, oc, kind=kind)
    zeros = {n: torch.zeros_like(after[n]) for n in names}
    fresh.load_state_dict(zeros)
    assert fresh.n_steps == 0 and not net.get_param_device("pose_fc.weight").any()
    fresh.load_state_dict(after)
    again = fresh.state_dict()
    assert again["optimizer"]["step"] == N_STEPS
    for n in names:
        assert same_bits(again[n], after[n]) and same_bits(net.get_param_device(n), after[n])
        assert same_bits(again["optimizer"]["exp_avg"][n], after["optimizer"]["exp_avg"][n])
        assert same_bits(again["optimizer"]["exp_avg_sq"][n], after["optimizer"]["exp_avg_sq"][n])
    assert float(forward_loss(_meters()).detach()) == loss_fourth


# The learning rate of the three steps.  The reference's own schedule would run them at 3e-4 x (1 .. 3) / 360000, about 1e-9:
# nothing float32 can show.  Adam's first steps move EVERY weight by about lr whatever the gradient's size, so the pose output
# moves by about lr x sum |features|: on these random-weight networks the loss (0.025 at the start) falls after a step at 5e-5 and
# rises after one at 1e-4 (measured once, MegaPose, fc included).  2e-5 -- warmed up as 1e-5, 2e-5, 2e-5 -- stays five times
# below the rate that overshot and moves the weights by 50 to 100 times the replay's tolerance.
LR = dict(megapose=2e-5, cosypose=2e-5)
CLIP = dict(megapose=1000.0, cosypose=0.5)


def test_what_is_not_built_raises(world):
    from happypose_amd import training

    model, cfg, _, _, _ = _make("cosypose", world)
    with pytest.raises(NotImplementedError):
        training.HeadTrainer(model, world.mesh_db, training.CosyPoseTrainingConfig(loss_disentangled=False), kind="cosypose").step(
            world.data, _meters(), 1, 0)
    with pytest.raises(ValueError):
        training.HeadTrainer(model, world.mesh_db, cfg, kind="detector")
    with pytest.raises(TypeError):
        training.HeadTrainer(SimpleNamespace(backbone=None), world.mesh_db, cfg)
    with pytest.raises(AssertionError):
        model.backbone.set_param_device("layer1.0.conv1.weight", torch.zeros(64, 64, 3, 3, device=DEV))  # packed at finalise
    with pytest.raises(AssertionError):
        model.backbone.set_param_device("pose_fc.weight", torch.zeros(8, 512, device=DEV))  # wrong size
