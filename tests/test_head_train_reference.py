"""The float64 yardstick of head training (tests/head_train_ref.py) against an independent oracle, torch itself: torch.autograd on
an nn.Linear head and torch.optim.Adam / AdamW with clip_grad_norm_ and a LambdaLR warm-up, everything in float64.  Both sides are
float64 evaluations of the same formulas, so they agree to 1e-12 relative.  No GPU."""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import head_train_ref as R  # noqa: E402

from happypose_amd.training import HeadOptimConfig  # noqa: E402

RTOL = 1e-12


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), 1e-300)
    return np.abs(a - b).max() <= RTOL * scale


@pytest.mark.parametrize("B,C,pose_dim,n_logits,weighted", [(1, 24, 9, 0, False), (3, 24, 9, 1, True), (65, 512, 9, 4, True),
                                                            (64, 40, 9, 0, True)])
def test_head_backward_is_autograd_of_a_linear_head(B, C, pose_dim, n_logits, weighted):
    rs = np.random.RandomState(B * 1000 + C)
    O = pose_dim + n_logits
    feat, W, bias = rs.randn(B, C), rs.randn(O, C), rs.randn(O)
    d_pose, d_logits = rs.randn(B, pose_dim), (rs.randn(B, n_logits) if n_logits else None)
    w = rs.rand(B) if weighted else None
    if weighted:
        w[0] = 0.0
    lin = torch.nn.Linear(C, O).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(W)), lin.bias.copy_(torch.from_numpy(bias))
    x = torch.from_numpy(feat).requires_grad_()
    up = torch.from_numpy(R.weighted_d_out(d_pose, d_logits, n_logits, w))
    lin(x).backward(up)
    ref = R.head_backward(feat, d_pose, d_logits, n_logits, w, W)
    assert close(ref["dW"], lin.weight.grad.numpy()) and close(ref["db"], lin.bias.grad.numpy()) and close(ref["d_feat"], x.grad.numpy())
    # a NULL logits part is a zero gradient on those rows
    none = R.head_backward(feat, d_pose, None, n_logits, w, W)
    assert not none["dW"][pose_dim:].any() and not none["db"][pose_dim:].any()
    assert close(none["dW"][:pose_dim], ref["dW"][:pose_dim])
    # the bounds' scale dominates the value
    assert (ref["dW_abs"] >= np.abs(ref["dW"]) * (1 - 1e-12)).all() and (ref["d_feat_abs"] >= np.abs(ref["d_feat"]) * (1 - 1e-12)).all()


def test_fc_backward_is_autograd_of_the_fc_and_chains_with_the_head():
    rs = np.random.RandomState(5)
    B, C, O = 7, 32, 10
    pooled, Wfc, bfc, W = rs.randn(B, C), rs.randn(C, C), rs.randn(C), rs.randn(O, C)
    d_pose = rs.randn(B, O)
    fc, head = torch.nn.Linear(C, C).double(), torch.nn.Linear(C, O).double()
    with torch.no_grad():
        fc.weight.copy_(torch.from_numpy(Wfc)), fc.bias.copy_(torch.from_numpy(bfc)), head.weight.copy_(torch.from_numpy(W))
    feat = fc(torch.from_numpy(pooled))
    head(feat).backward(torch.from_numpy(d_pose))
    h = R.head_backward(feat.detach().numpy(), d_pose, W=W)
    f = R.fc_backward(h["d_feat"], pooled)
    assert close(h["dW"], head.weight.grad.numpy()) and close(f["dW"], fc.weight.grad.numpy()) and close(f["db"], fc.bias.grad.numpy())


def test_grad_sq_norm_is_the_square_of_torch_s_total_norm():
    g = np.random.RandomState(1).randn(4099)
    t = torch.from_numpy(g.copy()).requires_grad_()
    t.grad = torch.from_numpy(g.copy())
    total = torch.nn.utils.clip_grad_norm_([t], max_norm=1e9)
    assert close(np.sqrt(R.grad_sq_norm(g)), total.item())


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("max_norm", [0.5, 1000.0])  # the reference trainers' two values: one below, one above the norms met here
def test_adam_step_is_torch_optim_with_clipping_and_warm_up(decoupled, weight_decay, max_norm):
    rs = np.random.RandomState(3)
    n, n_warm, lr = 257, 3, 3e-3
    p0 = rs.randn(n)
    grads = [rs.randn(n) * s for s in (1.0, 0.1, 0.01, 2.0, 1e-3)]
    t = torch.from_numpy(p0.copy()).requires_grad_()
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([t], lr=lr, weight_decay=weight_decay)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda batch: min((batch + 1) / n_warm, 1.0))  # CP/training/train_pose.py:387-392
    cfg = HeadOptimConfig(lr=lr, n_warmup_steps=n_warm)
    p, m, v = p0, np.zeros(n), np.zeros(n)
    clipped = []
    for step, g in enumerate(grads, 1):
        t.grad = torch.from_numpy(g.copy())
        total = torch.nn.utils.clip_grad_norm_([t], max_norm=max_norm, norm_type=2)
        assert close(np.sqrt(R.grad_sq_norm(g)), total.item())
        clipped.append(total.item() > max_norm)
        assert opt.param_groups[0]["lr"] == pytest.approx(cfg.lr_at(step), rel=1e-15) and cfg.lr_at(step) == R.lr_at(lr, step, n_warm)
        opt.step()
        sched.step()
        p, m, v = R.adam_step(p, g, m, v, lr=cfg.lr_at(step), betas=cfg.betas, eps=cfg.eps, weight_decay=weight_decay, step=step,
                              decoupled=decoupled, max_norm=max_norm)
        st = opt.state[t]
        assert close(p, t.detach().numpy()) and close(m, st["exp_avg"].numpy()) and close(v, st["exp_avg_sq"].numpy()), step
    assert any(clipped) == (max_norm == 0.5) and (max_norm == 0.5 or not any(clipped))


def test_config_defaults_are_the_reference_trainers():
    c = HeadOptimConfig()
    # torch.optim.Adam(lr=3e-4, weight_decay=0.0): L2 form, torch's default betas and eps; MegaPose's clip; 50 epochs of 7200 batches
    assert (c.lr, c.betas, c.eps, c.weight_decay, c.decoupled, c.clip_grad_norm, c.n_warmup_steps) == \
        (3e-4, (0.9, 0.999), 1e-8, 0.0, False, 1000.0, 360000)
    assert HeadOptimConfig.cosypose().clip_grad_norm == 0.5 and HeadOptimConfig.cosypose(lr=1e-3).lr == 1e-3
    adam = torch.optim.Adam([torch.zeros(1, requires_grad=True)]).defaults
    assert (adam["betas"], adam["eps"]) == (c.betas, c.eps)
    assert HeadOptimConfig(n_warmup_steps=0).lr_at(1) == 3e-4 and c.lr_at(360000) == 3e-4 and c.lr_at(720000) == 3e-4
    assert c.lr_at(1) == 3e-4 * (1 / 360000)  # LambdaLR: base_lr * lambda(step)
