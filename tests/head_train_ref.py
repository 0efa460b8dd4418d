"""Float64 numpy restatement of the four definitions of head training in include/happypose_amd.h (hp_head_backward,
hp_fc_backward, hp_grad_sq_norm, hp_adamw_step) and of HeadOptimConfig.lr_at.  Nothing here knows about summation orders: the
sums are numpy's in float64, whose own error (about n 2^-53) is nine orders of magnitude below the float32 bounds it is used for.
tests/test_head_train_reference.py holds it against torch.autograd and torch.optim in float64."""

import numpy as np

U = 2.0 ** -24  # unit roundoff of float32


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def weighted_d_out(d_pose, d_logits=None, n_logits=0, w=None):
    """``g [B, O] = w_b * concat(d_pose, d_logits or zeros)``."""
    d_pose = _f64(d_pose)
    B = d_pose.shape[0]
    d_logits = np.zeros((B, n_logits)) if d_logits is None else _f64(d_logits)
    g = np.concatenate([d_pose, d_logits], axis=1)
    return g if w is None else g * _f64(w)[:, None]


def head_backward(feat, d_pose, d_logits=None, n_logits=0, w=None, W=None):
    """``dW [O, C]``, ``db [O]``, ``d_feat [B, C]`` (None without ``W``) and, under the same names with ``_abs``, the sums of
    the absolute values of the terms -- what the float32 bounds scale with."""
    feat, g = _f64(feat), weighted_d_out(d_pose, d_logits, n_logits, w)
    out = dict(dW=g.T @ feat, db=g.sum(0), dW_abs=np.abs(g).T @ np.abs(feat), db_abs=np.abs(g).sum(0), d_feat=None, d_feat_abs=None)
    if W is not None:
        out.update(d_feat=g @ _f64(W), d_feat_abs=np.abs(g) @ np.abs(_f64(W)))
    return out


def fc_backward(d_out, x):
    d_out, x = _f64(d_out), _f64(x)
    return dict(dW=d_out.T @ x, db=d_out.sum(0), dW_abs=np.abs(d_out).T @ np.abs(x), db_abs=np.abs(d_out).sum(0))


def grad_sq_norm(g) -> float:
    g = _f64(g)
    return float(np.dot(g, g))


def clip_coef(sq_norm: float, max_norm: float) -> float:
    """``clip_grad_norm_``: ``min(max_norm / (total_norm + 1e-6), 1)``."""
    return min(float(max_norm) / (np.sqrt(sq_norm) + 1e-6), 1.0)


def adam_step(p, g, m, v, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step, decoupled=False, sq_norm=None, max_norm=None):
    """One step of Adam (``decoupled=False``: L2 added to the gradient) or AdamW on float64 copies: ``(p, m, v)``."""
    p, g, m, v = _f64(p).copy(), _f64(g).copy(), _f64(m).copy(), _f64(v).copy()
    b1, b2 = betas
    if max_norm is not None:
        g = g * clip_coef(grad_sq_norm(g) if sq_norm is None else sq_norm, max_norm)
    if weight_decay != 0:
        if decoupled:
            p = p * (1 - lr * weight_decay)
        else:
            g = g + weight_decay * p
    m = m + (1 - b1) * (g - m)
    v = v * b2 + (1 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps
    p = p - (lr / (1 - b1 ** step)) * (m / denom)
    return p, m, v


def lr_at(lr: float, step: int, n_warmup_steps: int) -> float:
    """Step ``step`` (from 1) of the linear warm-up: ``lr min(step / n_warmup_steps, 1)``; no warm-up with 0."""
    return lr if n_warmup_steps <= 0 else lr * min(step / n_warmup_steps, 1.0)
