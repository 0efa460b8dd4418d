"""The training losses (csrc/pose_losses.hip, happypose_amd.losses) on the device against the reference's own float64 run
(tests/golden/g13_pose_losses.npz, tools/gen_golden_pose_losses.py), values and gradients.

Bounds, per golden case: the loss (and each part) within 4 x the difference between the reference's OWN float32 and float64 runs
of the case (largest over its four functions), floor one float32 ulp of the case's largest loss; the gradient within 4 x the same
difference of the gradients (floor: one ulp of the largest entry) plus the row's sign-flip allowance
k * 2 * max(|p|, 1) / (3N) * (largest entry of the row's chain), k = the recorded count of difference components below
tau = 16 * 2^-23 * (largest coordinate).  The generator asserted the symmetry margins, so no row is left out and the chosen
symmetries must be equal.  Every test prints its largest error next to the bound (CHANGELOG carries them)."""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pose_losses_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
FUNCS = ("sym", "add", "cp", "mp")
INPUTS = ("TCO_possible_gt", "TCO_input", "refiner_outputs", "K_crop", "points", "tCR", "upstream")


@pytest.fixture(scope="module")
def g13(golden_dir):
    return np.load(golden_dir / "g13_pose_losses.npz")


def case(g, i):
    pre = f"c{i}/"
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def dev(c, rows=None):
    return {k: torch.as_tensor(c[k] if rows is None else c[k][rows]).to(DEV) for k in INPUTS}


def run(f, t, upstream=None):
    """Function ``f`` through happypose_amd.losses with backward: loss, gradient, and (cp / mp through ops) parts and ids."""
    from happypose_amd import losses, ops

    up = t["upstream"] if upstream is None else upstream
    out = {}
    if f in ("sym", "add"):
        x = t["TCO_input"].clone().requires_grad_(True)
        if f == "sym":
            loss, out["assign"] = losses.loss_CO_symmetric(t["TCO_possible_gt"], x, t["points"])
            out["ids"] = ops.loss_co_symmetric_forward(t["TCO_possible_gt"], t["TCO_input"], t["points"])[1][:, None]
        else:
            loss = losses.compute_ADD_L1_loss(t["TCO_possible_gt"][:, 0], x, t["points"])
    else:
        x = t["refiner_outputs"].clone().requires_grad_(True)
        tCR = t["tCR"] if f == "mp" else None
        if f == "cp":
            loss = losses.loss_refiner_CO_disentangled(t["TCO_possible_gt"], t["TCO_input"], x, t["K_crop"], t["points"])
        else:
            loss, data = losses.loss_refiner_CO_disentangled_reference_point(t["TCO_possible_gt"], t["TCO_input"], x, t["K_crop"],
                                                                             t["points"], tCR)
            assert not any(v.requires_grad for v in data.values()) and same_bits(data["loss"], loss.detach())
        _, out["parts"], out["ids"] = ops.loss_refiner_forward(t["TCO_possible_gt"], t["TCO_input"], t["refiner_outputs"], t["K_crop"],
                                                               t["points"], tCR)
        if f == "mp":
            assert all(same_bits(data[k], out["parts"][:, j]) for j, k in enumerate(("loss_orn", "loss_xy", "loss_z")))
    assert loss.requires_grad
    loss.backward(up)
    out["loss"], out["grad"] = loss.detach(), x.grad
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    """torch.equal with NaN equal to NaN."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def ulp(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


@pytest.mark.parametrize("i", range(6))
def test_losses_and_gradients_against_the_reference(g13, i):
    c = case(g13, i)
    t = dev(c)
    n = c["points"].shape[1]
    yard_loss = max(np.abs(c[f"{f}_loss_32"] - c[f"{f}_loss_64"]).max() for f in FUNCS)
    yard_loss = max(yard_loss, max(np.abs(c[f"{f}_parts_32"] - c[f"{f}_parts_64"]).max() for f in ("cp", "mp")))
    yard_grad = max(np.abs(c[f"{f}_grad_32"] - c[f"{f}_grad_64"]).max() for f in FUNCS)
    b_loss = max(4 * yard_loss, ulp(np.concatenate([c[f"{f}_loss_64"] for f in FUNCS])))
    b_grad = max(4 * yard_grad, ulp(np.concatenate([c[f"{f}_grad_64"].ravel() for f in FUNCS])))
    for f in FUNCS:
        out = run(f, t)
        e_loss = np.abs(out["loss"] - c[f"{f}_loss_64"]).max()
        allow = R.allowance(c[f"{f}_k"], c["points"], c[f"{f}_chain"], c["upstream"].astype(np.float64))
        e_rows = np.abs(out["grad"] - c[f"{f}_grad_64"]).reshape(len(allow), -1).max(1)
        print(f"g13 case {i} (B, S, N = {len(allow)}, {c['TCO_possible_gt'].shape[1]}, {n}) {f}: loss error {e_loss:.3g} (bound {b_loss:.3g}), "
              f"gradient error {e_rows.max():.3g} (bound {b_grad:.3g} + allowance up to {allow.max():.3g})")
        assert e_loss <= b_loss, (f, e_loss, b_loss)
        assert (e_rows <= b_grad + allow).all(), (f, e_rows, b_grad, allow)
        if f != "add":
            ids = out["ids"]
            if f == "sym":  # an exact duplicate of the chosen pose is the same answer
                same = np.array_equal(out["assign"], c["sym_assign_32"])
                assert np.array_equal(ids, c["sym_ids"]) or same, (f, ids.ravel(), c["sym_ids"].ravel())
                assert same
            else:
                assert np.array_equal(ids, c[f"{f}_ids"]), (f, ids, c[f"{f}_ids"])
                e_parts = np.abs(out["parts"] - c[f"{f}_parts_64"]).max()
                print(f"g13 case {i} {f}: parts error {e_parts:.3g} (bound {b_loss:.3g})")
                assert e_parts <= b_loss, (f, e_parts, b_loss)
        if f == "sym":
            assert (out["grad"][:, 3] == 0).all()


def test_pred_equal_to_a_candidate_gives_zero_loss_and_gradient(g13):
    from happypose_amd import losses

    t = dev(case(g13, 0))
    pred = t["TCO_possible_gt"][:, 3].clone().requires_grad_(True)
    loss, assign = losses.loss_CO_symmetric(t["TCO_possible_gt"], pred, t["points"])
    loss.backward(t["upstream"])
    assert (loss == 0).all() and (pred.grad == 0).all() and torch.equal(assign, t["TCO_possible_gt"][:, 3])


def test_upstream_gradient_scales_row_wise(g13):
    t = dev(case(g13, 0))
    for f in ("sym", "mp"):
        one = run(f, t, torch.ones_like(t["upstream"]))["grad"].astype(np.float64)
        got = run(f, t)["grad"].astype(np.float64)
        want = one * t["upstream"].cpu().numpy().astype(np.float64).reshape(-1, *[1] * (one.ndim - 1))
        # both are one rounding of the same double: within an ulp of each other after the scaling
        assert (np.abs(got - want) <= 2.0 ** -22 * np.abs(want)).all(), f


def test_xy_and_z_terms_reach_their_own_outputs_only(g13):
    from happypose_amd import ops

    for i in (0, 4):
        t = dev(case(g13, i))
        for tCR in (None, t["tCR"]):
            args = (t["TCO_possible_gt"], t["TCO_input"], t["refiner_outputs"], t["K_crop"], t["points"], tCR)
            ids = ops.loss_refiner_forward(*args)[2]
            grad, parts = ops.loss_refiner_backward(*args, ids, t["upstream"], return_parts=True)
            assert (parts[:, 0, 6:] == 0).all() and (parts[:, 1, :6] == 0).all() and (parts[:, 1, 8] == 0).all() and (parts[:, 2, :8] == 0).all()
            assert (parts[:, 1, 6:8] != 0).any() and (parts[:, 2, 8] != 0).any() and (parts[:, 0, :6] != 0).any()
            assert torch.equal(parts.sum(1), grad)  # the terms' entries are disjoint: the sum adds zeros


def test_two_runs_are_bit_identical_and_rows_do_not_depend_on_the_batch(g13):
    for i in (2, 4):
        c = case(g13, i)
        t = dev(c)
        rows = np.arange(len(c["points"]))[1:4]
        for f in FUNCS:
            a, b, sub = run(f, t), run(f, t), run(f, dev(c, rows))
            for k in a:
                assert np.array_equal(a[k], b[k], equal_nan=True), (i, f, k)
                assert np.array_equal(a[k][rows], sub[k], equal_nan=True), (i, f, k)


def test_a_nan_row_is_nan_and_leaves_its_neighbours_alone(g13):
    c = case(g13, 0)
    clean = {f: run(f, dev(c)) for f in FUNCS}
    for key, idx in (("points", (2, 5, 1)), ("refiner_outputs", (2, 4)), ("TCO_possible_gt", (2, 6, 1, 2)), ("TCO_input", (2, 0, 3))):
        bad = dict(c)
        bad[key] = c[key].copy()
        bad[key][idx] = np.nan
        others = np.array([r for r in range(len(c["points"])) if r != 2])
        for f in FUNCS:
            reads = {"sym": ("points", "TCO_possible_gt", "TCO_input"), "add": ("points", "TCO_input"),
                     "cp": ("points", "refiner_outputs", "TCO_possible_gt", "TCO_input"),
                     "mp": ("points", "refiner_outputs", "TCO_possible_gt", "TCO_input")}[f]
            out = run(f, dev(bad))
            for k, v in out.items():
                assert np.array_equal(v[others], clean[f][k][others]), (key, f, k)
                if key in reads:
                    assert (v[2] == -1).all() if k == "ids" else np.isnan(v[2]).all(), (key, f, k, v[2])


def test_degenerate_6d_part_gives_a_nan_row(g13):
    c = dict(case(g13, 0))
    c["refiner_outputs"] = c["refiner_outputs"].copy()
    c["refiner_outputs"][1, :6] = (0.5, 0, 0, 2, 0, 0)  # y parallel to x, the cross product exactly zero: z = 0 / 0, as in the reference
    out = run("mp", dev(c))
    assert np.isnan(out["loss"][1]) and np.isnan(out["grad"][1]).all() and (out["ids"][1] == -1).all()
    assert np.isfinite(out["loss"][[0, 2, 3, 4, 5]]).all()


def test_empty_batch_l2_and_cpu_tensors(g13):
    from happypose_amd import losses

    c = case(g13, 0)
    t = dev(c)
    e = {k: v[:0] for k, v in t.items()}
    x = e["refiner_outputs"].clone().requires_grad_(True)
    loss, data = losses.loss_refiner_CO_disentangled_reference_point(e["TCO_possible_gt"], e["TCO_input"], x, e["K_crop"], e["points"], e["tCR"])
    loss.backward(e["upstream"])
    assert loss.shape == (0,) and x.grad.shape == (0, 9) and all(v.shape == (0,) for v in data.values())
    loss, assign = losses.loss_CO_symmetric(e["TCO_possible_gt"], e["TCO_input"], e["points"])
    assert loss.shape == (0,) and assign.shape == (0, 4, 4)
    assert losses.loss_refiner_CO_disentangled(e["TCO_possible_gt"], e["TCO_input"], e["refiner_outputs"], e["K_crop"], e["points"]).shape == (0,)
    assert losses.compute_ADD_L1_loss(e["TCO_possible_gt"][:, 0], e["TCO_input"], e["points"]).shape == (0,)
    with pytest.raises(NotImplementedError):
        losses.loss_CO_symmetric(t["TCO_possible_gt"], t["TCO_input"], t["points"], l1_or_l2=losses.l2)
    with pytest.raises(ValueError):
        losses.loss_CO_symmetric(t["TCO_possible_gt"], t["TCO_input"].cpu(), t["points"])
    with pytest.raises(ValueError):
        losses.loss_refiner_CO_disentangled(t["TCO_possible_gt"].cpu(), t["TCO_input"].cpu(), t["refiner_outputs"].cpu(), t["K_crop"].cpu(),
                                            t["points"].cpu())
