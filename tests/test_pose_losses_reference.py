"""tests/pose_losses_ref.py (the float64 restatement of the training losses and their analytic gradient) against the reference's
own float64 run (tests/golden/g13_pose_losses.npz, tools/gen_golden_pose_losses.py) and against central finite differences, and the
argument guards of the loss entry points that need no GPU."""

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pose_losses_ref as R  # noqa: E402

RTOL = 1e-12
INPUTS = ("TCO_possible_gt", "TCO_input", "refiner_outputs", "K_crop", "points", "tCR", "upstream")


@pytest.fixture(scope="module")
def g13(golden_dir):
    return np.load(golden_dir / "g13_pose_losses.npz")


def cases(g):
    for i in range(int(g["n_cases"])):
        pre = f"c{i}/"
        yield i, {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def close(got, want, what):
    scale = max(float(np.abs(want).max()), 1e-300)
    assert np.abs(got - want).max() <= RTOL * scale, (what, float(np.abs(got - want).max()), scale)


def restate(c, f):
    """Loss, parts, ids and gradient of function ``f`` of a golden case by the restatement."""
    gt, pts, up = c["TCO_possible_gt"], c["points"], c["upstream"].astype(np.float64)
    if f in ("sym", "add"):
        table = gt if f == "sym" else gt[:, :1]
        out = R.loss_co_symmetric(table, c["TCO_input"], pts)
        out["grad"] = R.grad_co_symmetric(table, c["TCO_input"], pts, out["sym_id"], up)
        out["ids"] = out["sym_id"][:, None]
        return out
    tCR = c["tCR"] if f == "mp" else None
    out = R.loss_refiner(gt, c["TCO_input"], c["refiner_outputs"], c["K_crop"], pts, tCR)
    out["grad_parts"] = R.grad_refiner(gt, c["TCO_input"], c["refiner_outputs"], c["K_crop"], pts, tCR, out["sym_ids"], up)
    out["grad"], out["ids"] = out["grad_parts"].sum(1), out["sym_ids"]
    return out


def test_golden_file_holds_the_cases_of_the_generator(g13):
    shapes = {(c["points"].shape[0], c["TCO_possible_gt"].shape[1], c["points"].shape[1]) for _, c in cases(g13)}
    assert {s[0] for s in shapes} == {1, 6, 37} and {s[1] for s in shapes} == {1, 2, 8, 64}
    assert {s[2] for s in shapes} == {1, 63, 64, 65, 257, 2600}
    assert all(g13[k].dtype.kind in "fiub" for k in g13.files)  # arrays only


def test_restatement_matches_the_reference_in_float64(g13):
    for i, c in cases(g13):
        for f in ("sym", "add", "cp", "mp"):
            out = restate(c, f)
            close(out["loss"], c[f"{f}_loss_64"], (i, f, "loss"))
            assert np.array_equal(out["ids"], c[f"{f}_ids"]), (i, f)
            full = c[f"{f}_grad_64"]
            close(out["grad"], full, (i, f, "grad"))
            if f == "sym":
                close(out["TCO_assign"], c["sym_assign_64"], (i, f, "assign"))
                assert (full[:, 3] == 0).all()
            if f in ("cp", "mp"):
                close(out["parts"], c[f"{f}_parts_64"], (i, f, "parts"))
                close(R.chain_max(c["TCO_possible_gt"], c["TCO_input"], c["refiner_outputs"], c["K_crop"], c["tCR"] if f == "mp" else None),
                      c[f"{f}_chain"], (i, f, "chain"))


def test_analytic_gradient_matches_central_differences(g13):
    """At the rows the generator marked free of difference components below 1e-6: a step of 1e-8 moves no sign there."""
    h, checked = 1e-8, 0
    for i, c in cases(g13):
        up = c["upstream"].astype(np.float64)
        for f in ("sym", "cp", "mp"):
            rows = np.flatnonzero(c[f"{f}_fd_free"])[:3]
            if not len(rows):
                continue
            sub = {k: c[k][rows].astype(np.float64) for k in INPUTS}
            x0 = sub["TCO_input"] if f == "sym" else sub["refiner_outputs"]
            entries = [(a, b) for a in range(3) for b in range(4)] if f == "sym" else [(k,) for k in range(9)]

            def total(x):
                if f == "sym":
                    return R.loss_co_symmetric(sub["TCO_possible_gt"], x, sub["points"])["loss"]
                return R.loss_refiner(sub["TCO_possible_gt"], sub["TCO_input"], x, sub["K_crop"], sub["points"], sub["tCR"] if f == "mp" else None)["loss"]

            grad = restate({k: c[k][rows] for k in INPUTS}, f)["grad"]
            for e in entries:
                xp, xm = x0.copy(), x0.copy()
                xp[(slice(None), *e)] += h
                xm[(slice(None), *e)] -= h
                fd = (total(xp) - total(xm)) / (2 * h) * up[rows]
                got = grad[(slice(None), *e)]
                assert np.abs(fd - got).max() <= 1e-6 * max(1.0, float(np.abs(grad).max())), (i, f, e, fd, got)
                checked += 1
    assert checked >= 100


def test_xy_and_z_terms_reach_their_own_outputs_only(g13):
    for i, c in cases(g13):
        for f in ("cp", "mp"):
            parts = restate(c, f)["grad_parts"]
            assert (parts[:, 0, 6:] == 0).all() and (parts[:, 1, :6] == 0).all() and (parts[:, 1, 8] == 0).all() and (parts[:, 2, :8] == 0).all()


def test_losses_module_refuses_l2_and_cpu_tensors(g13):
    import torch

    from happypose_amd import losses

    c = dict(cases(g13))[0]
    t = {k: torch.as_tensor(c[k]) for k in INPUTS}
    with pytest.raises(NotImplementedError):
        losses.loss_CO_symmetric(t["TCO_possible_gt"], t["TCO_input"], t["points"], l1_or_l2=losses.l2)
    with pytest.raises(ValueError):
        losses.loss_CO_symmetric(t["TCO_possible_gt"], t["TCO_input"], t["points"])
    with pytest.raises(ValueError):
        losses.loss_refiner_CO_disentangled_reference_point(t["TCO_possible_gt"], t["TCO_input"], t["refiner_outputs"], t["K_crop"],
                                                            t["points"], t["tCR"])


def test_argument_guards_without_gpu():
    from happypose_amd import _ffi

    lib = _ffi.lib()
    assert lib.hp_pose_loss_workspace_bytes(5, 64) == 5 * 64 * 12 and lib.hp_pose_loss_workspace_bytes(0, 1) == 0
    assert lib.hp_pose_loss_workspace_bytes(-1, 1) == -1 and lib.hp_pose_loss_workspace_bytes(1, 0) == -1
    # B == 0 is answered before anything else is looked at
    assert lib.hp_loss_co_symmetric(0, 0, 0, None, None, None, None, None, None, None, 0, None) == 0
    assert lib.hp_loss_co_symmetric_backward(0, 0, 0, None, None, None, None, None, None, None) == 0
    assert lib.hp_loss_refiner_disentangled(0, 0, 0, None, None, None, None, None, None, None, None, None, None, 0, None) == 0
    assert lib.hp_loss_refiner_disentangled_backward(0, 0, 0, None, None, None, None, None, None, None, None, None, None, None) == 0
    for s, n in ((0, 5), (5, 0)):
        assert lib.hp_loss_co_symmetric(1, s, n, None, None, None, None, None, None, None, 0, None) == -1
        assert b"hp_loss_co_symmetric" in lib.hp_last_error()
        assert lib.hp_loss_co_symmetric_backward(1, s, n, None, None, None, None, None, None, None) == -1
        assert lib.hp_loss_refiner_disentangled(1, s, n, None, None, None, None, None, None, None, None, None, None, 0, None) == -1
        assert lib.hp_loss_refiner_disentangled_backward(1, s, n, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert lib.hp_loss_co_symmetric(-1, 1, 1, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.hp_loss_refiner_disentangled(1, 1, 1, None, None, None, None, None, None, None, None, None, None, 0, None) == -1  # null pointers
