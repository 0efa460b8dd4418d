"""The coarse classifier's kernels (csrc/train_hyp.hip: hp_views_sphere26, hp_coarse_hypotheses; csrc/pose_losses.hip:
hp_loss_bce_logits) against the restatement tests/coarse_hyp_ref.py (itself checked by tests/test_coarse_hyp_reference.py).

Bounds.
* views: ``rtol = 1e-5, atol = 2e-6``, the bound of ``test_pose_prep_multiview_vs_oracle`` (tests/test_gpu_kernels.py) for the
  front views: the same double look-at, the same float32 tail, the same kind of reference.  The inputs keep ``|f x up|`` of every
  candidate out of (1e-9, 1e-5), asserted on the reference, so host and device cannot decide the degenerate rule differently.
* draw: integers, compared exactly.  Poses of the selected candidates: the bits of ``views_sphere26``.
* BCE: the kernel forms value and gradient in double and rounds once, so the error is half a float32 spacing of the float64 value
  plus double rounding.  Measured on an MI355X over every case below: 0.5 spacings at worst, value and gradient.  The bound is
  4 x that: ``BCE_SPACINGS = 2`` float32 spacings of the float64 reference value."""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import coarse_hyp_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
BCE_SPACINGS = 2.0


def dev(a):
    return torch.as_tensor(a).to(DEV)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def views():
    """Per batch size: the poses, the device's candidates and the reference's (computed once, read-only)."""
    from happypose_amd import ops

    out = {}
    for B in (1, 3, 65):
        T = R.poses(B, seed=B)
        out[B] = (T, ops.views_sphere26(dev(T)), R.views_sphere26(T))
    return out


@pytest.mark.parametrize("B", [1, 3, 65])  # 65 x 104 rows: more than one workgroup, poses that straddle a wavefront
def test_views_sphere26_against_the_reference(views, B):
    from happypose_amd import ops

    T, got, ref = views[B]
    cross = R.cross_norms(T)
    assert not ((cross > 1e-9) & (cross < 1e-5)).any(), "a test pose is too close to the degenerate look-at to be decided alike"
    assert (cross[0] < 1e-9).sum() == 2  # tCR_y == 0: the fallback path is in the comparison, all 16 entries
    assert got.shape == (B, 104, 4, 4) and got.dtype == torch.float32
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-5, atol=2e-6)
    if B > 2:
        assert not np.isfinite(ref[2]).all() and np.isfinite(ref[[0, 1]]).all()
    # without the rotations: every fourth candidate, bit for bit; the rotations are exact quarter turns of it
    plain = ops.views_sphere26(dev(T), inplane_rotations=False)
    assert plain.shape == (B, 26, 4, 4) and same_bits(plain, got[:, ::4].contiguous())
    v = got.view(B, 26, 4, 4, 4)
    fin = torch.isfinite(plain).all(-1).all(-1)
    for rot, (a, b) in {1: ((-1, 1), (1, 0)), 2: ((-1, 0), (-1, 1)), 3: ((1, 1), (-1, 0))}.items():
        r = v[:, :, rot]
        assert same_bits(r[fin][:, :, 3], plain[fin][:, :, 3]) and same_bits(r[fin][:, 2:], plain[fin][:, 2:])
        assert torch.equal(r[fin][:, 0, :3], a[0] * plain[fin][:, a[1], :3]) and torch.equal(r[fin][:, 1, :3], b[0] * plain[fin][:, b[1], :3])
    assert same_bits(ops.views_sphere26(dev(T)), got)


def test_views_sphere26_with_a_reference_point_and_argument_errors():
    from happypose_amd import ops

    T = R.poses(5, seed=11)[3:]
    tCR = (T[:, :3, 3] + np.float32([[0.02, -0.03, 0.05]])).astype(np.float32)
    cross = R.cross_norms(T, tCR)
    assert not ((cross > 1e-9) & (cross < 1e-5)).any()
    got = ops.views_sphere26(dev(T), dev(tCR))
    np.testing.assert_allclose(got.cpu().numpy(), R.views_sphere26(T, tCR), rtol=1e-5, atol=2e-6)
    assert not torch.equal(got, ops.views_sphere26(dev(T)))
    assert ops.views_sphere26(dev(T[:0])).shape == (0, 104, 4, 4)
    with pytest.raises(ValueError):
        ops.views_sphere26(torch.as_tensor(T))
    with pytest.raises(AssertionError):
        ops.views_sphere26(dev(T), dev(tCR[:1]))


@pytest.mark.parametrize("row_offset", [0, 2 ** 40])
@pytest.mark.parametrize("n_hyp", [1, 6, 104])
def test_coarse_hypotheses_draw_and_poses(views, n_hyp, row_offset):
    from happypose_amd import ops

    T, cand, _ = views[65]
    hyp, ids, pos = ops.coarse_hypotheses(dev(T), n_hyp, seed=R.SEED, row_offset=row_offset)
    assert hyp.shape == (65, n_hyp, 4, 4) and ids.shape == (65, n_hyp) and ids.dtype == torch.int32 and pos.dtype == torch.float32
    ref_ids, ref_pos = R.draw(65, n_hyp, R.SEED, row_offset)
    assert np.array_equal(ids.cpu().numpy(), ref_ids) and np.array_equal(pos.cpu().numpy(), ref_pos)
    want = torch.gather(cand, 1, ids.long()[:, :, None, None].expand(-1, -1, 4, 4))
    assert same_bits(hyp, want), "a selected candidate's pose is not the one views_sphere26 gives"
    again = ops.coarse_hypotheses(dev(T), n_hyp, seed=R.SEED, row_offset=row_offset)
    assert all(same_bits(a, b) for a, b in zip((hyp, ids.float(), pos), (again[0], again[1].float(), again[2])))
    # image b draws from (seed, row_offset + b) alone
    sub = ops.coarse_hypotheses(dev(T[20:27]), n_hyp, seed=R.SEED, row_offset=row_offset + 20)
    assert torch.equal(sub[1], ids[20:27]) and same_bits(sub[0], hyp[20:27].contiguous())


def test_coarse_hypotheses_forced_slot_and_argument_errors(views):
    from happypose_amd import ops

    T = views[65][0]
    for nrv, p in ((1, 1.0), (3, 1.0), (1, 0.0), (2, 0.7)):
        _, ids, pos = ops.coarse_hypotheses(dev(T), 6, seed=R.SEED + 1, n_rendered_views=nrv, p_force_positive=p)
        ref_ids, ref_pos = R.draw(65, 6, R.SEED + 1, 0, nrv, p)
        assert np.array_equal(ids.cpu().numpy(), ref_ids) and np.array_equal(pos.cpu().numpy(), ref_pos)
    for bad in (0, 105):
        with pytest.raises(AssertionError):
            ops.coarse_hypotheses(dev(T), bad, seed=1)
    with pytest.raises(AssertionError):
        ops.coarse_hypotheses(dev(T), 2, seed=1, n_rendered_views=3)
    with pytest.raises(ValueError):
        ops.coarse_hypotheses(torch.as_tensor(T), 6, seed=1)
    assert ops.coarse_hypotheses(dev(T[:0]), 6, seed=1)[0].shape == (0, 6, 4, 4)


# ---- the rendered-views-logits loss ------------------------------------------------------------------------------------------------
EDGE_LOGITS = np.array([0.0, 1e-4, -1e-4, 30.0, -30.0, 200.0, -200.0], np.float32)


def _spacings(got, ref):
    return float((np.abs(got.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)).max())


@pytest.mark.parametrize("temperature", [1.0, 0.5])
@pytest.mark.parametrize("shape", [(1,), (65,), (6, 104)])
def test_renderings_confidence_loss_against_float64(shape, temperature):
    from happypose_amd import losses

    n = int(np.prod(shape))
    rs = np.random.RandomState(n)
    x = (rs.randn(n) * 4).astype(np.float32)
    y = (rs.rand(n) < 0.5).astype(np.float32)
    if n >= 2 * len(EDGE_LOGITS):  # every edge logit against both labels
        x[:2 * len(EDGE_LOGITS)] = np.tile(EDGE_LOGITS, 2)
        y[:2 * len(EDGE_LOGITS)] = np.repeat([0.0, 1.0], len(EDGE_LOGITS))
    else:
        x[0] = 200.0 if temperature == 1.0 else -30.0
    up = (rs.rand(n) + 0.5).astype(np.float32)
    x, y, up = x.reshape(shape), y.reshape(shape), up.reshape(shape)
    ref_loss, ref_grad = R.bce_logits(x, y, temperature)
    ref_grad = ref_grad * up.astype(np.float64)
    logits = dev(x).requires_grad_()
    loss = losses.renderings_confidence_loss(logits, dev(y), temperature)
    assert loss.shape == logits.shape and loss.dtype == torch.float32 and loss.requires_grad
    loss.backward(dev(up))
    got_loss, got_grad = loss.detach().cpu().numpy(), logits.grad.cpu().numpy()
    assert np.isfinite(got_loss).all() and np.isfinite(got_grad).all()
    e_loss, e_grad = _spacings(got_loss, ref_loss), _spacings(got_grad, ref_grad)
    print(f"BCE {shape} T = {temperature}: value {e_loss:.3f}, gradient {e_grad:.3f} float32 spacings of the float64 value (bound {BCE_SPACINGS})")
    assert e_loss <= BCE_SPACINGS and e_grad <= BCE_SPACINGS
    if n >= 2 * len(EDGE_LOGITS):  # the saturated branch: the loss of a confident right answer is tiny but not lost, a wrong one is |x|
        flat = got_loss.reshape(-1)
        assert flat[5] == np.float32(200.0 / temperature) and flat[len(EDGE_LOGITS) + 6] == np.float32(200.0 / temperature)
        assert 0 < flat[4] < 1e-12 and 0 < flat[len(EDGE_LOGITS) + 3] < 1e-12
    again = losses.renderings_confidence_loss(dev(x), dev(y), temperature)
    assert same_bits(again, loss)


def test_renderings_confidence_loss_argument_errors():
    from happypose_amd import losses

    x, y = torch.zeros(4, device=DEV), torch.ones(4, device=DEV)
    with pytest.raises(ValueError):
        losses.renderings_confidence_loss(x.cpu(), y)
    with pytest.raises(ValueError):
        losses.renderings_confidence_loss(x, y.cpu())
    with pytest.raises(AssertionError):
        losses.renderings_confidence_loss(x, y[:3])
    with pytest.raises(AssertionError):
        losses.renderings_confidence_loss(x, y, 0.0)
    assert losses.renderings_confidence_loss(x[:0], y[:0]).shape == (0,)
