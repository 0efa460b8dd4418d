"""Properties of tests/coarse_hyp_ref.py, the float64 restatement the coarse-classifier kernels are compared with
(tests/test_gpu_coarse_hyp.py): what a candidate view is, what the draw promises.  No GPU."""

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import coarse_hyp_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def case():
    T = R.poses(9, seed=3)
    T = np.delete(T, 2, axis=0)  # the non-finite pose has its own test
    cams = np.stack([R.views_TC0_CV(t) for t in T[:, :3, 3].astype(np.float64)])
    return T, cams


def test_offsets_are_the_reference_loop():
    off = R.offsets()
    assert off.shape == (26, 3) and len({tuple(o) for o in off}) == 26 and (0, 1, 0) not in {tuple(o) for o in off}
    assert tuple(off[0]) == (0, 0, 0) and tuple(off[1]) == (0, 0, 1) and tuple(off[2]) == (0, 0, -1) and tuple(off[3]) == (-1, 0, 0)
    assert tuple(off[8]) == (1, 0, -1) and tuple(off[9]) == (0, 1, 1) and tuple(off[25]) == (1, 2, -1)


def test_every_candidate_is_a_rigid_transform(case):
    _, cams = case
    Rm = cams[..., :3, :3]
    assert np.abs(np.swapaxes(Rm, -1, -2) @ Rm - np.eye(3)).max() <= 1e-12
    assert np.abs(np.linalg.det(Rm) - 1.0).max() <= 1e-12
    assert (cams[..., 3, :] == [0, 0, 0, 1]).all()


def test_cameras_sit_on_the_offsets_and_look_at_the_reference_point(case):
    T, cams = case
    off = R.offsets()
    for b, tCR in enumerate(T[:, :3, 3].astype(np.float64)):
        radius = np.linalg.norm(tCR)
        pos, fwd = cams[b, :, :3, 3], cams[b, :, :3, 2]
        # distance from camera 0's centre: |tCR| |offset|; from the reference point: |tCR| |offset - (0, 1, 0)|
        assert np.allclose(np.linalg.norm(pos, axis=1), radius * np.linalg.norm(off, axis=1), rtol=1e-12, atol=1e-15)
        to_ref = tCR - pos
        dist = np.linalg.norm(to_ref, axis=1)
        assert np.allclose(dist, radius * np.linalg.norm(off - [0, 1, 0], axis=1), rtol=1e-12)
        assert np.abs(to_ref / dist[:, None] - fwd).max() <= 1e-12  # +z passes through tCR


def test_candidate_0_is_the_oracles_re_aimed_view(case):
    from oracle import geometry as G

    T, cams = case
    for b, tCR in enumerate(T[:, :3, 3].astype(np.float64)):
        want = G.views_TC0_CV(tCR, "TCO+front_1view", remove_TCO_rendering=True)
        assert want.shape == (1, 4, 4) and np.array_equal(cams[b, 0], want[0])
    full = R.views_sphere26(T)
    want = G.make_TCO_multiview(T, T[:, :3, 3], "TCO+front_1view", 2, remove_TCO_rendering=True)
    np.testing.assert_allclose(full[:, 0], want[:, 0], rtol=1e-6, atol=1e-7)


def test_the_four_rotations_share_a_translation_and_differ_by_quarter_turns(case):
    T, _ = case
    full, plain = R.views_sphere26(T), R.views_sphere26(T, inplane_rotations=False)
    assert full.shape == (len(T), 104, 4, 4) and plain.shape == (len(T), 26, 4, 4) and full.dtype == np.float32
    v = full.reshape(len(T), 26, 4, 4, 4)
    assert np.array_equal(v[:, :, 0], plain)
    for rot in range(1, 4):
        assert np.array_equal(v[:, :, rot, :, 3], plain[..., 3]) and np.array_equal(v[:, :, rot, 3], plain[..., 3, :])
        a = v[:, :, rot, :3, :3]
        r0, r1, r2 = plain[..., 0, :3], plain[..., 1, :3], plain[..., 2, :3]
        want = {1: (-r1, r0), 2: (-r0, -r1), 3: (r1, -r0)}[rot]
        assert np.array_equal(a[..., 0, :], want[0]) and np.array_equal(a[..., 1, :], want[1]) and np.array_equal(a[..., 2, :], r2)


def test_degenerate_and_non_finite_poses():
    T = R.poses(3, seed=3)
    cross = R.cross_norms(T)
    off = R.offsets()
    hit = cross < R.DEGENERATE
    # tCR_y == 0: exactly the offsets (0, 1, +-1) look along the up hint; the fallback keeps them rigid with the re-aimed camera's right
    for b in (0, 1):
        assert {tuple(o) for o in off[hit[b]]} == {(0, 1, 1), (0, 1, -1)}
        cams = R.views_TC0_CV(T[b, :3, 3].astype(np.float64))
        for v in np.nonzero(hit[b])[0]:
            assert np.array_equal(cams[v, :3, 0], cams[0, :3, 0])
            assert np.abs(cams[v, :3, :3].T @ cams[v, :3, :3] - np.eye(3)).max() <= 1e-12
    out = R.views_sphere26(T)
    assert np.isfinite(out[:2]).all() and not np.isfinite(out[2]).all()
    assert (cross[2] == 1).all()  # the identity view: no look-at is evaluated
    # |tCR| == 0: the identity view, every candidate is the pose (up to the quarter turns)
    T0 = R.poses(1, seed=4)
    T0[0, :3, 3] = 0
    assert np.array_equal(R.views_sphere26(T0, inplane_rotations=False), np.repeat(T0[:, None], 26, axis=1))


@pytest.mark.parametrize("n_hyp", [1, 6, 104])
def test_the_draw(n_hyp):
    n = 64
    ids, pos = R.draw(n, n_hyp, R.SEED)
    assert ids.shape == (n, n_hyp) and ids.dtype == np.int32 and pos.dtype == np.float32
    assert ids.min() >= 0 and ids.max() <= 103 and all(len(set(row)) == n_hyp for row in ids.tolist())
    assert np.array_equal(pos, (ids == 0).astype(np.float32)) and pos.sum(1).max() <= 1
    if n_hyp == 104:
        assert (np.sort(ids, axis=1) == np.arange(104)).all() and (pos.sum(1) == 1).all()
    # row b depends on (seed, row_offset + b) alone
    for off in (0, 2 ** 40):
        whole = R.draw(n, n_hyp, R.SEED, off)
        part = R.draw(7, n_hyp, R.SEED, off + 20)
        assert np.array_equal(part[0], whole[0][20:27]) and np.array_equal(part[1], whole[1][20:27])
    assert not np.array_equal(R.draw(n, n_hyp, R.SEED + 1)[0], ids)
    assert not np.array_equal(R.draw(n, n_hyp, R.SEED, 2 ** 40)[0], ids)


def test_forced_positive_goes_to_a_rendered_view_slot():
    n, n_hyp = 512, 6
    plain = R.draw(n, n_hyp, R.SEED, p_force_positive=0.0)[0]
    always = R.draw(n, n_hyp, R.SEED, p_force_positive=1.0)[0]
    absent = ~(plain == 0).any(1)
    assert absent.sum() > 400 and (always == 0).any(1).all()
    assert np.array_equal(always[~absent], plain[~absent])
    assert (always[absent, 0] == 0).all() and np.array_equal(always[absent, 1:], plain[absent, 1:])  # n_rendered_views == 1: slot 0
    three = R.draw(n, n_hyp, R.SEED, n_rendered_views=3, p_force_positive=1.0)[0]
    slots = np.argmax(three[absent] == 0, axis=1)
    assert set(slots.tolist()) == {0, 1, 2}


def test_positive_share():
    # 4096 images, n_hyp = 6: P(positive) = 6/104 + (1 - 6/104) 0.7 = 0.7173; 4 binomial standard deviations = 0.028.
    # Measured with this seed: 0.7078 (2899 of 4096).
    ids, pos = R.draw(4096, 6, R.SEED)
    share = float((pos.sum(1) > 0).mean())
    print(f"share of images with a positive: {share:.4f}")
    expected = 6 / 104 + (1 - 6 / 104) * 0.7
    assert abs(expected - 0.7173) < 1e-4 and abs(share - expected) <= 0.028


def test_bce_against_torch_float64():
    import torch

    x = np.array([0.0, 1e-4, -1e-4, 30.0, -30.0, 200.0, -200.0, 0.3, -2.5], np.float32)
    for T in (1.0, 0.5):
        for y in (np.zeros_like(x), np.ones_like(x)):
            loss, grad = R.bce_logits(x, y, T)
            xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
            want = torch.nn.BCEWithLogitsLoss(reduction="none")(xt / T, torch.tensor(y, dtype=torch.float64))
            want.sum().backward()
            assert np.isfinite(loss).all() and np.isfinite(grad).all()
            # torch forms (1 - y) x + max(-x, 0) + log(exp(-max) + exp(-x - max)): where |x| is large and the loss small its sum
            # cancels and is good to a few spacings of |x| only (it gives 0 for 1.4e-87): that is the allowance, not a relative one
            np.testing.assert_allclose(loss, want.detach().numpy(), rtol=1e-14, atol=4 * np.spacing(np.abs(x / T).max()))
            np.testing.assert_allclose(grad, xt.grad.numpy(), rtol=1e-13, atol=1e-300)
    # the saturated branch keeps its relative accuracy: log1p(exp(-30)) = exp(-30) (1 - exp(-30) / 2 + ...)
    assert abs(R.bce_logits([-30.0], [0.0])[0][0] / np.exp(-30.0) - 1) <= 1e-12
    assert abs(R.bce_logits([200.0], [1.0])[0][0] / np.exp(-200.0) - 1) <= 1e-12
