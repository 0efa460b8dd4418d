"""The float64 restatement the GPU tests of the forward-loss step compare with (tests/training_ref.py), checked on its own: the
box initialisation against the reference's golden, the Euler convention against scipy, the Philox / Box-Muller draw against the
moments of a normal distribution, and the meter arithmetic against the reference's formulas written out.  No GPU."""

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import training_ref as R  # noqa: E402


def test_tco_init_from_boxes_equals_the_reference_golden(golden_dir):
    g = np.load(golden_dir / "g4_pose_update.npz")
    for dtype in (np.float64, np.float32):  # the tolerance tests/test_oracle_golden.py holds the oracle to
        np.testing.assert_allclose(R.TCO_init_from_boxes((1.0, 1.0), g["det_boxes"], g["K"], dtype), g["init_v0"], rtol=1e-6, atol=1e-6)


def test_euler_matrix_is_scipys_extrinsic_xyz():
    from scipy.spatial.transform import Rotation

    rs = np.random.RandomState(0)
    ang = np.concatenate([rs.uniform(-np.pi, np.pi, (64, 3)), R.BIG_ANGLES.astype(np.float64), np.zeros((1, 3))])
    assert np.abs(R.euler2mat(ang) - Rotation.from_euler("xyz", ang).as_matrix()).max() <= 1e-12
    assert np.abs(R.euler2mat(ang, axes="rxyz") - Rotation.from_euler("XYZ", ang).as_matrix()).max() <= 1e-12
    # the case the GPU test uses to tell the conventions apart: they differ by far more than any rounding
    assert np.abs(R.euler2mat(R.BIG_ANGLES) - R.euler2mat(R.BIG_ANGLES, axes="rxyz")).max() > 0.5


def test_add_noise_composes_on_the_right_and_keeps_the_bottom_row():
    rs = np.random.RandomState(1)
    T = R.random_poses(rs, 5)
    T[:, 3] = (0.5, -1.0, 2.0, 3.0)  # not a rigid transform's bottom row: it is copied, not rebuilt
    nz = (rs.normal(size=(15, 6)) * 0.3).astype(np.float32)
    out = R.add_noise(T, nz, repeat=3)
    T3 = np.repeat(T, 3, axis=0).astype(np.float64)
    assert np.abs(out[:, :3, :3] - T3[:, :3, :3] @ R.euler2mat(nz[:, :3])).max() <= 1e-15
    assert np.array_equal(out[:, :3, 3], T3[:, :3, 3] + nz[:, 3:].astype(np.float64)) and np.array_equal(out[:, 3], T3[:, 3])
    zero = R.add_noise(T, np.zeros((5, 6), np.float32))
    assert np.array_equal(zero, T.astype(np.float64))


def test_drawn_normals_have_the_moments_of_a_normal_distribution():
    n = 4096
    z = R.normals(n, R.SEED)
    assert np.isfinite(z).all()
    # five standard errors: sigma / sqrt(n) of the mean, sigma / sqrt(2 n) of the standard deviation
    assert (np.abs(z.mean(0)) <= 5.0 / np.sqrt(n)).all(), z.mean(0)
    assert (np.abs(z.std(0) - 1.0) <= 5.0 / np.sqrt(2 * n)).all(), z.std(0)
    # the six columns are not copies of each other, rows depend on (seed, row_offset + i) alone
    c = np.corrcoef(z.T)
    assert np.abs(c - np.eye(6)).max() <= 5.0 / np.sqrt(n)
    assert np.array_equal(R.normals(64, R.SEED, 100), z[100:164]) and not np.array_equal(R.normals(64, R.SEED + 1), z[:64])
    assert not np.array_equal(R.noise_words(1, R.SEED, 2 ** 32), R.noise_words(1, R.SEED, 0))  # the row's high word counts
    scaled = R.draw_noise(n, R.SEED, 0, (15, 0, 15), (0.01, 0.01, 0))
    assert (scaled[:, 1] == 0).all() and (scaled[:, 5] == 0).all()
    np.testing.assert_allclose(scaled[:, 0], z[:, 0] * np.deg2rad(15.0), rtol=1e-15)
    np.testing.assert_allclose(scaled[:, 3], z[:, 3] * np.float64(np.float32(0.01)), rtol=1e-15)


def test_float32_evaluation_stays_close_to_the_float64_one():
    """The yardsticks of the GPU tests are rounding, not something larger: a few float32 ulp of the values' size."""
    for n, repeat in R.EXPLICIT_CASES:
        TCO, noise = R.explicit_case(n, repeat)
        y = R.yardstick(R.add_noise(TCO, noise, repeat, np.float32), R.add_noise(TCO, noise, repeat))
        assert 0 < y <= 16 * 2.0 ** -24 * 1.5, (n, repeat, y)
    y = R.yardstick(R.draw_noise(257, R.SEED, 0, R.EULER_DEG_STD, R.TRANS_STD, np.float32), R.draw_noise(257, R.SEED, 0, R.EULER_DEG_STD, R.TRANS_STD))
    assert 0 < y <= 64 * 2.0 ** -24, y


def test_meter_arithmetic_is_the_references():
    rs = np.random.RandomState(3)
    B, H, n_it, alpha = 3, 2, 2, 0.5
    losses = [rs.uniform(0, 1, B * H) for _ in range(n_it)]
    parts = [{k: rs.uniform(0, 1, B * H) for k in ("loss_orn", "loss_xy", "loss_z")} for _ in range(n_it)]
    m, total = R.megapose_meters(losses, parts, B, H, alpha)
    assert set(m) | {"time_render"} == R.megapose_meter_keys(n_it)
    # every mean is over equally many terms: they all reduce to plain means over (iteration, image, hypothesis)
    assert np.isclose(m["loss_TCO"], np.mean(losses)) and np.isclose(total, alpha * np.mean(losses))
    assert np.isclose(m["loss_TCO-iter=2"], losses[1].mean()) and np.isclose(m["loss_TCO-iter=1-loss_xy"], parts[0]["loss_xy"].mean())
    m, total = R.h_pose_meters(losses)
    assert set(m) == R.h_pose_meter_keys(n_it) and np.isclose(total, np.mean(losses)) and m["loss_TCO"] == total
