"""The BPnP oracle's first-order option and the small-rotation scenes, on the CPU.

tests/test_gpu_bpnp.py needs a reference at w = 0 exactly, where the stock oracle (kornia's blended
formula under autograd) is NaN: the unused Rodrigues branch contributes 0 * (gradient of sqrt at 0).
oracle.bpnp_oracle's first_order=True evaluates the first-order branch alone; here it is shown equal
to the stock oracle where both exist (|w| = 5e-4), and finite at 0 where the stock one is not."""
import numpy as np
import pytest
import torch

import bpnp_cases as bc
from oracle import bpnp_oracle as bo
from test_bpnp import K_LM


def test_first_order_option_equals_stock_oracle_below_the_switch():
    rng = np.random.default_rng(0)
    x, z, y = bc.small_rotation_case(rng, 5e-4, 2, 9, per_crop=False)
    assert all(0 < bc.theta2_f32(v) < bc.SWITCH2 for v in y)
    g = rng.normal(size=(2, 6))
    stock = bo.bpnp_backward(x, y, z, K_LM, g, dtype=torch.float64)
    first = bo.bpnp_backward(x, y, z, K_LM, g, dtype=torch.float64, first_order=True)
    for a, b in zip(stock, first):
        assert torch.isfinite(a).all()
        assert (a - b).abs().max() <= 1e-12 * a.abs().max()
    R = bo.angle_axis_to_rotation_matrix(torch.tensor(y[:, :3], dtype=torch.float64))
    assert torch.equal(R, bo.angle_axis_to_rotation_matrix(torch.tensor(y[:, :3], dtype=torch.float64), True))


def test_stock_oracle_is_nan_at_zero_and_first_order_is_not():
    rng = np.random.default_rng(1)
    x, z, y = bc.small_rotation_case(rng, 0.0, 1, 9, per_crop=False)
    assert not y[0, :3].any()
    g = rng.normal(size=(1, 6))
    stock = bo.bpnp_backward(x, y, z, K_LM, g, dtype=torch.float64)
    first = bo.bpnp_backward(x, y, z, K_LM, g, dtype=torch.float64, first_order=True)
    assert not torch.isfinite(stock[0]).all()
    assert all(torch.isfinite(a).all() and a.abs().max() > 0 for a in first)


@pytest.mark.parametrize("mag", bc.SMALL_W)
@pytest.mark.parametrize("per_crop", [False, True])
def test_small_rotation_case_is_a_noisy_minimum_on_its_side(mag, per_crop):
    rng = np.random.default_rng(int(mag * 1e6) + per_crop)
    bs, n = 2, 40
    x, z, y = bc.small_rotation_case(rng, mag, bs, n, per_crop)
    for b in range(bs):
        zb = z[b] if per_crop else z
        assert (bc.theta2_f32(y[b]) > bc.SWITCH2) == (mag > 1e-3)
        assert abs(np.sqrt(bc.theta2_f32(y[b])) - mag) < 1e-6
        again = bo.lm_refine(x[b], zb, K_LM, y[b])
        assert np.abs(again - y[b]).max() < 2e-7 * max(1.0, np.abs(y[b]).max())  # f32 rounding of the pose
        rms = np.sqrt(np.mean((bc.project(y[b], zb) - x[b]) ** 2))
        assert 0.5 < rms < 1.1  # noise 0.8 less the six fitted directions


def test_near_pi_scenes_angles():
    x, z, y = bc.near_pi_scenes(np.random.default_rng(2), 100, 0.3)
    ang = np.linalg.norm(y[:, :3], axis=1)
    assert (np.pi - ang[:6] <= 1e-3 + 1e-12).all() and (ang[:6] <= np.pi).all() and (ang[6:] < 2.5).all()
    assert x.shape == (8, 100, 2) and (y[:, 5] > 0.5).all()
