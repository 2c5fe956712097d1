"""csrc/bpnp.hip where tests/test_bpnp.py does not reach (GPU): the log map of R_init over the angle
set of tests/so3_ref.py, both branches of the rotation formula around |w| = 1e-3 in the backward and
the forward kernel, one wave's edge sizes n in {3, 64, 65}, per-crop points and cost_out in `solve`,
more crops than one launch's first wave of blocks, and the rotation BPnPModle returns for crops seen
near 180 degrees.

Bounds. Log map: 4 x the largest rebuild error of so3_ref.log_ref over the same set (1.248e-7 on the
CPU, so 4.99e-7; tests/test_so3_host.py holds the header's host build to the same bound and measured
1.248e-7). Gradients: 1e-5 of each gradient's max against the f64 oracle, and poses 2e-6 against the
oracle's LM, both the project's figures (tests/test_bpnp.py). cost_out: 1e-6 relative to the f64 cost
at the returned pose plus 2 n (4e-5 px)^2: the f32 rounding of the returned pose (2^-24 |y|, |w| <=
2.5) moves a pixel by up to 3.2e-5 px (124 px / rad for points 0.13 m from the centre at 0.6 m depth),
which is all the cost a zero-residual fit (n = 3) has."""
import numpy as np
import pytest
import torch

import bpnp_cases as bc
import so3_ref
from oracle import bpnp_oracle as bo
from test_bpnp import K_LM, scene

pytestmark = pytest.mark.gpu


def _f(dev):
    return lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)


def _cost64(y, x, z):
    e = bo._residual(np.asarray(y, np.float64), np.asarray(x, np.float64), np.asarray(z, np.float64),
                     K_LM.astype(np.float32).astype(np.float64))
    return float(e @ e)


def _check_cost(cost, y, x, z, per_crop):
    """cost_out [bs] against the f64 cost at the returned (f32) pose, inputs as the kernel read them."""
    x32, z32 = np.asarray(x, np.float32), np.asarray(z, np.float32)
    n = x32.shape[1]
    for b in range(len(y)):
        want = _cost64(y[b], x32[b], z32[b] if per_crop else z32)
        assert abs(float(cost[b]) - want) <= 1e-6 * want + 2 * n * 4e-5 ** 2, (b, float(cost[b]), want)


def test_rot_log_through_the_solve_kernel(dev):
    """krrn_bpnp_solve_f32 with R_init and iters = 0 returns rot_log(R_init) in y_out[:, :3], leaves
    y_init's translation, and reports the cost at that pose: one crop per matrix of
    so3_ref.rotation_set(), a single launch."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import ptr, stream_ptr
    R, ang = so3_ref.rotation_set()
    B, n = len(R), 5
    rng = np.random.default_rng(0)
    z = bc.points(rng, n).astype(np.float32)
    x = (rng.random((B, n, 2)) * np.array([640.0, 480.0])).astype(np.float32)  # residuals of 100s of pixels
    y0 = np.concatenate([rng.normal(size=(B, 3)), np.stack([bc.translation(rng) for _ in range(B)])], 1).astype(np.float32)
    f = _f(dev)
    xt, zt, Kt, yt, Rt = f(x), f(z), f(K_LM), f(y0), f(R.reshape(B, 9))
    y = torch.full((B, 6), float("nan"), dtype=torch.float32, device=dev)
    cost = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    _lib.call("krrn_bpnp_solve_f32", ptr(xt), ptr(zt), 0, ptr(Kt), ptr(yt), ptr(Rt), B, n, 0, ptr(y), ptr(cost),
              stream_ptr(dev))
    y, cost = y.cpu().numpy(), cost.cpu().numpy()
    assert np.isfinite(y).all() and np.array_equal(y[:, 3:], y0[:, 3:])
    err = so3_ref.rebuild_error(y[:, :3], R)
    bound = 4 * so3_ref.rebuild_error(so3_ref.log_ref(R), R).max()
    print(f"rot_log on the GPU: max rebuild error {err.max():.3e} at angle {ang[err.argmax()]!r}, bound {bound:.3e}")
    assert err.max() <= bound, (err.max(), ang[err.argmax()], bound)
    for b in range(B):
        want = _cost64(y[b], x[b], z)
        assert abs(float(cost[b]) - want) <= 1e-6 * want, (b, ang[b], float(cost[b]), want)


@pytest.mark.parametrize("mag", bc.SMALL_W)
@pytest.mark.parametrize("per_crop", [False, True])
def test_bpnp_small_rotations(dev, mag, per_crop):
    """backward at the LM minimum of noisy scenes on either side of |w| = 1e-3 (and at w = 0, where
    the reference is the oracle's first-order branch alone), and solve from a perturbed guess to the
    same minimum."""
    from pose_estimation_amd import bpnp
    rng = np.random.default_rng(int(mag * 1e6) + 10 * per_crop)
    bs, n = 3, 40
    x, z, y = bc.small_rotation_case(rng, mag, bs, n, per_crop)
    g = rng.normal(size=(bs, 6)).astype(np.float32)
    f = _f(dev)
    gx, gz, gK = bpnp.backward(f(x), f(y), f(z), f(K_LM), f(g))
    rx, rz, rK = bo.bpnp_backward(x.astype(np.float32), y, z.astype(np.float32), K_LM.astype(np.float32), g,
                                  dtype=torch.float64, first_order=mag == 0.0)
    for name, got, ref in (("x", gx, rx), ("z", gz, rz), ("K", gK, rK)):
        got, ref = got.cpu().double(), ref.double()
        assert got.shape == ref.shape and torch.isfinite(ref).all()
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"|w|={mag} per_crop={per_crop} grad_{name}: {err:.2e} of its max (bound 1e-5)")
        assert err < 1e-5, (name, err)
    y0 = y + np.concatenate([rng.normal(size=(bs, 3)) * 0.05, rng.normal(size=(bs, 3)) * 0.01], axis=1).astype(np.float32)
    got, cost = bpnp.solve(f(x), f(z), f(K_LM), ini_pose=f(y0), return_cost=True)
    got = got.cpu().double().numpy()
    for b in range(bs):
        zb = (z[b] if per_crop else z).astype(np.float32)
        ref = bo.lm_refine(x[b].astype(np.float32), zb, K_LM.astype(np.float32), y0[b])
        assert np.abs(got[b] - ref).max() < 2e-6, (b, got[b], ref)
    _check_cost(cost.cpu().numpy(), got, x, z, per_crop)


def _case(rng, bs, n, noise, per_crop):
    xs, zs, ys = zip(*[scene(rng, n, noise) for _ in range(bs)])
    if per_crop:
        return np.stack(xs), np.stack(zs), np.stack(ys)
    z = zs[0]
    return np.stack([bc.project(y, z) + noise * rng.normal(size=(n, 2)) for y in ys]), z, np.stack(ys)


@pytest.mark.parametrize("n", [3, 64, 65])
@pytest.mark.parametrize("per_crop", [False, True])
def test_bpnp_wave_edge_sizes(dev, n, per_crop):
    """n = 3 (the least the ABI takes: 61 idle lanes), 64 (every lane one point) and 65 (lane 0 a
    second point): solve with cost_out, then backward at the solution."""
    from pose_estimation_amd import bpnp
    rng = np.random.default_rng(200 + n + per_crop)
    bs = 3
    x, z, y = _case(rng, bs, n, 0.5, per_crop)
    y0 = (y + np.concatenate([rng.normal(size=(bs, 3)) * 0.02, rng.normal(size=(bs, 3)) * 0.005], axis=1)).astype(np.float32)
    f = _f(dev)
    got, cost = bpnp.solve(f(x), f(z), f(K_LM), ini_pose=f(y0), return_cost=True)
    got32 = got.cpu().numpy()
    for b in range(bs):
        zb = (z[b] if per_crop else z).astype(np.float32)
        ref = bo.lm_refine(x[b].astype(np.float32), zb, K_LM.astype(np.float32), y0[b])
        assert np.abs(got32[b].astype(np.float64) - ref).max() < 2e-6, (b, got32[b], ref)
    _check_cost(cost.cpu().numpy(), got32, x, z, per_crop)
    g = rng.normal(size=(bs, 6)).astype(np.float32)
    gx, gz, gK = bpnp.backward(f(x), got, f(z), f(K_LM), f(g))
    rx, rz, rK = bo.bpnp_backward(x.astype(np.float32), got32, z.astype(np.float32), K_LM.astype(np.float32), g,
                                  dtype=torch.float64)
    for name, a, ref in (("x", gx, rx), ("z", gz, rz), ("K", gK, rK)):
        a, ref = a.cpu().double(), ref.double()
        assert a.shape == ref.shape
        err = (a - ref).abs().max().item() / ref.abs().max().item()
        print(f"n={n} per_crop={per_crop} grad_{name}: {err:.2e} of its max (bound 1e-5)")
        assert err < 1e-5, (name, err)


def test_bpnp_solve_seventy_crops(dev):
    """B = 70 crops with their own points: every crop's pose and cost are its own."""
    from pose_estimation_amd import bpnp
    rng = np.random.default_rng(70)
    bs, n = 70, 12
    x, z, y = _case(rng, bs, n, 0.5, True)
    y0 = (y + np.concatenate([rng.normal(size=(bs, 3)) * 0.02, rng.normal(size=(bs, 3)) * 0.005], axis=1)).astype(np.float32)
    f = _f(dev)
    got, cost = bpnp.solve(f(x), f(z), f(K_LM), ini_pose=f(y0), return_cost=True)
    got = got.cpu().numpy()
    for b in range(bs):
        ref = bo.lm_refine(x[b].astype(np.float32), z[b].astype(np.float32), K_LM.astype(np.float32), y0[b])
        assert np.abs(got[b].astype(np.float64) - ref).max() < 2e-6, (b, got[b], ref)
    _check_cost(cost.cpu().numpy(), got, x, z, True)


def test_bpnp_end_to_end_near_pi(dev):
    """BPnPModle without ini_pose (EPnP-RANSAC rotation -> log map -> LM) on outlier-free scenes
    whose rotation is within 1e-3 of pi, and two ordinary ones: the rotation as well as the
    translation, both to 5e-3 (tests/test_bpnp.py's figure for t)."""
    from pose_estimation_amd.bpnp import BPnPModle
    torch.manual_seed(0)  # ransac_init draws its subsets with torch's generator
    x, z, y = bc.near_pi_scenes(np.random.default_rng(8), 100, 0.3)
    f = _f(dev)
    P6 = BPnPModle()(f(x), f(z), f(K_LM)).cpu().double().numpy()
    assert np.isfinite(P6).all()
    dR = np.abs(so3_ref.rodrigues_exact(P6[:, :3]) - so3_ref.rodrigues_exact(y[:, :3])).reshape(len(y), -1).max(1)
    dt = np.abs(P6[:, 3:] - y[:, 3:]).max(1)
    print(f"end to end: max |R - R_true| {dR.max():.2e}, max |t - t_true| {dt.max():.2e} (bound 5e-3)")
    assert dR.max() <= 5e-3, dR
    assert dt.max() <= 5e-3, dt
