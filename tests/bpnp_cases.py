"""Scenes for the BPnP kernels' small-rotation and near-pi tests (test infrastructure: pinned on the
CPU by tests/test_bpnp_oracle_host.py, run on the GPU by tests/test_gpu_bpnp.py).

kornia's angle_axis_to_rotation_matrix switches from Rodrigues to I + [w]x at theta^2 <= 1e-6, i.e.
|w| = 1e-3, and tests/test_bpnp.py draws |w| in [0.3, 2.5]. A noisy scene's least-squares pose lies
several 1e-3 from the true one, so a scene drawn at |w| = 9.9e-4 would land on either side of the
switch; `stationary_scene` therefore shapes the noise so that the pose it was drawn at stays the
minimum (the part of the noise inside the Jacobian's column space is taken out, which leaves
J^T e = 0 with |e| about the noise asked for). `small_rotation_case` still checks the side the
f32-rounded solution lies on, and draws again if it is not the intended one."""
import numpy as np

from oracle import bpnp_oracle as bo
from test_bpnp import K_LM

SWITCH2 = bo.KORNIA_EPS  # theta^2 at which the rotation formula switches
SMALL_W = [0.0, 5e-4, 9.9e-4, 1.01e-3, 2e-3]


def points(rng, n):
    return (rng.random((n, 3)) - 0.5) * 0.15


def translation(rng):
    return np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.1)])


def project(y, z):
    return bo._residual(np.asarray(y, np.float64), np.zeros((len(z), 2)), z, K_LM).reshape(len(z), 2)


def stationary_scene(rng, z, y, noise):
    """Pixels x [n, 2] whose summed squared reprojection error has a stationary point at y with
    residuals of about `noise` pixels."""
    n = len(z)
    e = noise * rng.normal(size=2 * n)
    J = np.empty((2 * n, 6))
    for j in range(6):
        h = 1e-7 * max(1.0, abs(y[j]))
        d = np.zeros(6)
        d[j] = h
        J[:, j] = (project(y + d, z) - project(y - d, z)).reshape(-1) / (2 * h)
    e -= J @ np.linalg.solve(J.T @ J, J.T @ e)
    return project(y, z) - e.reshape(n, 2)  # residual pi(z; y) - x = e


def theta2_f32(y):
    """theta^2 as the kernels see it: the f32 pose's angle-axis squared and summed in f64."""
    w = np.asarray(y, np.float32)[:3].astype(np.float64)
    return float(w @ w)


def small_rotation_case(rng, mag, bs, n, per_crop, noise=0.8, max_draws=20):
    """(x [bs, n, 2], z [n, 3] or [bs, n, 3], y f32 [bs, 6]): noisy scenes with |w| = mag about random
    axes and y their LM minimum, on the side of the switch mag lies on (mag = 0: w = 0 exactly, the
    translation that of the minimum)."""
    zs = [points(rng, n) for _ in range(bs)] if per_crop else [points(rng, n)] * bs
    xs, ys = [], []
    for b in range(bs):
        for _ in range(max_draws):
            a = rng.normal(size=3)
            y = np.concatenate([mag * a / np.linalg.norm(a), translation(rng)])
            x = stationary_scene(rng, zs[b], y, noise)
            sol = bo.lm_refine(x, zs[b], K_LM, y).astype(np.float32)
            if mag == 0.0:
                sol[:3] = 0.0
            if (theta2_f32(sol) > SWITCH2) == (mag * mag > SWITCH2):
                break
        else:
            raise RuntimeError(f"no scene on the intended side of the switch for |w| = {mag}")
        xs.append(x)
        ys.append(sol)
    return np.stack(xs), (np.stack(zs) if per_crop else zs[0]), np.stack(ys)


def near_pi_scenes(rng, n, noise):
    """(x [8, n, 2], z [n, 3], y [8, 6]): six poses whose rotation is pi - d about random and
    coordinate axes (d from 0 to 1e-3), then two ordinary ones (|w| = 1.1 and 2.3); one shared point
    set, pixel noise `noise`, no outliers."""
    z = points(rng, n)
    ws = []
    for d, axis in ((0.0, None), (1e-5, None), (1e-4, [0, 0, 1.0]), (3e-4, None), (1e-3, [-1.0, 0, 0]), (0.0, [0, 1.0, 0])):
        a = rng.normal(size=3) if axis is None else np.array(axis)
        ws.append((np.pi - d) * a / np.linalg.norm(a))
    for m in (1.1, 2.3):
        a = rng.normal(size=3)
        ws.append(m * a / np.linalg.norm(a))
    ys = np.stack([np.concatenate([w, translation(rng)]) for w in ws])
    xs = np.stack([project(y, z) + noise * rng.normal(size=(n, 2)) for y in ys])
    return xs, z, ys
