"""The SO(3) log map's test set and reference (test infrastructure for csrc/krrn_so3.h).

`rotation_set()` is the set of f32 rotation matrices both the host test (tests/test_so3_host.py,
the header compiled for the CPU) and the GPU test (tests/test_gpu_bpnp.py, the header inside
krrn_bpnp_solve_f32) run; `log_ref` is an f64 log map by another route (Shepperd's quaternion,
then 2 atan2(|q_v|, q_w)) that shares no branch with the header; `rebuild_error` is the measure.
"""
import numpy as np

ANGLES = [0.0, 1e-7, 1e-4, 1e-2, 0.5, 2.0] + [np.pi - d for d in (1.0, 1e-1, 1e-2, 1e-3, 3e-4, 1e-4, 1e-5, 1e-7, 0.0)]
N_RANDOM_AXES = 24


def rodrigues_exact(w):
    """[..., 3] f64 -> [..., 3, 3]: exp([w]x) = I + sin(t)/t [w]x + (1 - cos t)/t^2 [w]x^2, the two
    factors by their series below 1e-4 (no kornia epsilon: this is the exact map)."""
    w = np.asarray(w, np.float64)
    t2 = (w * w).sum(-1)
    t = np.sqrt(t2)
    small = t < 1e-4
    ts = np.where(small, 1.0, t)
    a = np.where(small, 1.0 - t2 / 6.0, np.sin(ts) / ts)
    # 1 - cos t = 2 sin^2(t / 2): no cancellation
    b = np.where(small, 0.5 - t2 / 24.0, 2.0 * np.sin(0.5 * ts) ** 2 / (ts * ts))
    Kx = np.zeros(w.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2] = -w[..., 2], w[..., 1]
    Kx[..., 1, 0], Kx[..., 1, 2] = w[..., 2], -w[..., 0]
    Kx[..., 2, 0], Kx[..., 2, 1] = -w[..., 1], w[..., 0]
    return np.eye(3) + a[..., None, None] * Kx + b[..., None, None] * (Kx @ Kx)


def rotation_set(seed=0):
    """(R f32 [n, 3, 3], angle f64 [n]): every angle of ANGLES about N_RANDOM_AXES random axes and
    the three coordinate axes, both signs of each axis, rounded to f32; then the three exact
    180-degree diagonal matrices (each has another dominant column)."""
    rng = np.random.default_rng(seed)
    mats, angs = [], []
    for th in ANGLES:
        ax = rng.normal(size=(N_RANDOM_AXES, 3))
        ax /= np.linalg.norm(ax, axis=1, keepdims=True)
        ax = np.concatenate([ax, np.eye(3)])
        ax = np.concatenate([ax, -ax])
        mats.append(rodrigues_exact(th * ax).astype(np.float32))
        angs.append(np.full(len(ax), th))
    mats.append(np.stack([np.diag(d) for d in ([1, -1, -1], [-1, 1, -1], [-1, -1, 1])]).astype(np.float32))
    angs.append(np.full(3, np.pi))
    return np.concatenate(mats), np.concatenate(angs)


def log_ref(R):
    """[n, 3, 3] -> [n, 3] f64: Shepperd's quaternion (the largest of w, x, y, z taken from the
    diagonal, the rest from the off-diagonal sums), normalised, then 2 atan2(|q_v|, q_w) q_v / |q_v|."""
    R = np.asarray(R, np.float64)
    out = np.empty((len(R), 3))
    for i, M in enumerate(R):
        tr = M[0, 0] + M[1, 1] + M[2, 2]
        cand = np.array([tr, M[0, 0], M[1, 1], M[2, 2]])
        j = int(np.argmax(cand))
        q = np.empty(4)  # (w, x, y, z) up to scale
        if j == 0:
            q[:] = [1.0 + tr, M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]
        else:
            a = j - 1
            b, c = (a + 1) % 3, (a + 2) % 3
            q[0] = M[c, b] - M[b, c]
            q[1 + a] = 1.0 + 2.0 * M[a, a] - tr
            q[1 + b] = M[b, a] + M[a, b]
            q[1 + c] = M[c, a] + M[a, c]
        q /= np.linalg.norm(q)
        if q[0] < 0:
            q = -q
        nv = np.linalg.norm(q[1:])
        out[i] = 0.0 if nv == 0.0 else 2.0 * np.arctan2(nv, q[0]) * q[1:] / nv
    return out


def log_parent(R):
    """The log map as the kernel had it before krrn_so3.h (branch chosen from sin(acos(c)) with c
    from the trace alone), restated so that the host test can show the set tells the two apart."""
    R = np.asarray(R, np.float64)
    out = np.empty((len(R), 3))
    for i, M in enumerate(R):
        c = min(1.0, max(-1.0, (M[0, 0] + M[1, 1] + M[2, 2] - 1.0) * 0.5))
        th = np.arccos(c)
        s = np.sin(th)
        v = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
        if s > 1e-6:
            out[i] = th / (2.0 * s) * v
        elif c > 0.0:
            out[i] = 0.5 * v
        else:
            k = int(np.argmax(np.diag(M)))
            nk = np.sqrt(max(0.0, (M[k, k] + 1.0) * 0.5))
            nv = np.array([nk if a == k else (M[a, k] + M[k, a]) / (4.0 * nk) for a in range(3)])
            out[i] = (-1.0 if nv @ v < 0.0 else 1.0) * th * nv
    return out


def rebuild_error(w, Rf):
    """Per matrix: max entry |exp([w32]x) - Rf| with w32 the vector rounded to f32 (as the kernel
    stores it) and Rf the f32 input matrix, both taken to f64."""
    w32 = np.asarray(w, np.float64).astype(np.float32).astype(np.float64)
    return np.abs(rodrigues_exact(w32) - np.asarray(Rf, np.float64)).reshape(len(w32), -1).max(1)
