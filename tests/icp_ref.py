"""numpy f64 restatement of the ICP pose refinement (krrn_icp_refine_f32; the definition is
include/krrn_hip.h's and DESIGN.md section 3's: the reference project has no ICP), the figures that
say how far every discrete decision of a run was from going the other way, and the seeded scene
family the ICP tests share (test infrastructure, like tests/umeyama_ref.py).

    res = icp(R0, t0, cloud, model, max_dist, max_iter=20, tol=1e-4, min_pairs=6)
    res['R'], res['t']                   the refined pose (f64)
    res['passes'], res['pairs'], res['rmse'], res['status'], res['nn_idx']   describe that pose
    res['nn_prev']                       the pairs of the pass before the last (None after one pass)
    res['margins']  nn_gap / thr_gap / conv_gap / sigma; check_conditions(res) asserts their limits

    sc = scene('work')                    # dict: R0, t0, cloud, model (f32), max_dist, kw, R_gt, t_gt
"""
import functools

import numpy as np

MAX_ITER = 20
TOL = 1e-4
MIN_PAIRS = 6
CONVERGED, MAX_ITER_HIT, STARVED, DEGENERATE = 0, 1, 2, 3

# conditions, not tolerances: where they hold, a bit-different f64 evaluation reaches the same decisions
MIN_NN_GAP = 1e-10      # (second - best) / second over every pass and point (exact duplicates of the best excluded)
MIN_THR_GAP = 1e-9      # |d^2 - max_dist^2| / max_dist^2 over every pass and point
MIN_CONV_GAP = 1e-6     # ||err_{k-1} - err_k| - tol err_{k-1}| / (tol err_{k-1}) over every pass k >= 1 that tests it
MIN_SIGMA_RATIO = 1e-3  # s2 / s1 of the covariance of every Kabsch update that gave a pose (umeyama_ref's limit)

_ROWS = 512  # cloud points per block of the brute-force distance table


def nearest(Q, Mo):
    """Brute force: (j, d2, gap) per row of Q [N, 3] against Mo [M, 3]; argmin takes the lowest index
    among equal distances. gap = (second - best) / second with exact duplicates of the best left out.
    A NaN distance (a non-finite cloud or model point) counts as +inf, as the kernel's strict `<` has it: a
    non-finite model point pairs with nothing, a non-finite cloud point has d2 = inf."""
    N = Q.shape[0]
    j = np.zeros(N, np.int64)
    d2 = np.zeros(N)
    gap = np.ones(N)
    for lo in range(0, N, _ROWS):
        q = Q[lo:lo + _ROWS]
        dx = q[:, None, 0] - Mo[None, :, 0]
        dy = q[:, None, 1] - Mo[None, :, 1]
        dz = q[:, None, 2] - Mo[None, :, 2]
        D = (dx * dx + dy * dy) + dz * dz
        D = np.where(np.isnan(D), np.inf, D)  # a NaN distance never wins (numpy's argmin would pick it)
        jj = np.argmin(D, axis=1)
        best = D[np.arange(len(q)), jj]
        with np.errstate(invalid="ignore", over="ignore"):
            second = np.where(D > best[:, None], D, np.inf).min(axis=1)
            g = np.where(np.isfinite(second), (second - best) / second, 1.0)
        j[lo:lo + _ROWS], d2[lo:lo + _ROWS], gap[lo:lo + _ROWS] = jj, best, g
    return j, d2, gap


def kabsch(Mk, Pk):
    """R, t, s2 / s1 of p ~ R m + t on the pairs (two-pass covariance, R = U diag(1, 1, sign) V^T); None where
    the pair set has no second direction (the kernel divides by the second singular value: not finite)."""
    K = Mk.shape[0]
    mm, mp = Mk.sum(0) / K, Pk.sum(0) / K
    cov = (Pk - mp).T @ (Mk - mm) / K
    U, D, Vt = np.linalg.svd(cov)
    if not (np.isfinite(D).all() and D[1] > 0.0):
        return None
    sign = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0.0 else 1.0
    R = U @ np.diag([1.0, 1.0, sign]) @ Vt
    t = mp - R @ mm
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        return None
    return R, t, float(D[1] / D[0])


def icp(R0, t0, cloud, model, max_dist, max_iter=MAX_ITER, tol=TOL, min_pairs=MIN_PAIRS):
    R0, t0 = np.asarray(R0, np.float32).reshape(3, 3), np.asarray(t0, np.float32).reshape(3)
    P = np.asarray(cloud, np.float32).astype(np.float64)
    Mo = np.asarray(model, np.float32).astype(np.float64)
    md = float(np.float32(max_dist))
    md2 = md * md
    R, t = R0.astype(np.float64), t0.astype(np.float64)
    nn_gap = thr_gap = conv_gap = sigma = np.inf
    err_prev = nn_prev = None
    for k in range(max_iter + 1):
        with np.errstate(invalid="ignore", over="ignore"):
            Q = (P - t) @ R  # rows R^T (p - t)
            j, d2, gap = nearest(Q, Mo)
            keep = d2 < md2
        fin = np.isfinite(d2)
        if fin.any():
            nn_gap = min(nn_gap, float(gap[fin].min()))
            # max_dist 0 (d2 < 0: never) and +inf (a finite d2 < inf: always) are decided without rounding
            if 0.0 < md2 < np.inf:
                thr_gap = min(thr_gap, float((np.abs(d2[fin] - md2) / md2).min()))
        K = int(keep.sum())
        err = float(d2[keep].sum() / K) if K else np.nan
        status = None
        if K < min_pairs:
            status = STARVED
        else:
            if k >= 1:
                lim = tol * err_prev
                if lim > 0.0:
                    conv_gap = min(conv_gap, abs(abs(err_prev - err) - lim) / lim)
                if abs(err_prev - err) <= lim:
                    status = CONVERGED
            if status is None and k == max_iter:
                status = MAX_ITER_HIT
        if status is None:
            new = kabsch(Mo[j[keep]], P[keep])
            if new is None:
                status = DEGENERATE
        if status is not None:
            return dict(R=R, t=t, passes=k + 1, pairs=K, rmse=float(np.sqrt(err)) if K else np.inf, status=status,
                        nn_idx=np.where(keep, j, -1).astype(np.int32), nn_prev=nn_prev,
                        margins=dict(nn_gap=nn_gap, thr_gap=thr_gap, conv_gap=conv_gap, sigma=sigma))
        R, t = new[:2]
        sigma = min(sigma, new[2])
        err_prev = err
        nn_prev = np.where(keep, j, -1).astype(np.int32)
    raise AssertionError("unreachable: pass max_iter always stops")


def check_conditions(res):
    m = res["margins"]
    assert m["nn_gap"] >= MIN_NN_GAP, m
    assert m["thr_gap"] >= MIN_THR_GAP, m
    assert m["conv_gap"] >= MIN_CONV_GAP, m
    assert m["sigma"] >= MIN_SIGMA_RATIO, m


def add(R, t, Rg, tg, model):
    """ADD: mean distance between the model under (R, t) and under (Rg, tg)."""
    Mo = np.asarray(model, np.float64)
    return float(np.linalg.norm((Mo @ np.asarray(R, np.float64).T + t) - (Mo @ Rg.T + tg), axis=1).mean())


# ---- scenes -------------------------------------------------------------------------------------------------------

MAX_DIST = 0.02


def rodrigues(axis, deg):
    k = axis / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make_model(rng, M):
    """M points on a bumpy ellipsoid of about 0.12 x 0.08 x 0.06 m (f32)."""
    u = rng.normal(size=(M, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = 1.0 + 0.1 * np.sin(5.0 * u[:, 0]) * np.cos(4.0 * u[:, 1]) + 0.05 * np.sin(7.0 * u[:, 2])
    return (u * r[:, None] * np.array([0.06, 0.04, 0.03])).astype(np.float32)


def make_scene(seed, N, M, noise=1e-3, rot_deg=5.0, dt=0.01, out_frac=0.0, shift=0.0, model=None, half=True):
    """A model, a ground-truth pose at about (0.05, -0.03, 0.8) m, a cloud of N points drawn from the half
    of the model nearest the camera (Gaussian noise, an out_frac share displaced by +-0.2 m per axis, the
    whole cloud moved by `shift` m along z; half=False draws from the whole model) and a start pose: the ground
    truth turned by rot_deg about a random axis and moved by N(0, dt)."""
    rng = np.random.default_rng(seed)
    model = make_model(rng, M) if model is None else np.asarray(model, np.float32)
    Rg = rodrigues(rng.normal(size=3), rng.uniform(0.0, 360.0))
    tg = np.array([0.05, -0.03, 0.8]) + rng.normal(scale=0.01, size=3)
    pc = model.astype(np.float64) @ Rg.T + tg
    near = np.argsort(pc[:, 2], kind="stable")[:max(model.shape[0] // 2, 1) if half else model.shape[0]]
    pick = rng.choice(near, N, replace=True)
    c = pc[pick] + (rng.normal(scale=noise, size=(N, 3)) if noise else 0.0)
    out = rng.random(N) < out_frac
    c[out] += rng.choice([-0.2, 0.2], size=(int(out.sum()), 3))
    c[:, 2] += shift
    R0 = rodrigues(rng.normal(size=3), rot_deg) @ Rg
    t0 = tg + rng.normal(scale=dt, size=3)
    return dict(R0=R0.astype(np.float32), t0=t0.astype(np.float32), cloud=c.astype(np.float32), model=model,
                max_dist=MAX_DIST, kw={}, R_gt=Rg, t_gt=tg, pick=pick)


# name -> (N, M, generator arguments, icp arguments); the noisy ones are NOISY
SPECS = {
    "tiny": (8, 8, dict(noise=0.0, rot_deg=1.0, dt=0.001), dict(min_pairs=3)),
    "odd": (257, 65, {}, {}),
    "outl": (300, 513, dict(out_frac=0.2), {}),
    "work": (1000, 2600, {}, {}),
    "max": (4096, 4096, {}, dict(max_iter=5)),
    "dup": (130, 65, {}, {}),
    "far": (100, 130, dict(shift=1.0), {}),
    "exact": (64, 100, dict(noise=0.0, rot_deg=3.0, dt=0.003), {}),
}
SCENES = tuple(SPECS)
NOISY = ("odd", "outl", "work", "max", "dup")


@functools.lru_cache(maxsize=None)
def scene(name, seed=0):
    """The named scene (read-only: shared between tests). `dup` stores its 65 model points twice; its
    'model65' is the single copy."""
    N, M, gen, kw = SPECS[name]
    sc = make_scene(seed + 100 * SCENES.index(name), N, M, **gen)
    sc["kw"] = dict(kw)
    if name == "dup":
        sc["model65"] = sc["model"]
        sc["model"] = np.concatenate([sc["model"], sc["model"]])
    for v in sc.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sc


@functools.lru_cache(maxsize=None)
def reference(name, seed=0):
    """icp() of the named scene, computed once per process."""
    sc = scene(name, seed)
    return icp(sc["R0"], sc["t0"], sc["cloud"], sc["model"], sc["max_dist"], **sc["kw"])


def mixed_batch():
    """Five N = 257 / M = 65 crops with their own max_dist: noisy, outliers, a far crop (STARVED in pass
    0), a noise-free one (stops early) and a tight max_dist."""
    gens = [dict(), dict(out_frac=0.2), dict(shift=1.0), dict(noise=0.0, rot_deg=1.0, dt=0.001), dict(rot_deg=2.0)]
    scs = [make_scene(900 + i, 257, 65, **g) for i, g in enumerate(gens)]
    md = np.array([0.02, 0.02, 0.02, 0.02, 0.012], np.float32)
    return scs, md
