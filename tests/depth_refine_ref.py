"""The render-based point-to-plane depth refiner (krrn_pose_refine_depth_f32; include/krrn_hip.h) restated in
numpy f64, on bop_ref's scene family, with a per-pass trace and decision margins. The render (depth, winning face,
face normal and their edge / depth / flip margins) is raster_ref.render's over the whole frame; this file adds
the refiner's own decisions:
  gate    ||d - z| - max_dist| on every covered pixel with an observed depth (kept or rejected)
  stop    ||err_{k-1} - err_k| / err_{k-1} - tol| in every pass >= 1 that reaches the convergence test
  pivot   the smallest Cholesky pivot over the damped matrix's trace, in every pass that solves
A pixel is decided when its edge, depth, flip and gate margins are >= raster_ref.MARGIN = 1e-9; a case is usable
when no pixel of any pass is undecided and the stop and pivot margins hold the same bound (check_conditions), so
that the kernel's passes, pairs and status must equal these exactly. The per-pixel expressions follow the
kernel's operation order; the sums over pixels are numpy's (pairwise), which moves R, t and rmse by rounding only.

Per crop, R, t = R0, t0 rounded to f32 (the ABI's input format), f64 from there on; pass k = 0, 1, ...: render
under (R, t); keep a pixel iff covered, d = depth / depth_scale > 0, |d - z| < max_dist, mask != 0 when given, and
the face normal n is not zero; p = z (xn, yn, 1), o = d (xn, yn, 1), r = n . (o - p); K kept, err_k = sum r^2 / K.
Stop in this order: K < min_pairs STARVED; k >= 1 and |err_{k-1} - err_k| <= tol err_{k-1} CONVERGED; k == max_iter
MAX_ITER. Else J = [((p - t) / rho) x n, n], A = sum J J^T, b = sum J r, A += damp trace(A) / 6 I, Cholesky (a pivot
that is not > 0 and finite, or a non-finite solution: DEGENERATE with the pose from before); xi = (w, v):
R <- exp(w / rho) R, t <- t + v."""
import functools

import numpy as np

import bop_ref as br
import raster_ref as rr

MAX_ITER = 10
TOL = 1e-4
MIN_PAIRS = 6
DIST_FRAC = 0.2
DAMP = 1e-4
STATUS = ("CONVERGED", "MAX_ITER", "STARVED", "DEGENERATE")
SCENES = br.SCENES


def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def render(verts, faces, R, t, K4, H, W):
    """raster_ref.render over the whole frame: depth, cover, normal [3, H, W] and the margin maps, cut to H x W."""
    S = max(H, W)
    res = rr.render(verts, faces, R, t, K4, 0, 0, S, np.asarray(verts, np.float32)[:1], margins=True)
    m = res["margins"]
    return {"depth": res["depth"][:H, :W], "cover": res["cover"][:H, :W], "normal": res["normal"][:, :H, :W],
            "face": res["face"][:H, :W],
            "margins": {k: m[k][:H, :W] for k in ("edge", "depth", "flip")}}


def cholesky_solve(A, g):
    """(xi or None, pivots) by the kernel's 6 x 6 Cholesky: None when a pivot is not > 0 and finite."""
    n = len(g)
    L = np.zeros((n, n))
    piv = []
    with np.errstate(all="ignore"):
        for j in range(n):
            s = A[j, j]
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            piv.append(float(s))
            if not (s > 0.0) or not np.isfinite(s):
                return None, piv
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, n):
                a = A[i, j]
                for k in range(j):
                    a = a - L[i, k] * L[j, k]
                L[i, j] = a / L[j, j]
        y = np.zeros(n)
        for i in range(n):
            a = g[i]
            for k in range(i):
                a = a - L[i, k] * y[k]
            y[i] = a / L[i, i]
        xi = np.zeros(n)
        for i in range(n - 1, -1, -1):
            a = y[i]
            for k in range(i + 1, n):
                a = a - L[k, i] * xi[k]
            xi[i] = a / L[i, i]
    return (xi if np.isfinite(xi).all() else None), piv


def rodrigues(w):
    th = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    E = np.eye(3)
    if th > 0.0:
        k = w / th
        Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        E = (E + np.sin(th) * Kx) + (1.0 - np.cos(th)) * (Kx @ Kx)
    return E


def refine(verts, faces, R0, t0, K4, depth_obs, depth_scale, max_dist, radius, mask=None, max_iter=MAX_ITER,
           tol=TOL, min_pairs=MIN_PAIRS, damp=DAMP, H=None, W=None):
    """One crop over the whole frame. depth_obs f32 [H, W] raw units (None: a frame index outside [0, F), nothing
    observed; then H, W must be given); mask [H, W] (any non-zero is set) or None. Returns R f32 [3, 3], t f32 [3],
    their f64 values (R64, t64), passes, pairs, rmse (f32), status and the per-pass trace: a list of dicts with K,
    err and the margins (module doc)."""
    if depth_obs is not None:
        H, W = depth_obs.shape
    R_in, t_in = np.asarray(R0, np.float32).reshape(3, 3), np.asarray(t0, np.float32).reshape(3)
    R, t = R_in.astype(np.float64), t_in.astype(np.float64)
    fx, fy, cx, cy = (np.float64(np.float32(k)) for k in K4)
    max_dist, rho = np.float64(max_dist), np.float64(radius)
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xn, yn = (cols - cx) / fx, (rows - cy) / fy
    with np.errstate(all="ignore"):
        d = np.zeros((H, W)) if depth_obs is None else _f32(depth_obs) / np.float64(depth_scale)
    on = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    trace = []
    err_prev = 0.0
    k = 0
    while True:
        with np.errstate(all="ignore"):
            rd = render(verts, faces, R, t, K4, H, W)
            z, n = rd["depth"], rd["normal"]
            seen = rd["cover"] & (d > 0.0)
            gap = np.abs(d - z)
            keep = seen & (gap < max_dist) & on & ((n != 0.0).any(0))
            p = np.stack([z * xn, z * yn, z])
            o = np.stack([d * xn, d * yn, d])
            r = (n[0] * (o[0] - p[0]) + n[1] * (o[1] - p[1])) + n[2] * (o[2] - p[2])
            q = (p - t[:, None, None]) / rho
            J = np.stack([q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0],
                          n[0], n[1], n[2]])
            K = int(keep.sum())
            Jk, rk = J[:, keep], r[keep]
            err = float((rk * rk).sum() / np.float64(K)) if K > 0 else np.inf
            marg = dict(rd["margins"])
            marg["gate"] = np.where(seen, np.abs(gap - max_dist), np.inf)
        step = {"K": K, "err": err, "margins": {m: float(v.min()) for m, v in marg.items()},
                "undecided": int(np.logical_or.reduce([v < rr.MARGIN for v in marg.values()]).sum()),
                "R": R.copy(), "t": t.copy()}
        trace.append(step)
        status = None
        if K < min_pairs:
            status = 2
        else:
            if k >= 1:
                with np.errstate(all="ignore"):
                    step["margins"]["stop"] = float(abs(abs(err_prev - err) / err_prev - tol))
                    if abs(err_prev - err) <= tol * err_prev:
                        status = 0
            if status is None and k == max_iter:
                status = 1
        if status is None:
            with np.errstate(all="ignore"):
                A = Jk @ Jk.T
                g = Jk @ rk
                tr = ((((A[0, 0] + A[1, 1]) + A[2, 2]) + A[3, 3]) + A[4, 4]) + A[5, 5]
                A = A + (damp * tr / 6.0) * np.eye(6)
                xi, piv = cholesky_solve(A, g)
                step["margins"]["pivot"] = float(min(piv) / np.trace(A)) if np.isfinite(piv).all() else -np.inf
                if xi is not None:
                    Rn, tn = rodrigues(xi[:3] / rho) @ R, t + xi[3:]
                    if not (np.isfinite(Rn).all() and np.isfinite(tn).all()):
                        xi = None
            if xi is None:
                status = 3
            else:
                R, t, err_prev = Rn, tn, err
                k += 1
                continue
        with np.errstate(all="ignore"):
            rmse = np.float32(np.sqrt(err))
        Ro, to = (R_in, t_in) if k == 0 else (R.astype(np.float32), t.astype(np.float32))
        return {"R": Ro, "t": to, "R64": R, "t64": t, "passes": k, "pairs": K, "rmse": rmse, "status": status,
                "trace": trace}


def check_conditions(res):
    """No undecided pixel in any pass, and every stop and pivot margin holds raster_ref.MARGIN: no exception."""
    for k, step in enumerate(res["trace"]):
        assert step["undecided"] == 0, (k, step["undecided"], step["margins"])
        for m, v in step["margins"].items():
            assert v >= rr.MARGIN, (k, m, v)


def angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, np.float64).reshape(3, 3) @ np.asarray(Rb, np.float64).reshape(3, 3).T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def scene_args(sc, **over):
    """The refiner's arguments for a bop_ref scene dict: the project's defaults (max_dist = DIST_FRAC x diameter,
    rho = diameter / 2), start = the scene's estimate."""
    a = dict(verts=sc["verts"], faces=sc["faces"], R0=sc["R_est"], t0=sc["t_est"], K4=sc["K4"], depth_obs=sc["depth"],
             depth_scale=br.DEPTH_SCALE, max_dist=DIST_FRAC * sc["diameter"], radius=sc["diameter"] / 2.0)
    a.update(over)
    return a


@functools.lru_cache(maxsize=None)
def reference(name):
    return refine(**scene_args(br.scene(name)))


@functools.lru_cache(maxsize=None)
def mixed_reference(b):
    return refine(**scene_args(br.mixed()[1][b]))
