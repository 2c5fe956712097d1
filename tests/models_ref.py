"""numpy restatement of krrn_model_extent_f64 and krrn_symmetry_residual_f64 (include/krrn_hip.h), operation for
operation in f64: every product and sum below is one numpy operation, so one rounding, in the header's order. max and
min do not depend on order, so the vectorised folds give the kernels' bits."""
import numpy as np


def _range(r, total, bound=None):
    """The kernels' guard: (first, count), or (0, 0) for a negative range, a count above the caller's bound or a range
    reaching past `total`."""
    first, n = int(r[0]), int(r[1])
    ok = first >= 0 and n >= 0 and first + n <= total and (bound is None or n <= bound)
    return (first, n) if ok else (0, 0)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def extent_one(v):
    """(d2, box f64 [6]) of one object's vertices f32 [V, 3]: the > walk from 0.0 over all pairs (a NaN term never
    wins), the < / > walks from +inf / -inf per axis."""
    x = np.asarray(v, np.float32).reshape(-1, 3).astype(np.float64)
    box = np.array([np.inf] * 3 + [-np.inf] * 3)
    for k in range(3):
        c = x[:, k][~np.isnan(x[:, k])]
        if len(c):
            box[k], box[3 + k] = c.min(), c.max()
    d2 = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(0, len(x), 256):                       # row blocks keep the [rows, V] arrays small
            dx = x[i:i + 256, None, 0] - x[None, :, 0]
            dy = x[i:i + 256, None, 1] - x[None, :, 1]
            dz = x[i:i + 256, None, 2] - x[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            win = d[d > d2]
            if win.size:
                d2 = float(win.max())
    return d2, box


def extent(verts, vert_range, max_v=None):
    """(d2 f64 [O], box f64 [O, 6]) of a batch, ranges guarded as the kernels guard them."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    out = [extent_one(verts[f:f + n]) for f, n in (_range(r, len(verts), max_v) for r in np.asarray(vert_range).reshape(-1, 2))]
    return np.array([o[0] for o in out]), np.stack([o[1] for o in out])


def tri_dist2(p, a, b, c):
    """The squared distance from p to the triangle (a, b, c), all f64 [..., 3] (broadcast): the closest point by the
    header's region tests, the first that holds deciding. Every case is evaluated everywhere and the deciding one is
    selected, which leaves the selected elements' bits as a scalar walk computes them."""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(t, np.float64) for t in (p, a, b, c)))
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        den = 1.0 / ((va + vb) + vc)
        v, w = vb * den, vc * den
        q = (a + ab * v[..., None]) + ac * w[..., None]                                     # the face's interior
        order = [  # lowest priority first, so that the first test of the header that holds is applied last
            ((va <= 0) & (e43 >= 0) & (e56 >= 0), b + (e43 / (e43 + e56))[..., None] * (c - b)),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[..., None] * ac),
            ((d6 >= 0) & (d5 <= d6), c),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[..., None] * ab),
            ((d3 >= 0) & (d4 <= d3), b),
            ((d1 <= 0) & (d2 <= 0), a),
        ]
        for test, point in order:
            q = np.where(test[..., None], point, q)
        d = p - q
        return _dot(d, d)


def residual_one(verts, faces, v_range, f_range, S):
    """res2 of one symmetry S f64 [12] of the object with vertices verts[v0 : v0 + nv] and faces faces[f0 : f0 + nf]
    (indices into verts; a face with an index outside it is skipped). Ranges already guarded."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    (v0, nv), (f0, nf) = v_range, f_range
    if nv == 0:
        return 0.0
    if nf == 0:
        return np.inf
    S = np.asarray(S, np.float64).reshape(12)
    x = verts[v0:v0 + nv].astype(np.float64)
    with np.errstate(all="ignore"):
        p = np.stack([((S[3 * r] * x[:, 0] + S[3 * r + 1] * x[:, 1]) + S[3 * r + 2] * x[:, 2]) + S[9 + r]
                      for r in range(3)], axis=1)
    tri = faces[f0:f0 + nf]
    ok = ((tri >= 0) & (tri < len(verts))).all(1)
    tri = tri[ok]
    worst = 0.0
    corners = verts.astype(np.float64)[tri] if len(tri) else np.zeros((0, 3, 3))
    for i in range(0, nv, 128):
        if len(tri):
            d = tri_dist2(p[i:i + 128, None, :], corners[None, :, 0], corners[None, :, 1], corners[None, :, 2])
            near = np.fmin.reduce(d, axis=1, initial=np.inf)      # the < walk from +inf: a NaN never wins
        else:
            near = np.full(len(p[i:i + 128]), np.inf)
        worst = max(worst, float(near.max()))                     # never NaN: finite or +inf
    return worst


def residual(verts, faces, vert_range, face_range, syms, sym_range, max_v=None, max_f=None):
    """res2 f64 [NStot] of a batch; a symmetry that no object owns stays NaN (the wrapper's fill)."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    syms = np.asarray(syms, np.float64).reshape(-1, 12)
    out = np.full(len(syms), np.nan)
    O = len(np.asarray(vert_range).reshape(-1, 2))
    for o in reversed(range(O)):                                  # the lowest object wins a shared symmetry
        vr = _range(np.asarray(vert_range).reshape(-1, 2)[o], len(verts), max_v)
        fr = _range(np.asarray(face_range).reshape(-1, 2)[o], len(faces), max_f)
        s0, ns = _range(np.asarray(sym_range).reshape(-1, 2)[o], len(syms))
        for s in range(s0, s0 + ns):
            out[s] = residual_one(verts, faces, vr, fr, syms[s])
    return out
