"""The GT-map rasteriser (krrn_raster_maps_f32, krrn_gt_maps_finish_f32; include/krrn_hip.h) restated in
numpy f64 with the same operation order, a seeded scene family, and per-pixel decision margins.

The kernel and this file evaluate the same IEEE f64 expressions, so they normally agree bit for bit; the
margins say how far every discrete decision is from flipping if they did not. f64 rounding over the few
dozen operations behind a decision is about 1e-14 relative; a pixel is *decided* when every margin is
>= MARGIN = 1e-9:
  edge    the smallest |w_k| over every face whose bounding box, grown by GROW = 1e-6 px, contains the pixel
          (coverage and the bounding-box test itself)
  depth   the relative z gap between the two nearest covering faces
  region  the relative gap of the squared distances to the two nearest region points
  flip    |n . c0| / |c0| of the winning face (which way its normal is turned)
check_conditions asserts that a generic scene has no undecided pixel. The `grid` scene is not generic on
purpose: every one of its ties is exact (all coordinates are small dyadic rationals), so its answers are
known without margins."""
import functools

import numpy as np

NEAR = 1e-3
MARGIN = 1e-9
GROW = 1e-6
LM_K4 = (572.4114, 573.57043, 325.2611, 242.04899)
H, W = 480, 640


def _edge(au, av, bu, bv, pu, pv):
    return (bu - au) * (pv - av) - (bv - av) * (pu - au)


def _camera(R, t, v):
    x, y, z = v
    return ((R[:, 0] * x + R[:, 1] * y) + R[:, 2] * z) + t


def render(verts, faces, R, t, K4, rmin, cmin, S, region_pts, margins=True):
    """One crop. verts f32 [V, 3], faces int [F, 3] (the crop's own range), R [3, 3] / t [3] f64, K4 f32
    (fx, fy, cx, cy), region_pts f32 [NR, 3]. Returns the raw maps in f64 / int (face, depth, coord [3, S, S],
    normal [3, S, S], region, cover) and, with `margins`, the per-pixel margin maps."""
    V = np.asarray(verts, np.float32).astype(np.float64)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    fx, fy, cx, cy = (np.float64(np.float32(k)) for k in K4)
    rp = np.asarray(region_pts, np.float32).astype(np.float64).reshape(-1, 3)
    best = np.full((S, S), np.inf)
    second = np.full((S, S), np.inf)
    face = np.full((S, S), -1, np.int64)
    q = np.zeros((3, S, S))
    edge_m = np.full((S, S), np.inf)
    g = GROW if margins else 0.0
    with np.errstate(all="ignore"):
        for f, idx in enumerate(F):
            if idx.min() < 0 or idx.max() >= len(V):
                continue
            c = [_camera(R, t, V[i]) for i in idx]
            if not all(ck[2] > NEAR for ck in c):
                continue
            u = [fx * ck[0] / ck[2] + cx for ck in c]
            v = [fy * ck[1] / ck[2] + cy for ck in c]
            A = _edge(u[0], v[0], u[1], v[1], u[2], v[2])
            if A == 0.0 or not np.isfinite(A):
                continue
            umin, umax, vmin, vmax = min(u), max(u), min(v), max(v)
            # a generous integer window around the box; the exact comparisons below decide
            x0 = int(np.clip(np.floor(umin - g) - 1 - cmin, 0, S))
            x1 = int(np.clip(np.ceil(umax + g) + 1 - cmin, -1, S - 1))
            y0 = int(np.clip(np.floor(vmin - g) - 1 - rmin, 0, S))
            y1 = int(np.clip(np.ceil(vmax + g) + 1 - rmin, -1, S - 1))
            if x1 < x0 or y1 < y0:
                continue
            pv, pu = np.meshgrid(np.arange(rmin + y0, rmin + y1 + 1, dtype=np.float64),
                                 np.arange(cmin + x0, cmin + x1 + 1, dtype=np.float64), indexing="ij")
            w0 = _edge(u[1], v[1], u[2], v[2], pu, pv) / A
            w1 = _edge(u[2], v[2], u[0], v[0], pu, pv) / A
            w2 = _edge(u[0], v[0], u[1], v[1], pu, pv) / A
            sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
            if margins:
                grown = (pu >= umin - g) & (pu <= umax + g) & (pv >= vmin - g) & (pv <= vmax + g)
                wm = np.minimum(np.minimum(np.abs(w0), np.abs(w1)), np.abs(w2))
                edge_m[sl] = np.where(grown, np.minimum(edge_m[sl], wm), edge_m[sl])
            inbox = (pu >= umin) & (pu <= umax) & (pv >= vmin) & (pv <= vmax)
            cov = inbox & (w0 >= 0.0) & (w1 >= 0.0) & (w2 >= 0.0)
            if not cov.any():
                continue
            q0, q1, q2 = w0 / c[0][2], w1 / c[1][2], w2 / c[2][2]
            z = 1.0 / ((q0 + q1) + q2)
            win = cov & (z < best[sl])
            lose = cov & ~win
            second[sl] = np.where(win, best[sl], np.where(lose, np.minimum(second[sl], z), second[sl]))
            best[sl] = np.where(win, z, best[sl])
            face[sl] = np.where(win, f, face[sl])
            for k, qk in enumerate((q0, q1, q2)):
                q[k][sl] = np.where(win, qk, q[k][sl])
        cover = face >= 0
        depth = np.where(cover, best, 0.0)
        coord = np.zeros((3, S, S))
        normal = np.zeros((3, S, S))
        region = np.zeros((S, S), np.int64)
        flip_m = np.full((S, S), np.inf)
        region_m = np.full((S, S), np.inf)
        ys, xs = np.nonzero(cover)
        if len(ys):
            fw = F[face[ys, xs]]                           # [P, 3] vertex indices of the winners
            p0, p1, p2 = V[fw[:, 0]], V[fw[:, 1]], V[fw[:, 2]]
            qq = q[:, ys, xs]
            m = best[ys, xs][:, None] * ((qq[0][:, None] * p0 + qq[1][:, None] * p1) + qq[2][:, None] * p2)
            coord[:, ys, xs] = m.T
            cam = lambda p: ((p[:, 0:1] * R[:, 0] + p[:, 1:2] * R[:, 1]) + p[:, 2:3] * R[:, 2]) + t  # noqa: E731
            c0, c1, c2 = cam(p0), cam(p1), cam(p2)
            e1, e2 = c1 - c0, c2 - c0
            n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
            ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            ok = (ln > 0.0) & np.isfinite(ln)
            n = np.where(ok[:, None], n / ln[:, None], 0.0)
            d = (n[:, 0] * c0[:, 0] + n[:, 1] * c0[:, 1]) + n[:, 2] * c0[:, 2]
            n = np.where((d > 0.0)[:, None], -n, n)
            normal[:, ys, xs] = n.T
            flip_m[ys, xs] = np.abs(d) / np.sqrt((c0 * c0).sum(1))
            df = m[:, None, :] - rp[None]
            d2 = (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]
            j = np.argmin(d2, 1)                           # the first (lowest) index among equal minima
            region[ys, xs] = j + 1
            if rp.shape[0] > 1:
                srt = np.sort(d2, 1)
                region_m[ys, xs] = (srt[:, 1] - srt[:, 0]) / np.maximum(srt[:, 1], 1e-300)
        two = cover & np.isfinite(second)
        depth_m = np.where(two, (np.where(two, second, 1.0) - np.where(two, best, 1.0)) / np.where(two, best, 1.0), np.inf)
    out = {"face": face, "depth": depth, "coord": coord, "normal": normal, "region": region, "cover": cover}
    if margins:
        out["margins"] = {"edge": edge_m, "depth": depth_m, "region": region_m, "flip": flip_m}
    return out


def undecided(res):
    """Pixels with a margin below MARGIN."""
    bad = np.zeros(res["face"].shape, bool)
    for m in res["margins"].values():
        bad |= m < MARGIN
    return bad


def check_conditions(res):
    bad = undecided(res)
    worst = {k: float(v.min()) for k, v in res["margins"].items()}
    assert not bad.any(), (int(bad.sum()), worst, np.argwhere(bad)[:5].tolist())
    for k in ("depth", "coord", "normal"):
        assert np.isfinite(res[k]).all(), k


def finish(coord, normal, region_raw, face, point_mask, cls, extent, lfborder):
    """krrn_gt_maps_finish_f32 for one crop: coord / normal f32 [3, HW], region_raw / face int [HW], point_mask
    u8 [HW], extent / lfborder f64 [3] -> xyz, normal f32 [3, HW], region i64, mask f32, multi_cls_mask i64,
    mask_obj f32 [HW]."""
    on = np.asarray(point_mask).reshape(-1) != 0
    c = np.asarray(coord, np.float32).astype(np.float64)
    xyz = ((c - np.asarray(lfborder, np.float64)[:, None]) / np.asarray(extent, np.float64)[:, None]).astype(np.float32)
    return {"xyz": np.where(on, xyz, np.float32(0)), "normal": np.where(on, np.asarray(normal, np.float32), np.float32(0)),
            "region": np.where(on, np.asarray(region_raw, np.int64), 0), "mask": on.astype(np.float32),
            "multi_cls_mask": on.astype(np.int64) * (int(cls) + 1),
            "mask_obj": (np.asarray(face) >= 0).astype(np.float32)}


def raycast(verts, faces, R, t, K4, rmin, cmin, S):
    """An independent check of coverage and depth: every pixel's ray against every triangle in 3-D
    (Moeller-Trumbore in the camera frame). (face [S, S] the nearest hit, the lowest index among hits within
    1e-12 of it; depth). Vertices behind the camera are not handled: for scenes in front of it only."""
    V = np.asarray(verts, np.float32).astype(np.float64) @ np.asarray(R, np.float64).reshape(3, 3).T + np.asarray(t)
    fx, fy, cx, cy = (np.float64(np.float32(k)) for k in K4)
    ys, xs = np.mgrid[0:S, 0:S]
    d = np.stack([(cmin + xs - cx) / fx, (rmin + ys - cy) / fy, np.ones((S, S))], -1).reshape(-1, 3)
    best = np.full(len(d), np.inf)
    face = np.full(len(d), -1, np.int64)
    for f, (i0, i1, i2) in enumerate(np.asarray(faces).reshape(-1, 3)):
        a, e1, e2 = V[i0], V[i1] - V[i0], V[i2] - V[i0]
        tvec = -a                                            # the ray origin is the camera centre
        pvec = np.cross(d, e2)
        det = pvec @ e1
        qvec = np.cross(tvec, e1)
        with np.errstate(all="ignore"):
            uu = (pvec @ tvec) / det
            vv = (d @ qvec) / det
            tt = (e2 @ qvec) / det                           # d.z = 1: the ray parameter is the camera depth
        hit = (np.abs(det) > 1e-300) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (tt > 0) & (tt < best - 1e-12)
        best = np.where(hit, tt, best)
        face = np.where(hit, f, face)
    return face.reshape(S, S), np.where(face >= 0, best, 0.0).reshape(S, S)


def sphere_depth_bounds(sc):
    """(depth of the ray's hit on the vertex sphere, on the inscribed sphere, rays that meet the inscribed one)."""
    V = sc["verts"].astype(np.float64)
    r_out = np.linalg.norm(V, axis=1).max()
    tri = V[sc["faces"]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    r_in = np.abs((n * tri[:, 0]).sum(1) / np.linalg.norm(n, axis=1)).min()
    r_lo = np.linalg.norm(V, axis=1).min()
    S = sc["S"]
    fx, fy, cx, cy = (float(k) for k in sc["K4"])
    ys, xs = np.mgrid[0:S, 0:S]
    d = np.stack([(sc["cmin"] + xs - cx) / fx, (sc["rmin"] + ys - cy) / fy, np.ones((S, S))], -1)
    c = sc["t"]

    def hit(r):
        a, b, cc = (d * d).sum(-1), (d * c).sum(-1), c @ c - r * r
        disc = b * b - a * cc
        return np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0))) / a, np.nan), disc > 0

    lo, _ = hit(r_out)
    hi, inner = hit(min(r_in, r_lo))
    return lo, hi, inner


# ---------------------------------------------------------------------------------------------- meshes

def icosphere(subdiv, radius=1.0):
    """(verts f64 [V, 3], faces int32 [20 * 4^subdiv, 3]), outward winding."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.array(a, np.float64) / np.linalg.norm(a) for a in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                w = v[a] + v[b]
                v.append(w / np.linalg.norm(w))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius, np.array(f, np.int32)


def rotation(rng):
    qr = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    return qr * np.sign(np.linalg.det(qr))


def fps_points(verts, n):
    """Farthest point sampling from index 0 (sample_model.py:33-46) in f64: the scenes' region points."""
    P = np.asarray(verts, np.float64)
    n = min(n, len(P))
    sel = [0]
    d = np.linalg.norm(P - P[0], axis=1)
    for _ in range(n - 1):
        sel.append(int(np.argmax(d)))
        d = np.minimum(d, np.linalg.norm(P - P[sel[-1]], axis=1))
    return P[sel].astype(np.float32)


def _centre_t(z, col, row, K4=LM_K4):
    """The translation that projects the model origin to pixel (col, row) at depth z."""
    return np.array([(col - K4[2]) * z / K4[0], (row - K4[3]) * z / K4[1], z])


def _scene(verts, faces, R, t, rmin, cmin, S, K4=LM_K4, nr=64, **extra):
    verts = np.asarray(verts, np.float32)
    return dict(verts=verts, faces=np.asarray(faces, np.int32).reshape(-1, 3), R=np.asarray(R, np.float64),
                t=np.asarray(t, np.float64), K4=np.asarray(K4, np.float32), rmin=int(rmin), cmin=int(cmin), S=int(S),
                region_pts=fps_points(verts, nr), **extra)


SCENES = ("tetra", "sphere", "layers", "grid", "behind", "border", "degenerate")
GENERIC = tuple(s for s in SCENES if s != "grid")
MIXED_B = 5


@functools.lru_cache(maxsize=None)
def scene(name):
    """S, then F, then what it pins: the table in the tests' docstrings."""
    rng = np.random.default_rng({n: 100 + i for i, n in enumerate(SCENES)}[name])
    if name == "tetra":      # S = 40 (2.5 tiles: partial tiles), F = 4
        v = np.array([[0.0, 0.0, -0.02], [0.021, 0.003, 0.011], [-0.013, 0.017, 0.009], [-0.006, -0.019, 0.012]])
        f = [(0, 1, 2), (0, 2, 3), (0, 3, 1), (1, 3, 2)]
        return _scene(v, f, _small_rot(rng), _centre_t(0.9, 229.3, 131.6), 112, 210, 40, nr=4)
    if name == "sphere":     # S = 80, F = 1280: five face chunks
        v, f = icosphere(3, 0.045)
        return _scene(v, f, rotation(rng), _centre_t(0.7, 300.4, 200.7), 161, 260, 80, radius=0.045)
    if name == "layers":     # S = 40: a small near quad over a large far one
        v = np.array([[-0.03, -0.028, 0.1], [0.031, -0.027, 0.1], [0.03, 0.029, 0.1], [-0.029, 0.03, 0.1],
                      [-0.008, -0.007, -0.1], [0.009, -0.006, -0.1], [0.008, 0.0075, -0.1], [-0.0065, 0.008, -0.1]])
        f = [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)]
        return _scene(v, f, _small_rot(rng), _centre_t(1.0, 100.37, 80.21), 60, 80, 40, nr=8)
    if name == "grid":       # S = 40: every projection on a pixel centre, every tie exact
        n = 5                                                # 5 x 5 vertices 8 px apart: pixels 64 .. 96
        v = np.array([[8 * i / 512.0, 8 * j / 512.0, 0.0] for j in range(n) for i in range(n)])
        f = []
        for j in range(n - 1):
            for i in range(n - 1):
                a = j * n + i
                f += [(a, a + 1, a + n + 1), (a, a + n + 1, a + n)]   # the shared edge is the cell's diagonal
        f.append(f[0])                                       # a duplicate at a higher index never wins
        f.append(f[13][::-1])                                # and one with the other winding
        return _scene(v, f, np.eye(3), [0.0, 0.0, 1.0], 60, 60, 40, K4=(512.0, 512.0, 64.0, 64.0), nr=16)
    if name == "behind":     # S = 40: part of the mesh has z <= 1e-3
        v, f = icosphere(1, 0.2)
        return _scene(v, f, rotation(rng), _centre_t(0.15, 330.2, 250.9), 230, 310, 40)
    if name == "border":     # S = 40 at rmin = 0: the object straddles the window and the image edge
        v, f = icosphere(2, 0.03)
        return _scene(v, f, rotation(rng), _centre_t(0.8, 118.6, 4.3), 0, 120, 40)
    if name == "degenerate":  # S = 40: faces that must be skipped, appended to a sound mesh
        v, f = icosphere(1, 0.02)
        nv = len(v)
        line = np.array([[0.0, 0.0, -0.03], [0.004, 0.002, -0.03], [0.008, 0.004, -0.03]])
        v = np.concatenate([v, line])
        junk = [(3, 3, 7), (5, 5, 5), (nv, nv + 1, nv + 2), (0, 1, nv + 3), (0, 1, 10 ** 6), (-1, 2, 3),
                (nv, nv, nv + 1)]
        return _scene(v, np.concatenate([f, np.array(junk, np.int32)]), rotation(rng), _centre_t(0.6, 400.3, 300.8),
                      281, 380, 40, n_sound=len(f))
    raise KeyError(name)


def _small_rot(rng):
    """A rotation a few degrees from identity (keeps hand-placed geometry facing the camera)."""
    a = rng.uniform(-0.06, 0.06, 3)
    Q, U = np.linalg.qr(np.eye(3) + np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]))
    return Q * np.sign(np.diag(U))


@functools.lru_cache(maxsize=None)
def reference(name):
    sc = scene(name)
    return render(sc["verts"], sc["faces"], sc["R"], sc["t"], sc["K4"], sc["rmin"], sc["cmin"], sc["S"],
                  sc["region_pts"])


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """B = 5 crops of S = 40 over one concatenated mesh: different objects, poses and face ranges, crop 3
    with face_count = 0. Returns a dict of batch arrays (verts, faces with global indices, face_range, R, t,
    K4, rc, region_pts [B, 64, 3]) and the per-crop scene dicts."""
    rng = np.random.default_rng(7)
    meshes = [icosphere(1, 0.02), (scene("tetra")["verts"], scene("tetra")["faces"]), icosphere(2, 0.025),
              (scene("layers")["verts"], scene("layers")["faces"])]
    voff = np.cumsum([0] + [len(m[0]) for m in meshes])
    foff = np.cumsum([0] + [len(m[1]) for m in meshes])
    verts = np.concatenate([np.asarray(m[0], np.float32) for m in meshes])
    faces = np.concatenate([np.asarray(m[1], np.int32) + voff[i] for i, m in enumerate(meshes)]).astype(np.int32)
    use = [2, 1, 0, 0, 3]
    crops = []
    for b, mi in enumerate(use):
        z = (0.8, 0.9, 0.7, 0.7, 1.0)[b]
        col, row = 200.3 + 37.7 * b, 150.6 + 21.3 * b
        rmin, cmin = int(row) - 19, int(col) - 21
        R = _small_rot(rng) if mi in (1, 3) else rotation(rng)
        crops.append(dict(verts=verts, faces=faces[foff[mi]:foff[mi + 1]] if b != 3 else faces[:0], R=R,
                          t=_centre_t(z, col, row), K4=np.asarray(LM_K4, np.float32), rmin=rmin, cmin=cmin, S=40,
                          region_pts=fps_points(meshes[mi][0], 64 if len(meshes[mi][0]) >= 64 else len(meshes[mi][0])),
                          face_range=(int(foff[mi]), 0 if b == 3 else int(foff[mi + 1] - foff[mi]))))
    for c in crops:  # one NR per batch: short point sets are filled up with distinct points far from the object
        rp = c["region_pts"]
        far = 10.0 + np.arange(64 - len(rp), dtype=np.float32)[:, None] * np.ones((1, 3), np.float32)
        c["region_pts"] = np.concatenate([rp, far])
    batch = dict(verts=verts, faces=faces, face_range=np.array([c["face_range"] for c in crops], np.int32),
                 R=np.stack([c["R"] for c in crops]).reshape(-1, 9), t=np.stack([c["t"] for c in crops]),
                 K4=np.stack([c["K4"] for c in crops]), rc=np.array([[c["rmin"], c["cmin"]] for c in crops], np.int32),
                 region_pts=np.stack([c["region_pts"] for c in crops]), S=40)
    return batch, crops


@functools.lru_cache(maxsize=None)
def mixed_reference(b):
    c = mixed_batch()[1][b]
    return render(c["verts"], c["faces"], c["R"], c["t"], c["K4"], c["rmin"], c["cmin"], c["S"], c["region_pts"])
