"""krrn_scene_render_f64, krrn_scene_overlay_u8 and krrn_scene_depth_diff_u8 (include/krrn_hip.h) restated in numpy
(not a test).

The render calls raster_ref.render once per instance over the whole frame (S = max(H, W) at rmin = cmin = 0, cut to
H x W, one dummy region point) and merges the instances with a strict < in instance order, so it culls nothing. To
raster_ref's own per-pixel margins (edge, depth and flip, each the smallest over the instances that bear on the pixel)
it adds
  inst    the relative depth gap between the two nearest instances at the pixel
  shade   how far s + 0.5 is from an integer (the truncation that makes the shade byte)
and a pixel is decided under raster_ref.MARGIN, as there. check_conditions asserts that a generic scene has no
undecided pixel. overlay and depth_diff are integer / f64 restatements and exact."""
import functools

import numpy as np

import raster_ref as rr


def _range(rng, b, total):
    """rast_range: (first, count) of row b, a bad range empty, cut at `total`."""
    first, n = int(rng[b][0]), int(rng[b][1])
    if first < 0 or n < 0 or first > total:
        n = 0
    if first + n > total:
        n = total - first
    return first, n


def render(verts, faces, face_range, R, t, K4, inst_range, H, W, margins=True):
    """N instances over F frames -> {"inst" int64 [F, H, W], "depth" f32, "shade" u8, "z" f64 (the depth before its
    rounding to f32)} and, with `margins`, "margins": {name: f64 [F, H, W]}."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    face_range = np.asarray(face_range, np.int64).reshape(-1, 2)
    inst_range = np.asarray(inst_range, np.int64).reshape(-1, 2)
    N, F = len(face_range), len(inst_range)
    R = np.asarray(R, np.float64).reshape(N, 3, 3)
    t = np.asarray(t, np.float64).reshape(N, 3)
    K4 = np.asarray(K4, np.float32).reshape(N, 4)
    S = max(H, W)
    inst = np.full((F, H, W), -1, np.int64)
    z = np.zeros((F, H, W))
    shade = np.zeros((F, H, W), np.uint8)
    names = ("edge", "depth", "flip", "inst", "shade")
    marg = {k: np.full((F, H, W), np.inf) for k in names}
    for f in range(F):
        n0, cnt = _range(inst_range, f, N)
        best = np.full((H, W), np.inf)
        second = np.full((H, W), np.inf)
        nz = np.zeros((H, W))
        flip = np.full((H, W), np.inf)
        for n in range(n0, n0 + cnt):
            f0, nf = _range(face_range, n, len(faces))
            res = rr.render(verts, faces[f0:f0 + nf], R[n], t[n], K4[n], 0, 0, S, np.zeros((1, 3), np.float32),
                            margins=margins)
            cover, d = res["cover"][:H, :W], res["depth"][:H, :W]
            win = cover & (d < best)
            lose = cover & ~win
            second = np.where(win, best, np.where(lose, np.minimum(second, d), second))
            best = np.where(win, d, best)
            inst[f] = np.where(win, n, inst[f])
            nz = np.where(win, res["normal"][2][:H, :W], nz)
            if margins:
                m = res["margins"]
                marg["edge"][f] = np.minimum(marg["edge"][f], m["edge"][:H, :W])
                marg["depth"][f] = np.minimum(marg["depth"][f], m["depth"][:H, :W])
                flip = np.where(win, m["flip"][:H, :W], flip)
        hit = inst[f] >= 0
        z[f] = np.where(hit, best, 0.0)
        lam = np.minimum(np.maximum(-nz, 0.0), 1.0)
        s = 64.0 + 191.0 * lam
        shade[f] = np.where(hit, (s + 0.5).astype(np.int64), 0).astype(np.uint8)
        if margins:
            two = hit & np.isfinite(second)
            one = np.where(two, best, 1.0)
            marg["inst"][f] = np.where(two, (np.where(two, second, 1.0) - one) / one, np.inf)
            marg["flip"][f] = np.where(hit, flip, np.inf)
            h = s + 0.5
            marg["shade"][f] = np.where(hit, np.minimum(h - np.floor(h), np.floor(h) + 1.0 - h), np.inf)
    out = {"inst": inst, "depth": z.astype(np.float32), "shade": shade, "z": z}
    if margins:
        out["margins"] = marg
    return out


def undecided(res):
    bad = np.zeros(res["inst"].shape, bool)
    for m in res["margins"].values():
        bad |= m < rr.MARGIN
    return bad


def check_conditions(res):
    bad = undecided(res)
    worst = {k: float(v.min()) for k, v in res["margins"].items()}
    assert not bad.any(), (int(bad.sum()), worst, np.argwhere(bad)[:5].tolist())
    assert np.isfinite(res["z"]).all()


def _ids(L, limit):
    L = np.asarray(L, np.int64)
    return L if limit is None else np.where((L < 0) | (L >= limit), -1, L)


def edge(L, radius):
    """edge_L [F, H, W]: L[p] >= 0 and some q with |dx|, |dy| <= radius inside the frame has L[q] != L[p]."""
    F, H, W = L.shape
    out = np.zeros(L.shape, bool)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y1 <= y0 or x1 <= x0:
                continue
            out[:, y0:y1, x0:x1] |= L[:, y0:y1, x0:x1] != L[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out & (L >= 0)


def overlay(rgb, est, shade, tint, alpha=128, radius=1, gt=None, gt_colour=(0, 255, 0)):
    """u8 [F, H, W, 3]; integers throughout (int64 arrays)."""
    c = np.asarray(rgb, np.uint8).astype(np.int64)
    tint = np.asarray(tint, np.int64).reshape(-1, 3)
    N = len(tint)
    e = _ids(est, N)
    on = e >= 0
    tp = np.concatenate([tint, np.zeros((1, 3), np.int64)])[np.where(on, e, N)]   # [F, H, W, 3]; zeros where off
    lit = (tp * np.asarray(shade, np.int64)[..., None] + 127) // 255
    mix = (c * (256 - int(alpha)) + lit * int(alpha) + 128) >> 8
    c = np.where(on[..., None], mix, c)
    c = np.where(edge(e, int(radius))[..., None], tp, c)
    if gt is not None:
        g = edge(_ids(gt, None), int(radius))
        c = np.where(g[..., None], np.asarray(gt_colour, np.int64), c)
    assert c.min() >= 0 and c.max() <= 255
    return c.astype(np.uint8)


def depth_diff(ren, obs, depth_scale=1.0, tol=0.02):
    r = np.asarray(ren, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        o = np.asarray(obs, np.float32).astype(np.float64) / np.float64(depth_scale)
        both = (r > 0.0) & (o > 0.0)
        e = np.where(both, r - o, 0.0)
        k = (np.minimum(np.abs(e) / np.float64(tol), 1.0) * 255.0 + 0.5).astype(np.int64)
    out = np.zeros(r.shape + (3,), np.int64)
    out[(r > 0.0) & ~both] = 128
    white = np.full(r.shape + (3,), 255, np.int64)
    red = white - k[..., None] * np.array([0, 1, 1])
    blue = white - k[..., None] * np.array([1, 1, 0])
    col = np.where((e > 0.0)[..., None], red, np.where((e < 0.0)[..., None], blue, white))
    out = np.where(both[..., None], col, out)
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------------------------- scenes

def concat(meshes):
    """[(verts, faces)] -> (verts f32 [Vtot, 3], faces int32 [Ftot, 3] with global indices, face ranges [(first, n)])."""
    vs, fs, rng, v0, f0 = [], [], [], 0, 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32))
        fs.append(np.asarray(f, np.int32) + v0)
        rng.append((f0, len(f)))
        v0, f0 = v0 + len(v), f0 + len(f)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32), rng


K_SMALL = (120.0, 120.0, 35.5, 19.5)                     # the 40 x 72 frames' camera
H_SMALL, W_SMALL = 40, 72                                # neither a multiple of 16: partial tiles on both sides


def _pack(meshes, use, R, t, K4, inst_range, H, W):
    verts, faces, rng = concat(meshes)
    return dict(verts=verts, faces=faces, face_range=np.array([rng[m] for m in use], np.int32).reshape(-1, 2),
                R=np.asarray(R, np.float64).reshape(-1, 9), t=np.asarray(t, np.float64).reshape(-1, 3),
                K4=np.tile(np.asarray(K4, np.float32), (len(use), 1)), inst_range=np.array(inst_range, np.int32),
                H=H, W=W)


@functools.lru_cache(maxsize=None)
def scene(name):
    """overlap  one 40 x 72 frame: three subdiv-1 spheres that overlap one another, listed out of depth order, one
                instance behind the camera and one that projects off the frame
       ties     two 48 x 64 frames, every tie exact: one sphere twice under one pose; a dyadic grid (raster_ref's `grid`
                construction) three times at depth exactly 1, twice under one pose and once shifted by 8 pixels
       frames   seven inst_range rows over five instances on 40 x 72: counts 2 (one a subdiv-2 sphere: 320 faces, two
                face chunks), 0 and 3, then a negative first, a negative count, a range cut at N, a first past N"""
    rng = np.random.default_rng({"overlap": 11, "ties": 12, "frames": 13}[name])
    ct = lambda z, col, row, K=K_SMALL: rr._centre_t(z, col, row, K4=K)  # noqa: E731
    if name == "overlap":
        meshes = [rr.icosphere(1, 0.1), rr.icosphere(1, 0.08)]
        t = [ct(1.0, 28.3, 18.6), ct(0.9, 38.4, 22.7), ct(1.1, 47.2, 16.4), [0.02, -0.01, -1.0], ct(1.0, 200.5, 20.3)]
        return _pack(meshes, [0, 1, 0, 0, 1], [rr.rotation(rng) for _ in t], t, K_SMALL, [(0, 5)], H_SMALL, W_SMALL)
    if name == "ties":
        n = 5
        gv = np.array([[8 * i / 512.0, 8 * j / 512.0, 0.0] for j in range(n) for i in range(n)])
        gf = []
        for j in range(n - 1):
            for i in range(n - 1):
                a = j * n + i
                gf += [(a, a + 1, a + n + 1), (a, a + n + 1, a + n)]
        K = (512.0, 512.0, 16.0, 8.0)                    # the grid covers pixels 16 .. 48 x 8 .. 40
        Rs = rr.rotation(rng)
        ts = rr._centre_t(0.9, 30.4, 22.7, K4=K)
        R = [Rs, Rs, np.eye(3), np.eye(3), np.eye(3)]
        t = [ts, ts, [8.0 / 512.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]]
        return _pack([rr.icosphere(1, 0.012), (gv, np.array(gf, np.int32))], [0, 0, 1, 1, 1], R, t, K,
                     [(0, 2), (2, 3)], 48, 64)
    if name == "frames":
        meshes = [rr.icosphere(2, 0.09), rr.icosphere(1, 0.07)]
        t = [ct(1.0, 30.6, 17.3), ct(0.85, 41.2, 24.4), ct(0.95, 18.3, 21.7), ct(1.05, 33.4, 15.2), ct(0.8, 52.7, 26.1)]
        rows = [(0, 2), (2, 0), (2, 3), (-1, 2), (3, -1), (4, 5), (7, 1)]
        return _pack(meshes, [0, 1, 1, 0, 1], [rr.rotation(rng) for _ in t], t, K_SMALL, rows, H_SMALL, W_SMALL)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    sc = scene(name)
    return render(sc["verts"], sc["faces"], sc["face_range"], sc["R"], sc["t"], sc["K4"], sc["inst_range"], sc["H"],
                  sc["W"], margins=name != "ties")
