"""The BOP-19 pose errors (krrn_bop_vsd_f32, krrn_bop_mssd_mspd_f32; include/krrn_hip.h) restated in numpy
f64 with the same operation order, on a seeded scene family over raster_ref's meshes, with per-pixel decision
margins. The two depth images of VSD are raster_ref.render's (the rasteriser's restatement, its `edge` margin
included); this file adds the margins of VSD's own decisions:
  vis   |(model - obs) - delta| wherever an observed and a model distance are both > 0 (the visibility test)
  tau   min_k |cost - taus[k]| on the intersection (the step counts)
A pixel is decided when every margin is >= raster_ref.MARGIN = 1e-9; a scene is usable when no pixel is
undecided, so that the kernel's integer counts must equal these exactly (check_conditions). The depth margin of
the rasteriser (which of two faces wins) is not needed: VSD reads the depth, not the face, and a swap between
faces within 1e-9 of each other moves no decision that `vis` and `tau` have not bounded."""
import functools

import numpy as np

import raster_ref as rr

DELTA = 0.015
TAUS = tuple(0.05 * k for k in range(1, 11))
DEPTH_SCALE = 1000.0   # the scenes' observed depth is in millimetres, f32


def depth_image(verts, faces, R, t, K4, H, W):
    """(depth f64 [H, W] with 0 where nothing covers, edge margin [H, W]) over the whole frame."""
    S = max(H, W)
    res = rr.render(verts, faces, R, t, K4, 0, 0, S, np.asarray(verts, np.float32)[:1], margins=True)
    return res["depth"][:H, :W], res["margins"]["edge"][:H, :W]


def _dist(d, ray):
    return np.where(d > 0.0, d * ray, 0.0)


def vsd(verts, faces, R_est, t_est, R_gt, t_gt, K4, depth_obs, depth_scale, diameter, delta=DELTA, taus=TAUS,
        images=None):
    """One crop over the whole frame. depth_obs f32 [H, W] raw units. Returns counts int [2 + T], e_vsd f64
    [T], the masks and the margin maps. images = (D_est, D_gt) replaces the two renders (an independent depth
    source for cross-checks; the edge margins are then not known and reported as inf)."""
    H, W = depth_obs.shape
    fx, fy, cx, cy = (np.float64(np.float32(k)) for k in K4)
    if images is None:
        d_est, edge_e = depth_image(verts, faces, R_est, t_est, K4, H, W)
        d_gt, edge_g = depth_image(verts, faces, R_gt, t_gt, K4, H, W)
    else:
        (d_est, d_gt), edge_e, edge_g = images, np.full((H, W), np.inf), np.full((H, W), np.inf)
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xn, yn = (cols - cx) / fx, (rows - cy) / fy
    ray = np.sqrt((xn * xn + yn * yn) + 1.0)
    with np.errstate(all="ignore"):
        obs = _dist(np.asarray(depth_obs, np.float32).astype(np.float64) / np.float64(depth_scale), ray)
        dist_est, dist_gt = _dist(d_est, ray), _dist(d_gt, ray)

        def visib(model):
            return ((obs > 0.0) & (model > 0.0) & ((model - obs) <= delta)) | ((obs == 0.0) & (model > 0.0))

        v_gt = visib(dist_gt)
        v_est = visib(dist_est) | (v_gt & (dist_est > 0.0))
        inter, union = v_gt & v_est, v_gt | v_est
        cost = np.abs(dist_gt - dist_est) / np.float64(diameter)
        tau = np.asarray(taus, np.float64)
        steps = [int((inter & (cost >= tk)).sum()) for tk in tau]
        un, it = int(union.sum()), int(inter.sum())
        e = np.array([np.float64(s + (un - it)) / np.float64(un) if un > 0 else 1.0 for s in steps])
        vis_m = np.full((H, W), np.inf)
        for model in (dist_est, dist_gt):
            both = (obs > 0.0) & (model > 0.0)
            vis_m = np.where(both, np.minimum(vis_m, np.abs((model - obs) - delta)), vis_m)
        tau_m = np.where(inter, np.abs(cost[..., None] - tau).min(-1), np.inf)
    return {"counts": np.array([un, it] + steps, np.int64), "e_vsd": e, "inter": inter, "union": union, "v_gt": v_gt,
            "d_est": d_est, "d_gt": d_gt,
            "margins": {"edge_est": edge_e, "edge_gt": edge_g, "vis": vis_m, "tau": tau_m}}


def undecided(res):
    bad = np.zeros(res["inter"].shape, bool)
    for m in res["margins"].values():
        bad |= m < rr.MARGIN
    return bad


def check_conditions(res):
    """No undecided pixel: every pixel of the frame takes part in the comparison."""
    bad = undecided(res)
    worst = {k: float(v.min()) for k, v in res["margins"].items()}
    assert not bad.any(), (int(bad.sum()), worst, np.argwhere(bad)[:5].tolist())


def mssd_mspd(verts, R_est, t_est, R_gt, t_gt, K4, syms):
    """One crop: verts f32 [V, 3], syms f64 [NS, 12]. Returns mssd, mspd, their arg-min symmetry indices (the
    lowest on ties; -1 if none is finite) and the per-symmetry maxima (m3 [NS], m2 [NS])."""
    V = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    syms = np.asarray(syms, np.float64).reshape(-1, 12)
    fx, fy, cx, cy = (np.float64(np.float32(k)) for k in K4)
    x, y, z = V[:, 0], V[:, 1], V[:, 2]

    def rigid(M, tv, x, y, z):
        M = np.asarray(M, np.float64).reshape(9)
        tv = np.asarray(tv, np.float64).reshape(3)
        return [((M[3 * k] * x + M[3 * k + 1] * y) + M[3 * k + 2] * z) + tv[k] for k in range(3)]

    m3, m2 = np.zeros(len(syms)), np.zeros(len(syms))
    if len(V) == 0 or len(syms) == 0:
        return np.inf, np.inf, -1, -1, m3, m2
    with np.errstate(all="ignore"):
        e = rigid(R_est, t_est, x, y, z)
        for s, S in enumerate(syms):
            sx, sy, sz = rigid(S[:9], S[9:], x, y, z)
            g = rigid(R_gt, t_gt, sx, sy, sz)
            dx, dy, dz = e[0] - g[0], e[1] - g[1], e[2] - g[2]
            d3 = np.sqrt((dx * dx + dy * dy) + dz * dz)
            du = (fx * e[0] / e[2] + cx) - (fx * g[0] / g[2] + cx)
            dv = (fy * e[1] / e[2] + cy) - (fy * g[1] / g[2] + cy)
            d2 = np.sqrt(du * du + dv * dv)
            m3[s] = np.where(np.isnan(d3), np.inf, d3).max()
            m2[s] = np.where(np.isnan(d2), np.inf, d2).max()
    i3 = int(np.argmin(m3)) if np.isfinite(m3).any() else -1
    i2 = int(np.argmin(m2)) if np.isfinite(m2).any() else -1
    return float(m3.min()), float(m2.min()), i3, i2, m3, m2


# ---------------------------------------------------------------------------------------------- scenes

def perturbed(rng, R, t, deg=3.0, mm=4.0):
    """The pose a few degrees / millimetres away."""
    a = rng.uniform(-1.0, 1.0, 3) * np.deg2rad(deg)
    th = np.linalg.norm(a)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    dR = np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)
    return dR @ np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64) + rng.uniform(-1.0, 1.0, 3) * mm / 1000.0


def diameter_of(verts):
    v = np.asarray(verts, np.float64)
    return float(2.0 * np.linalg.norm(v - v.mean(0), axis=1).max())


def observed(d_gt, rng, occlude=True, holes=True, background=1.5):
    """The observed frame (f32, millimetres) of a GT depth image: the object over a background plane behind it,
    an occluding plane 5 cm in front of the object's right third, and a patch of zeros over its upper left."""
    obs = np.where(d_gt > 0.0, d_gt, background)
    ys, xs = np.nonzero(d_gt > 0.0)
    if len(ys):
        x0, x1, y0, y1 = xs.min(), xs.max(), ys.min(), ys.max()
        if occlude:
            xc = x0 + (2 * (x1 - x0)) // 3
            obs[:, xc:] = np.minimum(obs[:, xc:], d_gt[d_gt > 0.0].min() - 0.05)
        if holes:
            obs[y0:y0 + max(2, (y1 - y0) // 3), x0:x0 + max(2, (x1 - x0) // 3)] = 0.0
    obs[rng.random(obs.shape) < 0.01] = 0.0
    return (obs * DEPTH_SCALE).astype(np.float32)


# name: (raster_ref mesh scene, what it pins)
SCENES = ("tetra", "sphere", "layers", "degenerate", "gross", "empty_obs", "small")
RAYCAST = ("tetra", "layers")      # raster_ref.raycast handles these (everything in front of the camera)


@functools.lru_cache(maxsize=None)
def scene(name):
    """tetra (4 faces), layers (4: occlusion inside the mesh), degenerate (87: faces that must be skipped),
    sphere (1280: five face chunks) on 480 x 640 with a perturbed estimate and the full observed frame;
    gross (80 faces): the estimate projects wholly off the GT silhouette; empty_obs (320): an all-zero observed
    frame; small (320): a 90 x 120 frame (5.6 x 7.5 tiles) with K scaled to match and the object cut by the top
    and right frame borders."""
    rng = np.random.default_rng(500 + SCENES.index(name))
    H, W, K4 = rr.H, rr.W, np.asarray(rr.LM_K4, np.float32)
    if name in ("tetra", "sphere", "layers", "degenerate"):
        sc = rr.scene(name)
        verts, faces, R_gt, t_gt = sc["verts"], sc["faces"], sc["R"], sc["t"]
    elif name == "gross":
        verts, faces = rr.icosphere(1, 0.03)
        R_gt, t_gt = rr.rotation(rng), rr._centre_t(0.8, 200.4, 180.7)
    elif name == "empty_obs":
        verts, faces = rr.icosphere(2, 0.04)
        R_gt, t_gt = rr.rotation(rng), rr._centre_t(0.6, 420.3, 300.6)
    elif name == "small":
        H, W = 90, 120
        K4 = (np.asarray(rr.LM_K4, np.float64) * (W / rr.W)).astype(np.float32)
        verts, faces = rr.icosphere(2, 0.03)
        R_gt, t_gt = rr.rotation(rng), rr._centre_t(0.3, 113.3, 3.7, K4=[float(k) for k in K4])
    else:
        raise KeyError(name)
    verts = np.asarray(verts, np.float32)
    if name == "gross":
        R_est, t_est = rr.rotation(rng), rr._centre_t(0.8, 420.2, 320.9)
    else:
        R_est, t_est = perturbed(rng, R_gt, t_gt)
    d_gt, _ = depth_image(verts, faces, R_gt, t_gt, K4, H, W)
    obs = np.zeros((H, W), np.float32) if name == "empty_obs" else observed(d_gt, rng)
    return dict(verts=verts, faces=np.asarray(faces, np.int32).reshape(-1, 3), R_est=R_est, t_est=t_est,
                R_gt=np.asarray(R_gt, np.float64), t_gt=np.asarray(t_gt, np.float64), K4=K4, H=H, W=W, depth=obs,
                diameter=diameter_of(verts))


def scene_vsd(sc, **over):
    a = dict(sc)
    a.update(over)
    return vsd(a["verts"], a["faces"], a["R_est"], a["t_est"], a["R_gt"], a["t_gt"], a["K4"], a["depth"], DEPTH_SCALE,
               a["diameter"], images=a.get("images"))


@functools.lru_cache(maxsize=None)
def reference(name):
    return scene_vsd(scene(name))


@functools.lru_cache(maxsize=None)
def mixed():
    """raster_ref.mixed_batch's B = 5 crops (one with face count 0) with a perturbed estimate, an observed
    frame and a diameter each: the batch arrays, the per-crop scene dicts, and frames f32 [5, 480, 640]."""
    bt, crops = rr.mixed_batch()
    rng = np.random.default_rng(77)
    out = []
    for b, c in enumerate(crops):
        R_est, t_est = perturbed(rng, c["R"], c["t"])
        d_gt, _ = depth_image(c["verts"], c["faces"], c["R"], c["t"], c["K4"], rr.H, rr.W)
        out.append(dict(verts=c["verts"], faces=c["faces"], R_est=R_est, t_est=t_est, R_gt=c["R"], t_gt=c["t"],
                        K4=c["K4"], H=rr.H, W=rr.W, depth=observed(d_gt, rng, occlude=b % 2 == 0),
                        diameter=0.05 + 0.01 * b))
    return bt, out, np.stack([c["depth"] for c in out])


@functools.lru_cache(maxsize=None)
def mixed_reference(b):
    return scene_vsd(mixed()[1][b])


def sym_tetra():
    """A tetrahedron with a 180-degree symmetry about the z axis (a digonal disphenoid: vertices (a, b, c),
    (-a, -b, c), (d, -e, -c), (-d, e, -c)), and that symmetry as a [2, 12] set (identity first)."""
    v = np.array([[0.021, 0.004, 0.012], [-0.021, -0.004, 0.012], [0.006, -0.017, -0.012], [-0.006, 0.017, -0.012]],
                 np.float32)
    S = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], [-1, 0, 0, 0, -1, 0, 0, 0, 1, 0, 0, 0]], np.float64)
    return v, S
