"""The pose-candidate score (krrn_pose_score_f32; include/krrn_hip.h) restated in numpy f64 with the same
operation order, on bop_ref's scene family, with per-pixel decision margins. The renders are raster_ref.render's
(through bop_ref.depth_image, its `edge` margin included), the observed distance and the ray are bop_ref's; this
file adds the margin of the score's own decisions:
  tol   min(|diff - tau|, |diff + tau|) wherever a model and an observed distance are both > 0 (claim and inter)
A pixel is decided when every margin is >= raster_ref.MARGIN = 1e-9; a case is usable when no pixel is undecided,
so that the kernel's integer counts must equal these exactly (check_conditions). As for VSD, the rasteriser's
depth margin is not needed: the score reads the depth, not the face.

The scenes' candidate sets, masks and boxes (scene_case) are seeded; the seeds were picked on the CPU so that
every case below passes check_conditions with this file alone."""
import functools

import numpy as np

import bop_ref as br
import raster_ref as rr

TAU = 0.015
COUNTS = ("render", "claim", "evid", "both", "inter", "union")
SCENES = ("tetra", "layers", "degenerate", "small", "empty_obs", "gross")
SEEDS = {"tetra": 900, "layers": 901, "degenerate": 902, "small": 903, "empty_obs": 904, "gross": 905}


def score(verts, faces, Rs, ts, K4, depth_obs, depth_scale, tau=TAU, mask=None, box=None):
    """One crop, C candidates, over the whole frame. depth_obs f32 [H, W] raw units (None: a frame index outside
    [0, F), nothing observed; then H, W come from `mask`, which must be given); mask [H, W] (any non-zero is set)
    or None; box (rmin, rmax, cmin, cmax) or None. Returns counts int [C, 6], score f64 [C], best, the per-candidate
    model distances and the margin maps."""
    H, W = (depth_obs if depth_obs is not None else mask).shape
    fx, fy, cx, cy = (np.float64(np.float32(k)) for k in K4)
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xn, yn = (cols - cx) / fx, (rows - cy) / fy
    ray = np.sqrt((xn * xn + yn * yn) + 1.0)
    tau = np.float64(tau)
    counts, scores, dists = [], [], []
    margins = {"tol": np.full((H, W), np.inf)}
    with np.errstate(all="ignore"):
        if depth_obs is None:
            obs = np.zeros((H, W))
        else:
            obs = br._dist(np.asarray(depth_obs, np.float32).astype(np.float64) / np.float64(depth_scale), ray)
        evid = np.zeros((H, W), bool)
        if mask is not None:
            r0, r1, c0, c1 = (0, H, 0, W) if box is None else (max(int(box[0]), 0), min(int(box[1]), H),
                                                                max(int(box[2]), 0), min(int(box[3]), W))
            inbox = (rows >= r0) & (rows < r1) & (cols >= c0) & (cols < c1)
            evid = (np.asarray(mask) != 0) & (obs > 0.0) & inbox
        for c, (R, t) in enumerate(zip(Rs, ts)):
            d, edge = br.depth_image(verts, faces, R, t, K4, H, W)
            m = br._dist(d, ray)
            pair = (m > 0.0) & (obs > 0.0)
            diff = m - obs
            claim = pair & ~(diff > tau)
            both = claim & evid
            inter = both & (np.abs(diff) <= tau)
            n = [int((m > 0.0).sum()), int(claim.sum()), int(evid.sum()), int(both.sum()), int(inter.sum())]
            un = n[1] + n[2] - n[3]
            counts.append(n + [un])
            scores.append(np.float64(n[4]) / np.float64(un) if un > 0 else np.float64(0.0))
            dists.append(m)
            margins[f"edge_{c}"] = edge
            tol = np.minimum(np.abs(diff - tau), np.abs(diff + tau))
            margins["tol"] = np.where(pair, np.minimum(margins["tol"], tol), margins["tol"])
    best, top = 0, 0.0
    for c, s in enumerate(scores):
        if s > top:
            best, top = c, s
    return {"counts": np.array(counts, np.int64).reshape(-1, 6), "score": np.array(scores, np.float64), "best": best,
            "dist": dists, "evid": evid, "margins": margins}


def undecided(res):
    bad = np.zeros(res["evid"].shape, bool)
    for m in res["margins"].values():
        bad |= m < rr.MARGIN
    return bad


def check_conditions(res):
    """No undecided pixel (cap: zero), which licenses the exact comparison of the counts."""
    bad = undecided(res)
    worst = {k: float(v.min()) for k, v in res["margins"].items()}
    assert not bad.any(), (int(bad.sum()), worst, np.argwhere(bad)[:5].tolist())


def silhouette(sc, R=None, t=None):
    """The mesh's coverage under (R, t) (default: the scene's GT pose), bool [H, W]."""
    d, _ = br.depth_image(sc["verts"], sc["faces"], sc["R_gt"] if R is None else R, sc["t_gt"] if t is None else t,
                          sc["K4"], sc["H"], sc["W"])
    return d > 0.0


def shifted_mask(sil):
    """An imperfect detector mask: the silhouette moved one pixel right and down, u8 of 0 / 255."""
    m = np.zeros(sil.shape, np.uint8)
    m[1:, 1:] = sil[:-1, :-1] * np.uint8(255)
    return m


def square_box(mask, H, W, pad=4):
    """(rmin, rmax, cmin, cmax) of a square around the mask's pixels, `pad` wider, not clipped to the frame (the
    kernel clips); a 32-pixel square at the frame's centre for an empty mask."""
    ys, xs = np.nonzero(mask)
    if not len(ys):
        return np.array([H // 2 - 16, H // 2 + 16, W // 2 - 16, W // 2 + 16], np.int32)
    cy, cx = (int(ys.min()) + int(ys.max()) + 1) // 2, (int(xs.min()) + int(xs.max()) + 1) // 2
    half = max(int(ys.max()) - int(ys.min()), int(xs.max()) - int(xs.min())) // 2 + 1 + pad
    return np.array([cy - half, cy + half, cx - half, cx + half], np.int32)


@functools.lru_cache(maxsize=None)
def scene_case(name):
    """The parity case of bop_ref.scene(name): C = 3 candidates (the scene's estimate, its GT pose, a coarser
    perturbation of 8 degrees / 15 mm), mask = the GT silhouette shifted one pixel, box = a square around it."""
    sc = br.scene(name)
    rng = np.random.default_rng(SEEDS[name])
    Rc, tc = br.perturbed(rng, sc["R_gt"], sc["t_gt"], deg=8, mm=15)
    Rs = np.stack([np.asarray(sc["R_est"], np.float64).reshape(3, 3), sc["R_gt"].reshape(3, 3), Rc])
    ts = np.stack([np.asarray(sc["t_est"], np.float64), sc["t_gt"], tc])
    mask = shifted_mask(silhouette(sc))
    return dict(sc, Rs=Rs, ts=ts, mask=mask, box=square_box(mask, sc["H"], sc["W"]))


def case_score(case, **over):
    a = dict(case)
    a.update(over)
    return score(a["verts"], a["faces"], a["Rs"], a["ts"], a["K4"], a["depth"], br.DEPTH_SCALE, a.get("tau", TAU),
                 a["mask"], a["box"])


@functools.lru_cache(maxsize=None)
def reference(name):
    return case_score(scene_case(name))


@functools.lru_cache(maxsize=None)
def mixed():
    """bop_ref.mixed()'s B = 5 batch with C = 2 candidates per crop (the estimate, the GT pose), each crop's mask
    (its GT silhouette shifted one pixel; all zero for the crop with no faces) and box: the batch arrays, the
    per-crop case dicts, the depth frames f32 [5, H, W] and the mask frames u8 [5, H, W]."""
    bt, crops, frames = br.mixed()
    cases = []
    for c in crops:
        mask = shifted_mask(silhouette(c))
        cases.append(dict(c, Rs=np.stack([np.asarray(c["R_est"], np.float64).reshape(3, 3), np.asarray(c["R_gt"]).reshape(3, 3)]),
                          ts=np.stack([np.asarray(c["t_est"], np.float64), np.asarray(c["t_gt"], np.float64)]),
                          mask=mask, box=square_box(mask, c["H"], c["W"])))
    return bt, cases, frames, np.stack([c["mask"] for c in cases])


@functools.lru_cache(maxsize=None)
def mixed_reference(b):
    return case_score(mixed()[1][b])
