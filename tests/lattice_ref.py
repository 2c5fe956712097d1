"""Lattice scenes for the render family (krrn_raster_maps_f32, krrn_bop_vsd_f32, krrn_bop_visib_u8,
krrn_pose_score_f32, krrn_pose_refine_depth_f32) and slice-edge cases for krrn_bop_mssd_mspd_f32. Nothing is
restated here: every expected answer comes from raster_ref.render, bop_ref.vsd / mssd_mspd,
bop_scene_ref.visibility, verify_ref.score and depth_refine_ref.refine, unchanged.

The lattice principle (raster_ref's `grid`, extended): K4 = (512, 512, cx, cy) with integer cx, cy, R = I,
vertices at multiples of 8 / 512 with z = 0, t = (., ., z) with z in {0.5, 1, 2}, depth_scale = 1024. Every
projected vertex is an integer pixel, every edge function an integer, every w_k a multiple of 1 / 64 (1 / 16,
1 / 256), the rendered depth exactly z. No number that enters a decision is rounded, so the scenes may sit *on* the
tile edges, the box edges and the thresholds that the generic families keep a margin of 1e-9 away from; they
are not members of those families and check_conditions is not meant for them. Kernel and restatement must agree
bit for bit; tests/test_lattice_host.py asserts the exactness facts and that every case fails if its rule is
broken (the evidence that the GPU cases of tests/test_gpu_render_edges.py can fail)."""
import functools

import numpy as np

import bop_ref as br
import bop_scene_ref as sr
import depth_refine_ref as dr
import raster_ref as rr
import verify_ref as vr

H, W = 40, 56                      # 2.5 x 3.5 tiles: the last tile column is 8 wide, the last tile row 8 high
K4 = np.array([512.0, 512.0, 24.0, 24.0], np.float32)
DEPTH_SCALE = 1024.0
BACKGROUND = 3072.0                # raw: 3 m
PX = (24, 24)                      # the principal point: ray == 1.0, distances equal depths
EYE = np.eye(3)
# pose name: t. At z = 1 the plane covers x 16..48, y 16..32 (column 48 alone in the partial tile column, tile
# column 0 culled at the box edge 16); z = 2: x 20..36, y 20..28; near: x 8..72, y 8..40 cut by the frame; shift:
# x 32..64 cut by the frame
POSES = {"z1": (0.0, 0.0, 1.0), "z2": (0.0, 0.0, 2.0), "near": (0.0, 0.0, 0.5), "shift": (16.0 / 512.0, 0.0, 1.0)}
# pose: (pixels, x0, x1, y0, y1, depth)
COVER = {"z1": (561, 16, 48, 16, 32, 1.0), "z2": (153, 20, 36, 20, 28, 2.0), "near": (1536, 8, 55, 8, 39, 0.5),
         "shift": (408, 32, 55, 16, 32, 1.0)}


def _cells(nx, ny):
    """Two faces per cell of an nx x ny vertex lattice, split along the cell's diagonal (as `grid`)."""
    f = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a = j * nx + i
            f += [(a, a + 1, a + nx + 1), (a, a + nx + 1, a + nx)]
    return np.array(f, np.int32)


@functools.lru_cache(maxsize=None)
def plane():
    """The 5 x 3 vertex plane (16 faces): vertices ((8 i - 8) / 512, (8 j - 8) / 512, 0)."""
    v = np.array([[(8 * i - 8) / 512.0, (8 * j - 8) / 512.0, 0.0] for j in range(3) for i in range(5)], np.float32)
    return v, _cells(5, 3)


def t_of(pose):
    return np.array(POSES[pose], np.float64)


@functools.lru_cache(maxsize=None)
def plane_depth(pose, h=H, w=W):
    """The plane's depth image [h, w] under `pose` (0 where nothing covers)."""
    v, f = plane()
    return br.depth_image(v, f, EYE, t_of(pose), K4, h, w)[0]


def observed(pose="z1", at=None, h=H, w=W):
    """The raw f32 frame: the plane's own depth under `pose` (raw 1024 z) over BACKGROUND; at = a raw value
    for pixel PX (np.float32)."""
    d = plane_depth(pose, h, w)
    obs = np.where(d > 0.0, d * DEPTH_SCALE, BACKGROUND).astype(np.float32)
    if at is not None:
        obs[PX[1], PX[0]] = np.float32(at)
    return obs


def ray_image(h=H, w=W):
    rows, cols = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    xn, yn = (cols - 24.0) / 512.0, (rows - 24.0) / 512.0
    return np.sqrt((xn * xn + yn * yn) + 1.0)


# ------------------------------------------------------------------------------------------------ A: rasteriser

GRID_K4 = np.array([512.0, 512.0, 64.0, 64.0], np.float32)
TIES_F = 640                                               # two and a half face chunks
# where the 32 cell faces sit: both sides of every wave boundary (64) and chunk boundary (256) of the list
TIES_ORIG = (0, 63, 64, 127, 128, 191, 192, 255, 256, 257, 300, 319, 320, 350, 383, 384, 400, 447, 448, 480, 511,
             512, 513, 540, 575, 576, 577, 590, 600, 605, 606, 607)


@functools.lru_cache(maxsize=None)
def ties_spread():
    """`grid`'s 32 cell faces spread over a list of 640: slot TIES_ORIG[k] holds cell face (13 k) mod 32; each has
    a duplicate with the other winding at a later slot (even k: the next free slot; odd k: the far end, 639
    downwards); every other slot holds a valid face 1000 px to the right of the window, which the cull drops.
    A scene dict like raster_ref.scene's, plus orig = the 32 slots."""
    g = rr.scene("grid")
    cells = g["faces"][:32]
    nv = len(g["verts"])
    verts = np.concatenate([g["verts"], g["verts"] + np.float32([1000.0 / 512.0, 0.0, 0.0])])
    faces = np.stack([cells[s % 32] + nv for s in range(TIES_F)]).astype(np.int32)
    used = set(TIES_ORIG)
    far = TIES_F - 1
    for k, s in enumerate(TIES_ORIG):
        c = cells[(13 * k) % 32]
        faces[s] = c
        if k % 2 == 0:
            d = s + 1
            while d in used:
                d += 1
        else:
            d = far
            far -= 1
        assert d > s and d not in used
        used.add(d)
        faces[d] = c[::-1]
    return dict(verts=verts, faces=faces, R=EYE, t=np.array([0.0, 0.0, 1.0]), K4=GRID_K4, rmin=60, cmin=60, S=40,
                region_pts=g["region_pts"], orig=np.array(TIES_ORIG))


def render_scene(sc, faces=None, **over):
    a = dict(sc)
    a.update(over)
    return rr.render(a["verts"], a["faces"] if faces is None else faces, a["R"], a["t"], a["K4"], a["rmin"], a["cmin"],
                     a["S"], a["region_pts"], margins=False)


def face_map_in_order(sc, order):
    """The `face` map a walk would give that visits the list in `order` (strict <: the first visited wins equal
    z), in the list's own indices."""
    order = np.asarray(order)
    face = render_scene(sc, faces=sc["faces"][order])["face"]
    return np.where(face >= 0, order[np.maximum(face, 0)], -1)


def wave_reversed_order(F):
    """Waves 3, 2, 1, 0 inside each chunk of 256."""
    out = []
    for base in range(0, F, 256):
        for w in (3, 2, 1, 0):
            out += [i for i in range(base + 64 * w, base + 64 * w + 64) if i < F]
    return np.array(out)


def chunk_reversed_order(F):
    return np.concatenate([np.arange(b, min(b + 256, F)) for b in range(0, F, 256)][::-1])


@functools.lru_cache(maxsize=None)
def tile_edges():
    """`grid` in a window of S = 49 at 48: the mesh spans local 16..48, its first row / column on tile 1's first
    sample point, its last alone in the 1-pixel partial tiles."""
    return dict(rr.scene("grid"), rmin=48, cmin=48, S=49)


def region_points(nr):
    """NR = 1: one point; NR = 256: 128 distinct lattice points of the plane, then the same 128 again (a region
    index above 128 means a tie went to the higher j)."""
    if nr == 1:
        return np.zeros((1, 3), np.float32)
    p = np.array([[(2 * i - 8) / 512.0, (2 * j - 8) / 512.0, 0.0] for j in range(8) for i in range(16)], np.float32)
    return np.concatenate([p, p])


# S: (rmin, cmin) on the plane at z1 (x 16..48, y 16..32)
SIZE_WINDOWS = {1: (16, 48), 16: (20, 40), 17: (16, 32), 480: (0, 0)}


def size_scene(S, nr):
    v, f = plane()
    rmin, cmin = SIZE_WINDOWS[S]
    return dict(verts=v, faces=f, R=EYE, t=t_of("z1"), K4=K4, rmin=rmin, cmin=cmin, S=S, region_pts=region_points(nr))


@functools.lru_cache(maxsize=None)
def size_reference(S, nr):
    return render_scene(size_scene(S, nr))


# ------------------------------------------------------------------------------------------ B: frame kernels

DELTA, TAUS, DIAMETER, TAU = 0.25, (0.125, 0.25, 0.5), 4.0, 0.25


def vsd(est, gt, depth, delta=DELTA, taus=TAUS):
    v, f = plane()
    return br.vsd(v, f, EYE, t_of(est), EYE, t_of(gt), K4, depth, DEPTH_SCALE, DIAMETER, delta=delta, taus=taus)


def visibility(pose, depth, delta=DELTA):
    v, f = plane()
    return sr.visibility(v, f, EYE, t_of(pose), K4, depth, depth_scale=DEPTH_SCALE, delta=delta)


def score(poses, depth, tau=TAU, mask=None):
    """Candidates `poses` against `depth`; mask default = the z1 silhouette, no box."""
    v, f = plane()
    h, w = depth.shape
    m = (plane_depth("z1", h, w) > 0.0).astype(np.uint8) if mask is None else mask
    return vr.score(v, f, [EYE] * len(poses), [t_of(p) for p in poses], K4, depth, DEPTH_SCALE, tau=tau, mask=m)


# -------------------------------------------------------------------------------------------- C: depth refiner

RAW_OFF = 1032.0                   # (1 + 2^-7) x 1024: the observed surface 2^-7 m behind the plane
GAP = 2.0 ** -7


def refine_frame():
    """Raw 1032 on the 561 pixels the plane covers at z1, 0 elsewhere."""
    return np.where(plane_depth("z1") > 0.0, RAW_OFF, 0.0).astype(np.float32)


# case: the arguments that differ from (max_dist 0.25, radius 1, the module defaults of depth_refine_ref)
REFINE_CASES = {
    "pivot": dict(damp=0.0),
    "radius0_damp0": dict(radius=0.0, damp=0.0),
    "radius0": dict(radius=0.0),
    "gate_equal": dict(max_dist=GAP),
    "gate_above": dict(max_dist=GAP * (1.0 + 2.0 ** -52), max_iter=0),
    "pairs_561": dict(min_pairs=561, max_iter=0),
    "pairs_562": dict(min_pairs=562, max_iter=0),
}
# case: (status, passes, pairs, rmse)
REFINE_EXPECTED = {
    "pivot": ("DEGENERATE", 0, 561, GAP), "radius0_damp0": ("DEGENERATE", 0, 561, GAP),
    "radius0": ("DEGENERATE", 0, 561, GAP), "gate_equal": ("STARVED", 0, 0, np.inf),
    "gate_above": ("MAX_ITER", 0, 561, GAP), "pairs_561": ("MAX_ITER", 0, 561, GAP),
    "pairs_562": ("STARVED", 0, 561, GAP),
}


def refine_args(case=None, **over):
    v, f = plane()
    a = dict(verts=v, faces=f, R0=EYE, t0=t_of("z1"), K4=K4, depth_obs=refine_frame(), depth_scale=DEPTH_SCALE,
             max_dist=0.25, radius=1.0)
    a.update(REFINE_CASES[case] if case else {})
    a.update(over)
    return a


@functools.lru_cache(maxsize=None)
def refine_reference(case):
    return dr.refine(**refine_args(case))


# Generic-scene cases (bop_ref's tetra; test_gpu_depth_refine.py's comparison applies). tol = 0 on tetra is not
# among them: in pass 6 the restatement's relative change of err comes within 4.9e-10 of 0, under the `stop`
# margin of depth_refine_ref.check_conditions, so CONVERGED against MAX_ITER is not decided there.
STARVE_MIN_PAIRS = 125


def starve_mask():
    sc = br.scene("tetra")
    m = np.zeros((sc["H"], sc["W"]), np.uint8)
    m[:, 227:] = 1
    return m


@functools.lru_cache(maxsize=None)
def starve_reference():
    """bop_ref's tetra under a mask that keeps 126 pixels in pass 0 and 124 in pass 1: STARVED after an update."""
    return dr.refine(**dr.scene_args(br.scene("tetra"), mask=starve_mask(), min_pairs=STARVE_MIN_PAIRS))


# ------------------------------------------------------------------------------------------- D: MSSD / MSPD

SYM_SPLIT = 16                     # kBopSymSplit: slices of cdiv(NS, 16) symmetries
# NS: the symmetry the estimate is built from (15, 17, 33: in the last non-empty slice; 16, 32: in slice 0)
MS_TARGET = {15: 14, 16: 0, 17: 16, 32: 1, 33: 32}


def slice_of(s, ns):
    return s // -(-ns // SYM_SPLIT)


def small_syms(ns):
    """ns distinct rotations about the z axis by 0.02 k rad, identity first, as [ns, 12]."""
    S = np.zeros((ns, 12))
    for k in range(ns):
        c, s = np.cos(0.02 * k), np.sin(0.02 * k)
        S[k, :9] = [c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0]
    return S


@functools.lru_cache(maxsize=None)
def ms_mesh(subdiv=2):
    r = {2: 0.04, 3: 0.05}[subdiv]
    return rr.icosphere(subdiv, r)[0].astype(np.float32) * np.float32([1.0, 0.8, 1.2])


def _ms_case(rng, verts, syms, k):
    """The estimate = the GT pose composed with syms[k], then moved by 0.05 degrees / 0.1 mm."""
    R_gt, t_gt = rr.rotation(rng), rr._centre_t(rng.uniform(0.5, 1.0), rng.uniform(100, 500), rng.uniform(100, 400))
    R_est, t_est = br.perturbed(rng, R_gt @ syms[k, :9].reshape(3, 3), R_gt @ syms[k, 9:] + t_gt, deg=0.05, mm=0.1)
    return dict(verts=verts, syms=syms, R_est=R_est, t_est=t_est, R_gt=R_gt, t_gt=t_gt)


@functools.lru_cache(maxsize=None)
def ms_cases():
    """name -> case dict (verts, syms, the two poses). ns15 .. ns33: the slice edges; tie_low / tie_zero: NS = 17
    with a bit-copy of the arg-min symmetry in another slice; v1 / v256 / v257: vertex counts at the 256-thread
    stride, cut out of the 642-vertex mesh."""
    rng = np.random.default_rng(41)
    out = {}
    for ns, k in MS_TARGET.items():
        out[f"ns{ns}"] = _ms_case(rng, ms_mesh(), small_syms(ns), k)
    low = _ms_case(rng, ms_mesh(), small_syms(17), 5)
    low["syms"] = low["syms"].copy()
    low["syms"][16] = low["syms"][5]                          # the copy in the last slice: index 5 must win
    out["tie_low"] = low
    zero = _ms_case(rng, ms_mesh(), small_syms(17), 16)
    zero["syms"] = zero["syms"].copy()
    zero["syms"][0] = zero["syms"][16]                        # the copy at 0, the original at 16: index 0 must win
    out["tie_zero"] = zero
    big = ms_mesh(3)
    for nv, first in ((1, 0), (256, 100), (257, 300)):
        out[f"v{nv}"] = dict(_ms_case(rng, big[first:first + nv], small_syms(3), 2), first=first)
    return out


def ms_reference(c):
    return br.mssd_mspd(c["verts"], c["R_est"], c["t_est"], c["R_gt"], c["t_gt"], rr.LM_K4, c["syms"])
