"""Ground-truth visibility (krrn_bop_visib_u8; include/krrn_hip.h) restated in numpy f64 on top of
raster_ref.render and bop_ref, with the same operation order, per-pixel decision margins like bop_ref.vsd's, and
the seeded scene family that tests/bop_tree.py writes out as a BOP tree.

Margins: `edge` (the rasteriser's: coverage) and `vis` = |(dist - obs) - delta| wherever an observed and a model
distance are both > 0. A pixel is decided when both are >= raster_ref.MARGIN; every image of the family has zero
undecided pixels (check_conditions), so the kernel's planes, counts and boxes must equal these exactly.

The family: frames of 64 x 48 (12 tiles), observed depth uint16 with depth_scale 1.0 (image `half`: 0.5, i.e.
raw units of half a millimetre), camera K_TINY (image `other`: K_OTHER), three instances per image:
  stack   front (a sphere), rear (a sphere the front one partly hides in the observed depth), hidden (a tetrahedron
          wholly behind the front sphere: px_count_visib = 0, bbox_visib = -1)
  other   border (a sphere crossing the frame's left and top borders), behind (behind the camera: nothing is drawn),
          plain (a tetrahedron)
  half    border2 (crossing the right border), plain2, norange (an empty face range: exists for the kernel only,
          a BOP tree cannot express it)
The observed depth is bop_ref.observed of the nearest surface over the instances drawn (its hole over the upper
left of the silhouettes, 1 % random zeros and, in image `half` only, its occluding plane, which leaves border2
under min_visib = 0.1), quantised to the image's integer raw units.
`ragged` is a fourth image of 50 x 41 (frames whose rows are cut by the right border and are not 16-byte aligned:
the kernel's per-pixel store path), used by the kernel tests only."""
import functools

import numpy as np

import bop_ref as br
import raster_ref as rr

DELTA = br.DELTA
H, W = 48, 64
K_TINY = tuple(np.float32(k) * np.float32(0.1) for k in rr.LM_K4)
K_OTHER = (61.5, 60.25, 30.75, 25.5)


def bbox(m):
    """BOP's calc_2d_bbox over the set pixels: (x, y, x_max - x_min, y_max - y_min); four -1 without one."""
    ys, xs = np.nonzero(m)
    if not len(ys):
        return [-1, -1, -1, -1]
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]


def visibility(verts, faces, R, t, K4, depth, depth_scale=1.0, delta=DELTA, image=None):
    """One instance over the whole frame. depth f32 [H, W] raw units. Returns mask, mask_visib (bool), info int
    [11], visib_fract, the rendered depth and the margin maps. image = a depth image [H, W] that replaces the
    render (an independent depth source for cross-checks; the edge margin is then reported as inf)."""
    h, w = depth.shape
    fx, fy, cx, cy = (np.float64(np.float32(k)) for k in K4)
    d, edge = br.depth_image(verts, faces, R, t, K4, h, w) if image is None else (image, np.full((h, w), np.inf))
    rows, cols = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    xn, yn = (cols - cx) / fx, (rows - cy) / fy
    ray = np.sqrt((xn * xn + yn * yn) + 1.0)
    with np.errstate(all="ignore"):
        obs = br._dist(np.asarray(depth, np.float32).astype(np.float64) / np.float64(depth_scale), ray)
        dist = br._dist(d, ray)
        mask = d > 0.0
        vis = ((obs > 0.0) & (dist > 0.0) & ((dist - obs) <= delta)) | ((obs == 0.0) & (dist > 0.0))
        both = (obs > 0.0) & (dist > 0.0)
        vis_m = np.where(both, np.abs((dist - obs) - delta), np.inf)
    n_all, n_valid, n_vis = int(mask.sum()), int((mask & (obs > 0.0)).sum()), int(vis.sum())
    fract = float(np.float64(n_vis) / np.float64(n_all)) if n_all > 0 else 0.0
    return {"mask": mask, "mask_visib": vis, "info": np.array([n_all, n_valid, n_vis] + bbox(mask) + bbox(vis), np.int64),
            "visib_fract": fract, "depth": d, "margins": {"edge": edge, "vis": vis_m}}


def undecided(res):
    bad = np.zeros(res["mask"].shape, bool)
    for m in res["margins"].values():
        bad |= m < rr.MARGIN
    return bad


def check_conditions(res):
    bad = undecided(res)
    worst = {k: float(v.min()) for k, v in res["margins"].items()}
    assert not bad.any(), (int(bad.sum()), worst, np.argwhere(bad)[:5].tolist())


# ---------------------------------------------------------------------------------------------- scenes

@functools.lru_cache(maxsize=None)
def meshes():
    """{obj id: (verts f32 [V, 3] metres, faces int32 [F, 3])}: 1 a tetrahedron, 2 / 3 icospheres of subdivision
    1 / 2. The vertices are what a loader reads back from a PLY written in millimetres with 4 decimals."""
    tet = rr.scene("tetra")
    out = {1: (np.asarray(tet["verts"], np.float64) * 4.0, tet["faces"]), 2: rr.icosphere(1, 0.09),
           3: rr.icosphere(2, 0.11)}
    return {o: (ply_round(v), np.asarray(f, np.int32).reshape(-1, 3)) for o, (v, f) in out.items()}


def ply_lines(v):
    return [f"{a:.4f} {b:.4f} {c:.4f}" for a, b, c in np.asarray(v, np.float64) * 1000.0]


def ply_round(v):
    return (np.array([np.float32(ln.split()) for ln in ply_lines(v)], dtype=np.float32) / 1000.0).astype(np.float32)


IMAGES = ("stack", "other", "half")
EXTRA = ("ragged",)
# image: (H, W, K4, depth_scale, seed, bop_ref.observed's occluding plane,
#         [(name, obj, z, col, row, drawn into the observed depth)])
_LAYOUT = {
    "stack": (H, W, K_TINY, 1.0, 11, False,
              [("front", 3, 0.80, 30.3, 22.6, True), ("rear", 2, 1.10, 37.7, 27.2, True),
               ("hidden", 1, 1.20, 29.6, 23.1, True)]),
    "other": (H, W, K_OTHER, 1.0, 12, False,
              [("border", 3, 0.90, 4.4, 5.7, True), ("behind", 2, -0.70, 30.2, 20.3, False),
               ("plain", 1, 0.45, 40.3, 30.8, True)]),
    "half": (H, W, K_TINY, 0.5, 13, True,
             [("border2", 2, 0.75, 60.2, 20.4, True), ("plain2", 3, 1.00, 25.6, 26.3, True),
              ("norange", 1, 0.60, 30.0, 20.0, False)]),
    "ragged": (41, 50, K_TINY, 1.0, 14, False,
               [("a", 3, 0.85, 40.6, 30.3, True), ("b", 2, 0.95, 12.2, 14.8, True), ("c", 1, 0.50, 30.1, 8.4, True)]),
}


@functools.lru_cache(maxsize=None)
def image(name):
    """One image of the family: dict(H, W, K4 f32 [4], depth_scale, raw uint16 [H, W], depth f32 [H, W] metres as
    a loader decodes it, inst = [dict(name, obj, verts, faces (empty for `norange`), R, t)])."""
    h, w, K4, scale, seed, occlude, layout = _LAYOUT[name]
    rng = np.random.default_rng(seed)
    K4 = np.asarray(K4, np.float32)
    inst, nearest = [], np.zeros((h, w))
    for nm, obj, z, col, row, drawn in layout:
        v, f = meshes()[obj]
        R = rr._small_rot(rng) if obj == 1 else rr.rotation(rng)
        t = rr._centre_t(z, col, row, K4=[float(k) for k in K4])
        inst.append(dict(name=nm, obj=obj, verts=v, faces=f[:0] if nm == "norange" else f, R=np.asarray(R, np.float64),
                         t=np.asarray(t, np.float64)))
        if drawn:
            d, _ = br.depth_image(v, f, R, t, K4, h, w)
            nearest = np.where((d > 0.0) & ((nearest == 0.0) | (d < nearest)), d, nearest)
    obs_mm = br.observed(nearest, rng, occlude=occlude).astype(np.float64)            # millimetres
    raw = np.round(obs_mm / scale).astype(np.uint16)
    depth = (raw.astype(np.float64) * scale / 1000.0).astype(np.float32)
    return dict(name=name, H=h, W=w, K4=K4, depth_scale=scale, raw=raw, depth=depth, inst=inst)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement for each instance of image `name` (a list, in instance order)."""
    im = image(name)
    return [visibility(i["verts"], i["faces"], i["R"], i["t"], im["K4"], im["depth"]) for i in im["inst"]]


def concat_meshes():
    """(verts f32 [Vtot, 3], faces int32 [Ftot, 3] global indices, {obj: (first face, count)})."""
    vs, fs, rng, v0, f0 = [], [], {}, 0, 0
    for obj, (v, f) in sorted(meshes().items()):
        vs.append(v)
        fs.append(f + v0)
        rng[obj] = (f0, len(f))
        v0, f0 = v0 + len(v), f0 + len(f)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32), rng
