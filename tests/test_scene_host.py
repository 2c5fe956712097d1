"""The scene entry points and what sits on them, without a GPU: the ABI signatures and every host-side argument check
of krrn_scene_render_ws / krrn_scene_render_f64 / krrn_scene_overlay_u8 / krrn_scene_depth_diff_u8 (made before any HIP
call, so the pointers are never dereferenced), tests/scene_ref.py against per-pixel Python loops on hand cases, the
refusals of scene.*, bop_scene.vis_results and evaluate.test_epoch(vis_dir=...) that come before a device is touched,
and the keyword's default."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import scene_ref as sf
from pose_estimation_amd import _lib, bop_scene, scene

EARG, ESHAPE = -1, -2
N0 = ctypes.c_void_p(0)
P, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
RENDER = ("verts", "faces", "face_range", "R", "t", "K4", "inst_range", "ws", "inst", "depth", "shade")
OVERLAY = ("rgb", "est", "shade", "tint", "gt", "out")
DIFF = ("ren", "obs", "out")


def _fake(names):
    return {k: ctypes.c_void_p((i + 1) << 40) for i, k in enumerate(names)}   # far apart, never dereferenced


def _render(Vtot=10, Ftot=12, N=3, F=2, H=40, W=72, **over):
    p = dict(_fake(RENDER), **over)
    return _lib.lib().krrn_scene_render_f64(p["verts"], Vtot, p["faces"], Ftot, p["face_range"], p["R"], p["t"], p["K4"],
                                            p["inst_range"], N, F, H, W, p["ws"], p["inst"], p["depth"], p["shade"], N0)


def _overlay(N=3, alpha=128, radius=1, col=(0, 255, 0), F=2, H=40, W=72, **over):
    p = dict(_fake(OVERLAY), **over)
    return _lib.lib().krrn_scene_overlay_u8(p["rgb"], p["est"], p["shade"], p["tint"], N, alpha, radius, p["gt"], col[0],
                                            col[1], col[2], F, H, W, p["out"], N0)


def _diff(depth_scale=1.0, tol=0.02, F=2, H=40, W=72, **over):
    p = dict(_fake(DIFF), **over)
    return _lib.lib().krrn_scene_depth_diff_u8(p["ren"], p["obs"], depth_scale, tol, F, H, W, p["out"], N0)


FRAMES = [dict(F=0), dict(F=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-1), dict(H=65536, W=32768),
          dict(H=46341, W=46341)]


def test_abi_lists_the_entry_points():
    s = _lib.SIGNATURES
    assert s["krrn_scene_render_ws"] == [I, P]
    assert s["krrn_scene_render_f64"] == [P, I, P, I, P, P, P, P, P, I, I, I, I, P, P, P, P, P]
    assert s["krrn_scene_overlay_u8"] == [P, P, P, P, I, I, I, P, I, I, I, I, I, I, P, P]
    assert s["krrn_scene_depth_diff_u8"] == [P, P, D, D, I, I, I, P, P]


def test_render_ws():
    lib = _lib.lib()
    n = ctypes.c_longlong(-7)
    assert lib.krrn_scene_render_ws(5, N0) == EARG and lib.krrn_scene_render_ws(-1, N0) == EARG
    assert lib.krrn_scene_render_ws(-1, ctypes.byref(n)) == ESHAPE and n.value == -7
    assert lib.krrn_scene_render_ws(0, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.krrn_scene_render_ws(5, ctypes.byref(n)) == 0 and n.value == 20
    assert lib.krrn_scene_render_ws(0x7fffffff, ctypes.byref(n)) == 0 and n.value == 4 * 0x7fffffff


@pytest.mark.parametrize("name", RENDER)
def test_render_null_pointer_is_earg(name):
    assert _render(**{name: N0}) == EARG
    assert _render(N=-1, **{name: N0}) == EARG and _render(H=0, **{name: N0}) == EARG    # pointers are checked first
    assert _render(N=0, **{name: N0}) == EARG


@pytest.mark.parametrize("bad", FRAMES + [dict(N=-1), dict(Vtot=0), dict(Vtot=-2), dict(Ftot=-1)])
def test_render_bad_shape_is_eshape(bad):
    assert _render(**bad) == ESHAPE
    assert _render(**dict(dict(inst=ctypes.c_void_p(1 << 40)), **bad)) == ESHAPE         # shapes before overlaps


def test_render_overlap_is_earg():
    px = 2 * 40 * 72
    at = lambda k, off=0: ctypes.c_void_p(((RENDER.index(k) + 1) << 40) + off)  # noqa: E731
    for k, size in (("verts", 120), ("faces", 144), ("face_range", 24), ("R", 216), ("t", 72), ("K4", 48),
                    ("inst_range", 16)):
        for out in ("ws", "inst", "depth", "shade"):
            assert _render(**{out: at(k)}) == EARG, (k, out)
            assert _render(**{out: at(k, size - 1)}) == EARG, (k, out)                   # the input's last byte
    # two outputs over one another: each plane's extent
    assert _render(depth=at("inst", 4 * px - 1)) == EARG
    assert _render(shade=at("depth", 4 * px - 1)) == EARG
    assert _render(inst=at("shade", px - 1)) == EARG
    assert _render(inst=at("ws", 47)) == EARG
    assert _render(ws=at("verts", -1)) == EARG                                           # ws reaches into verts
    # F H W up to 2^62 elements: the extents saturate instead of wrapping
    assert _render(F=0x7fffffff, H=32768, W=65535, inst=at("depth", 1 << 20)) == EARG


def test_render_host_checks_pass_the_legal_edge():
    """What the shape checks must let through is seen with an overlap behind it: a shape error would come first, and
    nothing is launched."""
    over = dict(depth=ctypes.c_void_p(((RENDER.index("inst") + 1) << 40) + 1))
    assert _render(N=0, Ftot=0, F=1, H=1, W=1, **over) == EARG
    assert _render(H=32768, W=65535, **over) == EARG                                     # H W = 2^31 - 32768 fits


@pytest.mark.parametrize("name", [k for k in OVERLAY if k != "gt"])
def test_overlay_null_pointer_is_earg(name):
    assert _overlay(**{name: N0}) == EARG
    assert _overlay(alpha=300, **{name: N0}) == EARG and _overlay(gt=N0, **{name: N0}) == EARG


@pytest.mark.parametrize("bad", FRAMES + [dict(N=-1), dict(alpha=-1), dict(alpha=257), dict(radius=0), dict(radius=5),
                                          dict(radius=-1), dict(col=(-1, 0, 0)), dict(col=(0, 256, 0)),
                                          dict(col=(0, 0, 1000))])
def test_overlay_bad_shape_is_eshape(bad):
    assert _overlay(**bad) == ESHAPE
    assert _overlay(gt=N0, **bad) == ESHAPE
    assert _overlay(**dict(dict(out=ctypes.c_void_p(1 << 40)), **bad)) == ESHAPE


def test_overlay_overlap_is_earg():
    px = 2 * 40 * 72
    at = lambda k, off=0: ctypes.c_void_p(((OVERLAY.index(k) + 1) << 40) + off)  # noqa: E731
    for k, size in (("rgb", 3 * px), ("est", 4 * px), ("shade", px), ("tint", 9), ("gt", 4 * px)):
        assert _overlay(out=at(k)) == EARG and _overlay(out=at(k, size - 1)) == EARG, k
        assert _overlay(out=at(k, -1)) == EARG, k
    assert _overlay(out=at("rgb"), gt=N0) == EARG


@pytest.mark.parametrize("name", DIFF)
def test_depth_diff_null_pointer_is_earg(name):
    assert _diff(**{name: N0}) == EARG and _diff(tol=0.0, **{name: N0}) == EARG


@pytest.mark.parametrize("bad", FRAMES + [dict(tol=0.0), dict(tol=-0.02), dict(tol=float("inf")), dict(tol=float("nan")),
                                          dict(depth_scale=0.0), dict(depth_scale=-0.0)])
def test_depth_diff_bad_shape_is_eshape(bad):
    assert _diff(**bad) == ESHAPE
    assert _diff(**dict(dict(out=ctypes.c_void_p(1 << 40)), **bad)) == ESHAPE


def test_depth_diff_overlap_is_earg():
    px = 2 * 40 * 72
    for k in ("ren", "obs"):
        base = (DIFF.index(k) + 1) << 40
        for off in (0, 4 * px - 1, -1, -(3 * px - 1)):
            assert _diff(out=ctypes.c_void_p(base + off)) == EARG, (k, off)


# ------------------------------------------------------------------------------------- scene_ref against pixel loops

K = (64.0, 64.0, 0.0, 0.0)


def _quad(x0, x1, y0, y1, z):
    """(verts, faces) of the axis-aligned quad whose corners project to pixels (x0 .. x1, y0 .. y1) at depth z under
    K, the identity rotation and no translation. Dyadic: every edge function and depth is exact."""
    c = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return np.array([[u * z / 64.0, v * z / 64.0, z] for u, v in c]), np.array([(0, 1, 2), (0, 2, 3)], np.int32)


def _rect_loop(rects, inst_range, H, W):
    """A z-buffer over axis-aligned rectangles (x0, x1, y0, y1, z), inclusive, one pixel at a time."""
    F = len(inst_range)
    inst, depth = np.full((F, H, W), -1, np.int64), np.zeros((F, H, W), np.float32)
    shade = np.zeros((F, H, W), np.uint8)
    for f, (n0, cnt) in enumerate(inst_range):
        for y in range(H):
            for x in range(W):
                best = math.inf
                for n in range(n0, n0 + cnt):
                    x0, x1, y0, y1, z = rects[n]
                    if x0 <= x <= x1 and y0 <= y <= y1 and z < best:
                        best = z
                        inst[f, y, x], depth[f, y, x], shade[f, y, x] = n, np.float32(z), 255   # facing the camera
    return inst, depth, shade


def _ref_rects(rects, inst_range, H, W):
    v, f, rng = sf.concat([_quad(*r) for r in rects])
    n = len(rects)
    return sf.render(v, f, rng, np.tile(np.eye(3).reshape(1, 9), (n, 1)), np.zeros((n, 3)), np.tile(K, (n, 1)), inst_range,
                     H, W, margins=False)


def test_render_ref_two_quads_and_a_tie():
    H, W = 12, 20
    # a near small quad over a far large one, listed far first and (frame 1) near first; frame 2: one quad twice
    rects = [(2, 14, 1, 9, 2.0), (6, 10, 3, 6, 1.0), (6, 10, 3, 6, 1.0), (2, 14, 1, 9, 2.0), (4, 8, 2, 5, 0.5),
             (4, 8, 2, 5, 0.5)]
    rows = [(0, 2), (2, 2), (4, 2)]
    got = _ref_rects(rects, rows, H, W)
    inst, depth, shade = _rect_loop(rects, rows, H, W)
    assert np.array_equal(got["inst"], inst) and np.array_equal(got["shade"], shade)
    assert got["depth"].tobytes() == depth.tobytes()
    assert set(np.unique(got["inst"][0])) == {-1, 0, 1} and (got["inst"][0][3:7, 6:11] == 1).all()
    assert (got["inst"][1][3:7, 6:11] == 2).all() and (got["inst"][1][1, 2:15] == 3).all()
    assert set(np.unique(got["inst"][2])) == {-1, 4}                                     # an exact tie: the lower index
    assert int((got["inst"][2] == 4).sum()) == 5 * 4
    # bad ranges are empty or cut; nothing past N is drawn
    odd = _ref_rects(rects, [(-1, 2), (3, -1), (5, 9), (7, 1), (6, 0)], H, W)
    assert [sorted(np.unique(p).tolist()) for p in odd["inst"]] == [[-1], [-1], [-1, 5], [-1], [-1]]


def test_render_ref_shade_and_empty():
    # a tilted triangle: the flat normal's z gives the shade; nothing behind the camera
    v = np.array([[-0.2, -0.2, 1.0], [0.3, -0.2, 1.5], [-0.2, 0.3, 1.0]])
    f = np.array([(0, 1, 2)], np.int32)
    Kc = (32.0, 32.0, 8.0, 8.0)
    got = sf.render(v, f, [(0, 1), (0, 1)], np.tile(np.eye(3).reshape(1, 9), (2, 1)), [[0, 0, 0], [0, 0, -3.0]], [Kc, Kc],
                    [(0, 2)], 16, 16, margins=False)
    e1, e2 = v[1] - v[0], v[2] - v[0]
    n = np.cross(e1, e2)
    n = n / np.linalg.norm(n)
    n = -n if n @ v[0] > 0 else n
    want = int(64.0 + 191.0 * min(max(-n[2], 0.0), 1.0) + 0.5)
    assert set(np.unique(got["shade"])) == {0, want} and 64 < want < 255
    assert set(np.unique(got["inst"])) == {-1, 0}
    assert ((got["shade"] > 0) == (got["inst"] >= 0)).all() and ((got["depth"] > 0) == (got["inst"] >= 0)).all()


def _overlay_loop(rgb, est, shade, tint, alpha, radius, gt, col):
    F, H, W = est.shape
    N = len(tint)
    out = np.zeros((F, H, W, 3), np.uint8)

    def ident(Lp, v, bound):
        v = int(v)
        return -1 if bound and not 0 <= v < N else v

    def is_edge(Lp, f, y, x, bound):
        c = ident(Lp, Lp[f, y, x], bound)
        if c < 0:
            return False
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W and ident(Lp, Lp[f, yy, xx], bound) != c:
                    return True
        return False

    for f in range(F):
        for y in range(H):
            for x in range(W):
                c = [int(k) for k in rgb[f, y, x]]
                e = ident(est, est[f, y, x], True)
                if e >= 0:
                    lit = [(int(tint[e][k]) * int(shade[f, y, x]) + 127) // 255 for k in range(3)]
                    c = [(c[k] * (256 - alpha) + lit[k] * alpha + 128) >> 8 for k in range(3)]
                if is_edge(est, f, y, x, True):
                    c = [int(k) for k in tint[e]]
                if gt is not None and is_edge(gt, f, y, x, False):
                    c = list(col)
                out[f, y, x] = c
    return out


def test_overlay_ref_against_a_pixel_loop():
    rng = np.random.default_rng(5)
    F, H, W = 2, 9, 11
    rgb = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    shade = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    tint = np.array([(230, 25, 75), (0, 255, 0), (255, 255, 255)], np.uint8)
    est = np.full((F, H, W), -1, np.int32)
    est[0, 0:4, 0:5] = 0                                 # a region in the frame's corner: its outline stops at the border
    est[0, 3:9, 7:11] = 1                                # flush with the bottom right corner
    est[0, 6, 2] = 2                                     # a single pixel
    est[1] = 1                                           # a whole frame of one id: no edge anywhere
    est[1, 4, 5] = 3                                     # an id outside [0, N): counts as -1, and makes an edge
    est[1, 0, 0] = -5
    gt = np.full((F, H, W), -1, np.int32)
    gt[0, 2:7, 3:9] = 0
    gt[1, :, 0:6] = 7                                    # a gt id is taken as it stands
    for alpha, radius, g in ((128, 1, gt), (0, 1, None), (256, 1, None), (77, 4, gt), (200, 2, None)):
        want = _overlay_loop(rgb, est, shade, tint, alpha, radius, g, (9, 250, 31))
        got = sf.overlay(rgb, est, shade, tint, alpha, radius, g, (9, 250, 31))
        assert np.array_equal(got, want), (alpha, radius)
    r1 = sf.overlay(rgb, est, shade, tint, 0, 1)
    inner = np.zeros((F, H, W), bool)
    inner[0, 0:3, 0:4] = True                            # the corner region's pixels away from its inner border
    assert np.array_equal(r1[inner], rgb[inner])         # alpha 0 off the outline: the frame itself
    assert (r1[0, 3, 0:5] == tint[0]).all() and (r1[0, 0:4, 4] == tint[0]).all()   # the outline, in the plain tint
    assert np.array_equal(r1[1, 6:9, 7:11], rgb[1, 6:9, 7:11]) and (r1[1, 4, 5] == rgb[1, 4, 5]).all()
    assert (r1[1, 0, 0] == rgb[1, 0, 0]).all() and (r1[1, 1, 1] == tint[1]).all()   # a negative id is no instance
    assert (r1[1, 3:6, 4:7][np.arange(9).reshape(3, 3) != 4] == tint[1]).all()      # the ring about the foreign id
    r2 = sf.overlay(rgb, est, shade, tint, 256, 1)
    lit = (tint[0].astype(np.int64) * int(shade[0, 1, 1]) + 127) // 255
    assert (r2[0, 1, 1] == lit).all()                    # alpha 256: the lit tint alone


def _diff_loop(ren, obs, scale, tol):
    out = np.zeros(ren.shape + (3,), np.uint8)
    for i in np.ndindex(ren.shape):
        r, o = float(ren[i]), float(obs[i]) / scale
        if r > 0 and o > 0:
            e = r - o
            k = int(min(abs(e) / tol, 1.0) * 255.0 + 0.5)
            out[i] = (255, 255 - k, 255 - k) if e > 0 else ((255 - k, 255 - k, 255) if e < 0 else (255, 255, 255))
        elif r > 0:
            out[i] = (128, 128, 128)
    return out


def test_depth_diff_ref_against_a_pixel_loop():
    rng = np.random.default_rng(6)
    ren = (0.5 + rng.random((2, 7, 9))).astype(np.float32)
    obs = (ren.astype(np.float64) + rng.uniform(-0.04, 0.04, ren.shape)).astype(np.float32)
    ren[0, 0, :3] = 0.0
    obs[0, 1, :3] = 0.0
    obs[0, 0, 0] = 0.0
    obs[1, 2, 2] = np.nan
    ren[1, 3, 3] = np.nan
    obs[1, 4, 4] = ren[1, 4, 4]
    obs[1, 5, 5] = -1.0
    for scale, tol in ((1.0, 0.02), (1000.0, 0.02), (1.0, 0.5), (-1.0, 0.02)):
        o = (obs.astype(np.float64) * scale).astype(np.float32) if scale > 0 else obs
        assert np.array_equal(sf.depth_diff(ren, o, scale, tol), _diff_loop(ren, o, scale, tol)), (scale, tol)
    got = sf.depth_diff(ren, obs)
    assert got[0, 0, 0].tolist() == [0, 0, 0] and got[0, 0, 1].tolist() == [0, 0, 0]
    assert got[0, 1, 0].tolist() == [128, 128, 128] and got[1, 2, 2].tolist() == [128, 128, 128]
    assert got[1, 3, 3].tolist() == [0, 0, 0] and got[1, 4, 4].tolist() == [255, 255, 255]
    assert got[1, 5, 5].tolist() == [128, 128, 128]


def test_scene_conditions_hold():
    """The generic scenes of the GPU tests have no undecided pixel; the tie scene's answers are exact."""
    for name in ("overlap", "frames"):
        sf.check_conditions(sf.reference(name))
    tie = sf.reference("ties")
    assert set(np.unique(tie["inst"][0])) == {-1, 0} and set(np.unique(tie["inst"][1])) == {-1, 2, 3}
    assert set(np.unique(tie["z"][1])) == {0.0, 1.0}


# ------------------------------------------------------------------------------------------------------ refusals

def test_palette():
    p = scene.palette([1, 2, 13, 12, 0])
    assert p.dtype == np.uint8 and p.shape == (5, 3)
    assert (p[0] == p[2]).all() and (p[3] == p[4]).all() and not (p[0] == p[1]).all()
    assert len({tuple(c) for c in scene.palette(range(12))}) == 12
    assert scene.palette([]).shape == (0, 3)


def test_bindings_refuse_before_touching_a_device():
    v, f = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    args = ([(0, 2)], np.eye(3)[None], [[0, 0, 1.0]], [[1.0, 1.0, 0, 0]], [(0, 1)], 8, 8)
    with pytest.raises(RuntimeError, match="HIP path only"):
        scene.render(v, f, *args)
    for bad in (v.double(), v[:, :2], v.reshape(-1), np.zeros((4, 3), np.float32), torch.zeros((4, 6))[:, ::2]):
        with pytest.raises(ValueError, match="verts must be"):
            scene.render(bad, f, *args)
    for bad in (f.long(), f.float(), f[:, :2]):
        with pytest.raises(ValueError, match="faces must be"):
            scene.render(v, bad, *args)
    rgb = torch.zeros((1, 4, 5, 3), dtype=torch.uint8)
    est, sh = torch.zeros((1, 4, 5), dtype=torch.int32), torch.zeros((1, 4, 5), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP path only"):
        scene.overlay(rgb, est, sh, [(1, 2, 3)])
    for bad in (rgb.float(), rgb[..., :2], rgb[0], rgb.permute(0, 3, 1, 2)):
        with pytest.raises(ValueError, match="rgb must be"):
            scene.overlay(bad, est, sh, [(1, 2, 3)])
    with pytest.raises(ValueError, match="est must be"):
        scene.overlay(rgb, est.long(), sh, [(1, 2, 3)])
    with pytest.raises(ValueError, match="est must be"):
        scene.overlay(rgb, est[:, :3], sh, [(1, 2, 3)])
    with pytest.raises(ValueError, match="shade must be"):
        scene.overlay(rgb, est, sh.int(), [(1, 2, 3)])
    with pytest.raises(ValueError, match="gt must be"):
        scene.overlay(rgb, est, sh, [(1, 2, 3)], gt=sh)
    d = torch.zeros((1, 4, 5))
    with pytest.raises(RuntimeError, match="HIP path only"):
        scene.depth_diff(d, d.clone())
    with pytest.raises(ValueError, match="ren must be"):
        scene.depth_diff(d.double(), d)
    with pytest.raises(ValueError, match="obs must be"):
        scene.depth_diff(d, d[:, :3])


def test_vis_refusals(tmp_path):
    """Raised before the model, a batch or a device is touched: the model is a dummy."""
    import bop_tree
    from pose_estimation_amd.dataset import PoseDataset
    from pose_estimation_amd.evaluate import test_epoch as run_epoch
    root = str(tmp_path / "tree")
    bop_tree.write_tree(root)
    dummy = torch.nn.Linear(1, 1)
    out = str(tmp_path / "vis")
    bare = PoseDataset("test", 500, False, root, 0.0, 8, n_model_pts=4, layout="bop")
    lm = PoseDataset("test", 500, False, None, 0.0, 8, cls_type="all", num_frames=2)
    for ds in (bare, lm):
        with pytest.raises(ValueError, match="vis_results needs.*layout='bop'.*meshes=True"):
            bop_scene.vis_results(ds, [], out, "cpu")
        with pytest.raises(ValueError, match="vis_dir.*layout='bop'.*meshes=True"):
            run_epoch(dummy, ds, bs=2, device="cpu", vis_dir=out)
    full = PoseDataset("test", 500, False, root, 0.0, 8, n_model_pts=4, layout="bop", meshes=True)
    with pytest.raises(ValueError, match="vis_dir runs on one rank"):
        run_epoch(dummy, full, bs=2, device="cpu", vis_dir=out, world=2, rank=0)
    assert not os.path.exists(out)


def test_vis_is_off_by_default():
    from pose_estimation_amd.evaluate import test_epoch as run_epoch
    par = inspect.signature(run_epoch).parameters
    assert par["vis_dir"].default is None and par["vis_diff"].default is False
    par = inspect.signature(bop_scene.vis_results).parameters
    assert [(k, par[k].default) for k in ("gt", "diff", "chunk_images", "alpha", "radius", "tol", "overwrite")] == [
        ("gt", True), ("diff", False), ("chunk_images", 8), ("alpha", 128), ("radius", 1), ("tol", 0.02),
        ("overwrite", False)]
