"""krrn_pose_windows_f64 called directly, every output between sentinel guards, against tests/zoom_ref.py's numpy
restatement with array_equal: P at the wave and block edges, two frame sizes, one case per branch of the rule, the
extreme points at index 0, at P - 1 and at the last lane of the last wave, and the argument refusals.

The branch cases use a camera under which a point's pixel is exact: R = I, t = (0, 0, 1), z = 0, so Z = 1 and
u = fx x + cx with fx = 2 and x a multiple of 1 / 16; with pad = 1.25 the products are exact too, so the `ceil` and
`floor` edges are hit exactly and not to rounding. The pose cases use real rotations, a LineMOD-like K and the
default pad."""
import numpy as np
import pytest
import torch

from pose_estimation_amd import _lib, zoom
from pose_estimation_amd._lib import P as PTR, stream_ptr
from tests import zoom_ref as Z
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu

EARG, ESHAPE = -1, -2
B = 7
PS = [1, 63, 64, 65, 255, 256, 257, 2600]
FRAMES = {"480x640": dict(H=480, W=640, q=10, ms=40, T=80), "48x64": dict(H=48, W=64, q=1, ms=8, T=40)}
FX = 2.0
PAD = 1.25


def _dev(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _outputs(dev, nb):
    return {"rc": Guarded(dev, (nb, 2), torch.int32), "side": Guarded(dev, (nb,), torch.int32),
            "bbox": Guarded(dev, (nb, 4), torch.float32), "scale": Guarded(dev, (nb,), torch.float32),
            "intr": Guarded(dev, (nb, 4), torch.float32), "status": Guarded(dev, (nb,), torch.int32)}


def _args(ins, out, nb, npts, H, W, T, pad, ms):
    return [PTR(ins["pts"].data_ptr()), npts, PTR(ins["R"].data_ptr()), PTR(ins["t"].data_ptr()),
            PTR(ins["K4"].data_ptr()), H, W, T, float(pad), ms, PTR(ins["rc_in"].data_ptr()),
            PTR(ins["side_in"].data_ptr()), nb, PTR(out["rc"].ptr), PTR(out["side"].ptr), PTR(out["bbox"].ptr),
            PTR(out["scale"].ptr), PTR(out["intr"].ptr), PTR(out["status"].ptr)]


def _prev(nb):
    """Previous windows that no rule would produce: a row that keeps its window must return exactly these."""
    return (np.array([[3 + b, 5 + 2 * b] for b in range(nb)], np.int32), np.array([11 + b for b in range(nb)], np.int32))


def _run(dev, pts, R, t, K4, H, W, T, pad, ms):
    nb, npts = pts.shape[:2]
    rc_in, side_in = _prev(nb)
    ins = {"pts": _dev(dev, pts.astype(np.float32)), "R": _dev(dev, R.astype(np.float64)),
           "t": _dev(dev, t.astype(np.float64)), "K4": _dev(dev, K4.astype(np.float32)), "rc_in": _dev(dev, rc_in),
           "side_in": _dev(dev, side_in)}
    out = _outputs(dev, nb)
    assert _lib.lib().krrn_pose_windows_f64(*_args(ins, out, nb, npts, H, W, T, pad, ms), stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    got = {k: v.get() for k, v in out.items()}
    ref = Z.windows(pts.astype(np.float32), R, t, K4.astype(np.float32), H, W, T, pad, ms, rc_in, side_in)
    return got, ref, rc_in, side_in


def _same(got, ref):
    for k in ("rc", "side", "status"):
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    for k in ("bbox", "scale", "intr"):
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (k, got[k], ref[k])


def _slots(npts):
    """Where the extreme points go: (index of the (umin, vmin) corner, index of the (umax, vmax) corner)."""
    last_lane = (npts // 256) * 256 - 1 if npts >= 256 else npts - 1  # the largest i < P with i % 256 == 255
    return [(0, npts - 1), (npts - 1, 0), (npts // 2, last_lane)]


def _cloud(rng, npts, box, slot, K4):
    """P points whose pixels lie strictly inside `box` = (umin, umax, vmin, vmax), on a 1 / 8 pixel grid, except the
    two corner points at `slot`; as camera-plane points (z = 0) of the exact camera."""
    umin, umax, vmin, vmax = box
    u = umin + (umax - umin) * np.round(rng.uniform(0.25, 0.75, npts) * 8) / 8
    v = vmin + (vmax - vmin) * np.round(rng.uniform(0.25, 0.75, npts) * 8) / 8
    a, b = slot
    u[a], v[a] = umin, vmin
    u[b], v[b] = umax, vmax  # P == 1: the one point is the (umax, vmax) corner
    pts = np.stack([(u - K4[2]) / K4[0], (v - K4[3]) / K4[1], np.zeros(npts)], 1)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts), "the case is not exact in f32"
    return pts


def _cases(fr, npts):
    """name -> (box, R, t) under the exact camera; the boxes in units of q = W / 64."""
    H, W, q = fr["H"], fr["W"], fr["q"]
    eye, t1 = np.eye(3).reshape(9), np.array([0.0, 0.0, 1.0])
    mid = (30.0 * q, 22.0 * q)

    def box(cu, cv, eu, ev):
        return (cu - eu / 2, cu + eu / 2, cv - ev / 2, cv + ev / 2)

    c = {
        "centred": (box(mid[0] + 3.25, mid[1] - 2.75, 16 * q, 10 * q), eye, t1),
        "cut_left": (box(2.0 * q, mid[1], 12 * q, 6 * q), eye, t1),
        "cut_right": (box(W - 2.0 * q, mid[1], 12 * q, 6 * q), eye, t1),
        "cut_top": (box(mid[0], 2.0 * q, 6 * q, 12 * q), eye, t1),
        "cut_bottom": (box(mid[0], H - 2.0 * q, 6 * q, 12 * q), eye, t1),
        "larger_than_frame": (box(mid[0], mid[1], 3 * W, 2 * H), eye, t1),
        "tiny": (box(mid[0], mid[1], 0.25 * q, 0.125 * q), eye, t1),
        "z_zero": (box(mid[0], mid[1], 16 * q, 10 * q), eye, t1),
        "z_negative": (box(mid[0], mid[1], 16 * q, 10 * q), eye, t1),
        "nan_in_R": (box(mid[0], mid[1], 16 * q, 10 * q), np.where(np.arange(9) == 1, np.nan, eye), t1),
        "nan_in_R_depth_row": (box(mid[0], mid[1], 16 * q, 10 * q), np.where(np.arange(9) == 8, np.nan, eye), t1),
        "inf_in_t": (box(mid[0], mid[1], 16 * q, 10 * q), eye, np.array([np.inf, 0.0, 1.0])),
        "left_of_frame": (box(-9.0 * q, mid[1], 8 * q, 8 * q), eye, t1),
        "right_of_frame": (box(W + 9.0 * q, mid[1], 8 * q, 8 * q), eye, t1),
        "above_frame": (box(mid[0], -9.0 * q, 8 * q, 8 * q), eye, t1),
        "below_frame": (box(mid[0], H + 9.0 * q, 8 * q, 8 * q), eye, t1),
        # the frame test's own edges: umax == 0 and umin == W - 1 are still inside
        "touches_left": (box(-4.0 * q, mid[1], 8 * q, 8 * q), eye, t1),
        "touches_right": (box(W - 1 + 4.0 * q, mid[1], 8 * q, 8 * q), eye, t1),
        # e * pad an exact integer (16 q * 1.25 = 20 q), and just above one (+ 1 / 8 pixel: 20 q + 0.15625)
        "ceil_exact": (box(mid[0], mid[1], 16 * q, 10 * q), eye, t1),
        "ceil_above": (box(mid[0], mid[1], 16 * q + 0.125, 10 * q), eye, t1),
        # floor's argument (umin + umax) / 2 - S / 2 + 1 with fraction exactly .0 and .5: an even and an odd side, a
        # centre at .0 and at .5
        "floor_even_0": (box(mid[0], mid[1], 16 * q, 16 * q), eye, t1),
        "floor_even_5": (box(mid[0] + 0.5, mid[1] + 0.5, 16 * q, 16 * q), eye, t1),
        "floor_odd_0": (box(mid[0] + 0.5, mid[1] + 0.5, 16 * q + 0.125, 16 * q + 0.125), eye, t1),
        "floor_odd_5": (box(mid[0], mid[1], 16 * q + 0.125, 16 * q + 0.125), eye, t1),
    }
    return c


def _case_batch(fr, npts):
    """Every case, then the centred one again with the other placements of its extreme points; padded to a multiple
    of B crops. Returns (names, pts [n, P, 3], R [n, 9], t [n, 3], K4 [n, 4])."""
    rng = np.random.default_rng(npts)
    K4 = np.array([FX, FX, fr["W"] / 2 + 1.0, fr["H"] / 2 - 1.0])
    slots = _slots(npts)
    names, pts, Rs, ts = [], [], [], []
    cases = _cases(fr, npts)
    for k, (name, (bx, R, t)) in enumerate(cases.items()):
        p = _cloud(rng, npts, bx, slots[k % 3], K4)
        if name == "z_zero":
            p[npts - 1, 2] = -1.0   # Z = z + 1 = 0
        if name == "z_negative":
            p[0, 2] = -2.0
        names.append(name), pts.append(p), Rs.append(R), ts.append(t)
    for s in slots:
        names.append(f"centred@{s}"), pts.append(_cloud(rng, npts, cases["centred"][0], s, K4))
        Rs.append(cases["centred"][1]), ts.append(cases["centred"][2])
    while len(names) % B:
        names.append("pad"), pts.append(pts[0]), Rs.append(Rs[0]), ts.append(ts[0])
    n = len(names)
    return names, np.stack(pts), np.stack(Rs), np.stack(ts), np.tile(K4, (n, 1))


@pytest.mark.parametrize("npts", PS)
@pytest.mark.parametrize("frame", list(FRAMES))
def test_branch_cases_match_the_restatement(dev, frame, npts):
    fr = FRAMES[frame]
    H, W, q, ms, T = fr["H"], fr["W"], fr["q"], fr["ms"], fr["T"]
    names, pts, R, t, K4 = _case_batch(fr, npts)
    row = {}
    for lo in range(0, len(names), B):
        sl = slice(lo, lo + B)
        got, ref, rc_in, side_in = _run(dev, pts[sl], R[sl], t[sl], K4[sl], H, W, T, PAD, ms)
        _same(got, ref)
        keep = got["status"] != 0
        assert np.array_equal(got["rc"][keep], rc_in[keep]) and np.array_equal(got["side"][keep], side_in[keep])
        for k, name in enumerate(names[sl]):
            row[name] = dict(ref["rows"][k], got_rc=tuple(got["rc"][k]), got_side=int(got["side"][k]),
                             prev=(tuple(rc_in[k]), int(side_in[k])))
    # each case takes the branch it was built for (by the restatement, which the device equals)
    st = {n: r["status"] for n, r in row.items()}
    assert st["z_zero"] == st["z_negative"] == st["nan_in_R"] == st["nan_in_R_depth_row"] == st["inf_in_t"] == 1
    assert st["left_of_frame"] == st["right_of_frame"] == st["above_frame"] == st["below_frame"] == 2
    for n in ("z_zero", "nan_in_R", "left_of_frame"):
        assert (row[n]["got_rc"], row[n]["got_side"]) == row[n]["prev"]
    assert row["tiny"]["side"] == ms
    for n in row:
        if st[n] == 0:
            (r0, c0), S = row[n]["rc"], row[n]["side"]
            assert ms <= S <= min(H, W) and 0 <= r0 <= H - S and 0 <= c0 <= W - S, n
    if npts == 1:  # one point: every box is that point, the side is min_side
        return
    assert st["touches_left"] == st["touches_right"] == 0
    assert row["larger_than_frame"]["side"] == min(H, W) and row["larger_than_frame"]["rc"][0] == 0
    assert row["centred"]["status"] == 0 and not row["centred"]["clamped"]
    assert len({(row[n]["rc"], row[n]["side"]) for n in row if n.startswith("centred")}) == 1
    assert row["cut_left"]["rc"][1] == 0 and row["cut_right"]["rc"][1] == W - row["cut_right"]["side"]
    assert row["cut_top"]["rc"][0] == 0 and row["cut_bottom"]["rc"][0] == H - row["cut_bottom"]["side"]
    assert all(row[n]["clamped"] for n in ("cut_left", "cut_right", "cut_top", "cut_bottom"))
    assert row["ceil_exact"]["side"] == 20 * q and row["ceil_above"]["side"] == 20 * q + 1
    # side 20 q, centre 30 q: floor(30 q - 10 q + 1) exactly; half a pixel on: the .5 floors away
    assert row["floor_even_0"]["rc"][1] == 20 * q + 1 and row["floor_even_5"]["rc"][1] == 20 * q + 1
    # side 20 q + 1: centre .5 gives an exact integer, centre .0 a fraction of .5
    assert row["floor_odd_0"]["rc"][1] == 20 * q + 1 and row["floor_odd_5"]["rc"][1] == 20 * q


def _poses(npts, H, W, seed):
    """B crops with real rotations, a LineMOD-like K scaled to the frame and object-sized point clouds about a metre
    away, projecting near the frame's middle: what an eval batch feeds the kernel."""
    rng = np.random.default_rng(seed)
    sc = W / 640.0
    K4 = np.array([[572.4114 * sc * (1 + 0.01 * b), 573.57043 * sc, 325.2611 * sc + b, 242.04899 * sc - b]
                   for b in range(B)], np.float32)
    Rm = np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(B)])
    Rm *= np.sign(np.linalg.det(Rm))[:, None, None]
    z = rng.uniform(0.5, 1.2, B)
    t = np.stack([rng.uniform(-0.25, 0.25, B) * z, rng.uniform(-0.2, 0.2, B) * z, z], 1)
    pts = ((rng.random((B, npts, 3)) - 0.5) * rng.uniform(0.05, 0.25, (B, 1, 3))).astype(np.float32)
    return pts, Rm.reshape(B, 9), t, K4


@pytest.mark.parametrize("npts", PS)
@pytest.mark.parametrize("frame", list(FRAMES))
def test_pose_batches_match_the_restatement(dev, frame, npts):
    """Real poses with the default pad (1.2: inexact products) and the default min_side where the frame holds it."""
    fr = FRAMES[frame]
    H, W = fr["H"], fr["W"]
    pts, R, t, K4 = _poses(npts, H, W, seed=npts + H)
    got, ref, _, _ = _run(dev, pts, R, t, K4, H, W, fr["T"], zoom.ZOOM_PAD, zoom.ZOOM_MIN_SIDE)
    _same(got, ref)
    assert (got["status"] == 0).any()


def test_the_python_entry_point_stages_the_pose_as_f64(dev):
    """zoom.pose_windows with an f32 [B, 3, 3] rotation and f32 t, as the solver returns them, equals the restatement
    fed the same values widened to f64."""
    H, W, T = 480, 640, 80
    pts, R, t, K4 = _poses(257, H, W, seed=3)
    R32, t32 = R.astype(np.float32), t.astype(np.float32)
    rc_in, side_in = _prev(B)
    out = zoom.pose_windows(_dev(dev, pts), _dev(dev, R32).reshape(B, 3, 3), _dev(dev, t32), _dev(dev, K4), (H, W),
                            _dev(dev, rc_in), _dev(dev, side_in), T)
    torch.cuda.synchronize()
    ref = Z.windows(pts, R32.astype(np.float64), t32.astype(np.float64), K4, H, W, T, zoom.ZOOM_PAD, zoom.ZOOM_MIN_SIDE,
                    rc_in, side_in)
    got = {k: out[o].cpu().numpy() for k, o in (("rc", "rc"), ("side", "side"), ("bbox", "bbox"),
                                               ("scale", "resize_scale"), ("intr", "resize_intrinsic"),
                                               ("status", "status"))}
    _same(got, ref)
    assert out["rc"].dtype == torch.int32 and out["status"].dtype == torch.int32 and out["bbox"].shape == (B, 4)


def test_host_refusals(dev):
    """Null pointers KRRN_EARG; B = 0 and 65536, P = 0, T = 0, H = 0, min_side = 0 and above min(H, W), pad 0,
    negative, NaN and inf KRRN_ESHAPE; nothing is launched, every output keeps its sentinel."""
    H, W, T, npts = 48, 64, 40, 5
    pts, R, t, K4 = _poses(npts, H, W, seed=1)
    rc_in, side_in = _prev(B)
    ins = {"pts": _dev(dev, pts), "R": _dev(dev, R), "t": _dev(dev, t), "K4": _dev(dev, K4), "rc_in": _dev(dev, rc_in),
           "side_in": _dev(dev, side_in)}
    out = _outputs(dev, B)
    lib, st = _lib.lib(), stream_ptr(dev)
    good = _args(ins, out, B, npts, H, W, T, 1.2, 8)
    for i in (0, 2, 3, 4, 10, 11, 13, 14, 15, 16, 17, 18):
        a = list(good)
        a[i] = PTR(0)
        assert lib.krrn_pose_windows_f64(*a, st) == EARG, i
    for i, v in [(12, 0), (12, 65536), (1, 0), (7, 0), (5, 0), (6, 0), (9, 0), (9, 49), (8, 0.0), (8, -1.2),
                 (8, float("nan")), (8, float("inf"))]:
        a = list(good)
        a[i] = v
        assert lib.krrn_pose_windows_f64(*a, st) == ESHAPE, (i, v)
    a = list(good)
    a[9] = 48  # min_side == min(H, W) is allowed
    assert lib.krrn_pose_windows_f64(*a[:13], *[PTR(o.ptr) for o in _outputs(dev, B).values()], st) == 0
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out.values())
