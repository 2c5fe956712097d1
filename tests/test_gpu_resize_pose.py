"""The fractional maps of a resized crop are the right geometry: PnP on exact correspondences through
build_inputs(resize=T) recovers the pose from 2x-reduced crops as well as from native ones, and loses it by far more
than the bound when the maps are rounded to whole pixels. No network: pred["xyz"] is made analytically.

Construction (numpy, f64). Per crop an ellipsoid with a LineMOD object's extents (models_info) under a known pose.
The depth frame holds the ellipsoid's surface along the ray of every integer pixel of the crop's window. For every
resized pixel (i, j) the ray through its centre (c0 + centre(j), r0 + centre(i)), the value x_map / y_map must have,
is intersected with the ellipsoid; the hit in normalised model coordinates is pred["xyz"][:, i, j], and mask_label
is set at the pixel's nearest source pixel where both rays hit. So a correct map makes every correspondence exact
up to f32, and a map that is off by half a source pixel shifts every image point by that much.

Bound. The native crops (side 80 == T) measure the path's own error e0 on this construction; the
side-160 crops must stay within MULT * e0 + FLOOR. FLOOR is what f32 alone allows: a pixel coordinate below 640
rounds by at most 640 * 2^-24 = 3.8e-5 px, which is 6.7e-8 rad at f = 572 px and 6.7e-8 m at 1 m; 1e-6 rad and 1e-6 m
leave 15x. Measured on an MI355X over seeds 0..4 (rotation rad / translation m): e0 5.9e-8 .. 9.7e-8 / 2.4e-8 ..
9.8e-8, side 160 6.6e-8 .. 7.9e-8 / 2.9e-8 .. 4.3e-8, at most 1.47x its seed's e0, so MULT = 4 leaves 2.7x over the
worst seed. The control (maps rounded to integers: half a source pixel) read at least 8.4e-4 / 5.7e-4 and must
exceed 10x the bound, or the bound discriminates nothing."""
import numpy as np
import pytest
import torch

from pose_estimation_amd.config import models_info
from pose_estimation_amd.dataset import build_inputs
from pose_estimation_amd.pose import get_pose
from pose_estimation_amd.synthetic import LM_K, rand_rotation
from tests import resize_ref as R

pytestmark = pytest.mark.gpu

H, W, T, N = 480, 640, 80, 1000
SIDES = [80, 160, 80, 160]
OBJS = [1, 5, 6, 9]
MULT = 4.0
FLOOR_ROT, FLOOR_T = 1e-6, 1e-6  # rad, metres


def _hit(u, v, K, Rm, t, centre, semi):
    """The nearest intersection of the rays through pixels (u, v) with the ellipsoid (model frame: centre, semi-axes)
    under pose (Rm, t). Returns (hit mask, depth along z, model coordinates [..., 3])."""
    fx, fy, cx, cy = K
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)  # camera ray, z = 1
    dm = d @ Rm                               # R^T d, per row
    om = (-t) @ Rm - centre                   # R^T (0 - t) - centre
    a = ((dm / semi) ** 2).sum(-1)
    b = 2 * ((dm / semi) * (om / semi)).sum(-1)
    c = ((om / semi) ** 2).sum() - 1.0
    disc = b * b - 4 * a * c
    hit = disc > 0
    lam = (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a)
    return hit, lam, om + lam[..., None] * dm + centre


def make_case(seed):
    """Frames, windows, poses and the analytic xyz of B = 4 crops (sides 80 and 160 at T = 80)."""
    rng = np.random.default_rng(seed)
    info = models_info()
    B = len(SIDES)
    K = np.array([LM_K[0, 0], LM_K[1, 1], LM_K[0, 2], LM_K[1, 2]], np.float64)
    depth = np.zeros((B, H, W), np.float32)
    ml = np.zeros((B, H, W), np.uint8)
    xyz = np.zeros((B, 3, T, T), np.float32)
    boxes, Rs, ts, exts, lfbs = [], [], [], [], []
    for b, (S, obj) in enumerate(zip(SIDES, OBJS)):
        lfb, ext = np.array(info[obj]["min"]) / 1000.0, np.array(info[obj]["size"]) / 1000.0
        centre, semi = lfb + ext / 2, ext / 2
        r0, c0 = int(rng.integers(0, H - S + 1)), int(rng.integers(0, W - S + 1))
        z = ext.max() * K[0] / (0.8 * S)  # the largest extent spans 0.8 of the window
        Rm = rand_rotation(rng)
        uc, vc = c0 + (S - 1) / 2 + rng.uniform(-2, 2), r0 + (S - 1) / 2 + rng.uniform(-2, 2)
        t = np.array([(uc - K[2]) * z / K[0], (vc - K[3]) * z / K[1], z]) - Rm @ centre
        vv, uu = np.mgrid[r0:r0 + S, c0:c0 + S].astype(np.float64)
        hit_i, lam_i, _ = _hit(uu, vv, K, Rm, t, centre, semi)
        depth[b, r0:r0 + S, c0:c0 + S] = np.where(hit_i, lam_i, 0.0)
        ctr, n = R.centre(S, T), R.nearest(S, T)
        assert len(set(n.tolist())) == T  # distinct nearest pixels: the label can be set per resized pixel
        hit_r, _, pm = _hit(np.broadcast_to(c0 + ctr[None, :], (T, T)), np.broadcast_to(r0 + ctr[:, None], (T, T)), K,
                            Rm, t, centre, semi)
        ok = hit_r & hit_i[n[:, None], n[None, :]]
        ml[b, (r0 + n)[:, None], (c0 + n)[None, :]] = ok * 255
        xyz[b] = np.where(ok[..., None], (pm - lfb) / ext, 0.0).transpose(2, 0, 1)
        assert ok.sum() > N
        boxes.append((r0, r0 + S, c0, c0 + S))
        Rs.append(Rm), ts.append(t), exts.append(ext), lfbs.append(lfb)
    g = torch.Generator().manual_seed(seed)
    sel = torch.stack([torch.randperm(N, generator=g)[:256] for _ in range(B)]).int()
    subsets = torch.stack([torch.randperm(256, generator=g)[:5] for _ in range(B * 100)]).view(B, 100, 5).int()
    return {"depth": depth, "mask_label": ml, "xyz": xyz, "boxes": boxes, "K": K, "R": np.stack(Rs), "t": np.stack(ts),
            "extent": np.stack(exts), "lfborder": np.stack(lfbs), "sel": sel, "subsets": subsets}


def _errors(Re, te, case):
    Re, te = Re.double().cpu().numpy(), te.double().cpu().numpy()
    rot = np.array([2 * np.arcsin(min(1.0, np.linalg.norm(Re[b] - case["R"][b]) / (2 * np.sqrt(2))))
                    for b in range(len(Re))])
    return rot, np.linalg.norm(te - case["t"], axis=1)


def solve(dev, case, round_maps=False):
    """(data, rotation errors [B] rad, translation errors [B] m) of get_pose on build_inputs(resize=T)'s batch."""
    B = len(SIDES)
    fr = {"rgb": torch.zeros((B, H, W, 3), dtype=torch.uint8, device=dev),
          "depth": torch.from_numpy(case["depth"]).to(dev), "mask_label": torch.from_numpy(case["mask_label"]).to(dev)}
    K4 = torch.tensor(np.tile(case["K"], (B, 1)), dtype=torch.float32)
    seed = torch.tensor([11], dtype=torch.int64, device=dev)
    data = build_inputs(fr, list(range(B)), case["boxes"], N, K4, seed, stream_id=2, resize=T)
    data.update({"intrinsic": K4.to(dev), "extent": torch.from_numpy(case["extent"]).to(dev),
                 "lfborder": torch.from_numpy(case["lfborder"]).to(dev)})
    if round_maps:
        data = dict(data, x_map_choosed=torch.round(data["x_map_choosed"]), y_map_choosed=torch.round(data["y_map_choosed"]))
    Re, te = get_pose({"xyz": torch.from_numpy(case["xyz"]).to(dev)}, data, sel=case["sel"], subsets=case["subsets"])
    torch.cuda.synchronize()
    return (data,) + _errors(Re, te, case)


def measure(dev, seed):
    """The figures the bound is made of: e0 (native crops), the side-160 crops' error and the control's, each the
    maximum over its crops, as (rotation rad, translation m) pairs."""
    case = make_case(seed)
    native = [b for b, S in enumerate(SIDES) if S == T]
    big = [b for b, S in enumerate(SIDES) if S != T]
    data, rot, tr = solve(dev, case)
    _, crot, ctr = solve(dev, case, round_maps=True)
    return {"case": case, "data": data, "e0": (rot[native].max(), tr[native].max()),
            "resized": (rot[big].max(), tr[big].max()), "control": (crot[big].min(), ctr[big].min())}


def test_fractional_maps_are_the_geometry(dev):
    m = measure(dev, seed=0)
    print("e0 %r resized %r control %r" % (m["e0"], m["resized"], m["control"]))
    bound = (MULT * m["e0"][0] + FLOOR_ROT, MULT * m["e0"][1] + FLOOR_T)
    assert m["resized"][0] <= bound[0] and m["resized"][1] <= bound[1], (m["resized"], bound)
    # the control: whole-pixel maps are half a source pixel off; either figure exceeding 10x its bound would show a
    # wrong map, both must, or the bound above could not tell the two apart
    assert m["control"][0] > 10 * bound[0] and m["control"][1] > 10 * bound[1], (m["control"], bound)

    # every cloud row is a pixel of the depth frame, back-projected: bit for bit
    case, data = m["case"], m["data"]
    fx, fy, cx, cy = [np.float32(v) for v in case["K"]]
    cloud = data["cloud"].cpu().numpy()
    for b in range(len(SIDES)):
        z = cloud[b, :, 2]
        col = np.rint(cloud[b, :, 0].astype(np.float64) * fx / z + cx).astype(np.int64)
        row = np.rint(cloud[b, :, 1].astype(np.float64) * fy / z + cy).astype(np.int64)
        r0, r1, c0, c1 = case["boxes"][b]
        assert (row >= r0).all() and (row < r1).all() and (col >= c0).all() and (col < c1).all()
        pt2 = case["depth"][b, row, col]
        assert (pt2 != 0).all()
        ref = np.stack([(col.astype(np.float32) - cx) * pt2 / fx, (row.astype(np.float32) - cy) * pt2 / fy, pt2], 1)
        assert np.array_equal(cloud[b].view(np.uint32), ref.astype(np.float32).view(np.uint32)), b
