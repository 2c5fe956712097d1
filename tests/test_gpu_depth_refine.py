"""The depth refiner on the GPU (krrn_pose_refine_depth_f32 through depth_refine.refine) against its numpy f64
restatement (tests/depth_refine_ref.py).

passes, pairs and status are compared exactly, which the restatement's margins license
(depth_refine_ref.check_conditions: no decision of any pass within 1e-9 of flipping; test_depth_refine_host.py
asserts it for every case used here). R, t and rmse are compared within TOL = 1e-6, test_gpu_icp.py's bound: the
f32 output format's rounding, not a measured number. Scenes (frame, faces, what it pins): tetra (480 x 640, 4),
layers (4: planar faces, an unobservable slide), degenerate (87: skipped faces), sphere (1280: five face chunks,
MAX_ITER), small (90 x 120, 320: partial tiles, the object cut by two frame borders), gross and empty_obs (STARVED
in pass 0), mixed (B = 5 over one concatenated mesh, one empty face range, per-crop max_dist / radius tensors)."""
import numpy as np
import pytest
import torch

import bop_ref as br
import depth_refine_ref as dr
from pose_estimation_amd import depth_refine

pytestmark = pytest.mark.gpu

TOL = 1e-6
STARVED, MAX_ITER = dr.STATUS.index("STARVED"), dr.STATUS.index("MAX_ITER")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dt))


def _refine(dev, verts, faces, face_range, R, t, K4, frames, frame_idx, max_dist, radius, mask=None, **kw):
    Rn, tn, info = depth_refine.refine(
        _t(verts, np.float32).to(dev), _t(faces, np.int32).reshape(-1, 3).to(dev), _t(face_range, np.int32),
        _t(R, np.float32), _t(t, np.float32), _t(K4, np.float32), _t(frames, np.float32).to(dev),
        _t(frame_idx, np.int32), max_dist, radius, mask=None if mask is None else _t(mask, np.uint8).to(dev),
        depth_scale=br.DEPTH_SCALE, return_info=True, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in info.items()}
    out.update(R=Rn.cpu().numpy(), t=tn.cpu().numpy())
    return out


def _one(dev, sc, R=None, t=None, frame_idx=0, mask=None, **kw):
    R = sc["R_est"] if R is None else R
    t = sc["t_est"] if t is None else t
    got = _refine(dev, sc["verts"], sc["faces"], [[0, len(sc["faces"])]], np.asarray(R)[None], np.asarray(t)[None],
                  np.asarray(sc["K4"])[None], sc["depth"][None], [frame_idx], dr.DIST_FRAC * sc["diameter"],
                  sc["diameter"] / 2.0, mask=None if mask is None else mask[None], **kw)
    return {k: v[0] for k, v in got.items()}


def _check(tag, got, ref):
    dr.check_conditions(ref)
    dR, dt = np.abs(got["R"].astype(np.float64) - ref["R"]).max(), np.abs(got["t"].astype(np.float64) - ref["t"]).max()
    print(f"{tag}: status {dr.STATUS[int(got['status'])]} passes {int(got['passes'])} pairs {int(got['pairs'])} rmse "
          f"{float(got['rmse']):.3e} (ref {float(ref['rmse']):.3e})  |dR| {dR:.2e} |dt| {dt:.2e}")
    assert (int(got["status"]), int(got["passes"]), int(got["pairs"])) == (ref["status"], ref["passes"], ref["pairs"]), tag
    assert dR <= TOL and dt <= TOL, (tag, dR, dt)
    if np.isinf(ref["rmse"]):
        assert np.isinf(got["rmse"]) and got["rmse"] > 0, tag
    else:
        assert abs(float(got["rmse"]) - float(ref["rmse"])) <= TOL, tag
    if ref["passes"] == 0:                                       # no update: the start pose's own bits
        assert np.array_equal(_bits(got["R"]), _bits(ref["R"])) and np.array_equal(_bits(got["t"]), _bits(ref["t"])), tag


@pytest.mark.parametrize("name", br.SCENES)
def test_scene_parity(dev, name):
    _check(name, _one(dev, br.scene(name)), dr.reference(name))


def _mixed(dev, rows=None, **kw):
    bt, crops, frames = br.mixed()
    rows = list(range(len(crops))) if rows is None else rows
    dia = torch.tensor([crops[b]["diameter"] for b in rows], dtype=torch.float64)
    return _refine(dev, bt["verts"], bt["faces"], bt["face_range"][rows], np.stack([crops[b]["R_est"] for b in rows]),
                   np.stack([crops[b]["t_est"] for b in rows]), np.stack([crops[b]["K4"] for b in rows]), frames, rows,
                   dr.DIST_FRAC * dia, (dia / 2.0).to(dev), **kw)


def test_mixed_batch_parity_and_invariance(dev):
    """B = 5 over one concatenated mesh, each crop on its own frame, max_dist a host tensor and radius a device
    tensor [B]; crop 3 has an empty face range. Every crop run alone, and the same call again, give the same bits."""
    bt, crops, _ = br.mixed()
    got = _mixed(dev)
    for b in range(len(crops)):
        _check(f"mixed[{b}]", {k: v[b] for k, v in got.items()}, dr.mixed_reference(b))
    assert int(got["status"][3]) == STARVED and int(got["pairs"][3]) == 0
    assert np.array_equal(_bits(got["R"][3]), _bits(crops[3]["R_est"].astype(np.float32)))
    assert np.array_equal(_bits(got["t"][3]), _bits(crops[3]["t_est"].astype(np.float32)))
    again = _mixed(dev)
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), k
    for b in range(len(crops)):
        alone = _mixed(dev, rows=[b])
        for k in got:
            assert np.array_equal(_bits(got[k][b]), _bits(alone[k][0])), (b, k)


def test_max_iter_zero_is_one_evaluation(dev):
    sc, ref = br.scene("tetra"), dr.reference("tetra")
    got = _one(dev, sc, max_iter=0)
    assert (int(got["status"]), int(got["passes"]), int(got["pairs"])) == (MAX_ITER, 0, ref["trace"][0]["K"])
    assert np.array_equal(_bits(got["R"]), _bits(sc["R_est"].astype(np.float32)))
    assert np.array_equal(_bits(got["t"]), _bits(sc["t_est"].astype(np.float32)))
    assert abs(float(got["rmse"]) - np.sqrt(ref["trace"][0]["err"])) <= TOL


def test_mask(dev):
    """A mask that removes the occluded third changes nothing (the gate already rejects those pixels: the occluder
    is 5 cm in front, max_dist under 1 cm); the all-zero mask starves."""
    sc, ref = br.scene("tetra"), dr.reference("tetra")
    d_gt, _ = br.depth_image(sc["verts"], sc["faces"], sc["R_gt"], sc["t_gt"], sc["K4"], sc["H"], sc["W"])
    xs = np.nonzero(d_gt > 0.0)[1]
    xc = xs.min() + (2 * (xs.max() - xs.min())) // 3             # bop_ref.observed's occluder starts here
    mask = np.full(d_gt.shape, 255, np.uint8)
    mask[:, xc:] = 0
    assert (sc["depth"][:, xc:][d_gt[:, xc:] > 0.0] / br.DEPTH_SCALE < d_gt[d_gt > 0.0].min() - 0.04).all()
    plain, masked = _one(dev, sc), _one(dev, sc, mask=mask)
    _check("tetra, occluded third masked", masked, ref)
    for k in plain:
        assert np.array_equal(_bits(plain[k]), _bits(masked[k])), k
    none = _one(dev, sc, mask=np.zeros_like(mask))
    assert (int(none["status"]), int(none["passes"]), int(none["pairs"])) == (STARVED, 0, 0) and np.isinf(none["rmse"])
    assert np.array_equal(_bits(none["R"]), _bits(sc["R_est"].astype(np.float32)))


def test_poses_that_render_nothing_starve_with_their_own_bits(dev):
    """A NaN rotation, a pose behind the camera, a pose projected off the frame, and non-finite intrinsics: one
    batch beside a sound crop, which must not notice."""
    sc = br.scene("tetra")
    R, t = np.asarray(sc["R_est"], np.float32), np.asarray(sc["t_est"], np.float32)
    Rn = R.copy()
    Rn[1, 1] = np.nan
    Rs = np.stack([Rn, R, R, R, R])
    ts = np.stack([t, t * np.float32(-1.0), t + np.array([5.0, 0.0, 0.0], np.float32), t, t])
    K4 = np.stack([np.asarray(sc["K4"], np.float32)] * 5)
    K4[3, 0] = np.inf
    nf = len(sc["faces"])
    got = _refine(dev, sc["verts"], sc["faces"], [[0, nf]] * 5, Rs, ts, K4, sc["depth"][None], [0] * 5,
                  dr.DIST_FRAC * sc["diameter"], sc["diameter"] / 2.0)
    for b in range(4):
        assert (int(got["status"][b]), int(got["passes"][b]), int(got["pairs"][b])) == (STARVED, 0, 0), b
        assert np.isinf(got["rmse"][b])
        assert np.array_equal(_bits(got["R"][b]), _bits(Rs[b])) and np.array_equal(_bits(got["t"][b]), _bits(ts[b])), b
    alone = _one(dev, sc)
    for k in alone:
        assert np.array_equal(_bits(got[k][4]), _bits(alone[k])), k
    _check("tetra beside four dead crops", {k: v[4] for k, v in got.items()}, dr.reference("tetra"))


@pytest.mark.parametrize("frame_idx", [1, -1, 2 ** 30])
def test_frame_index_outside_the_frames_starves(dev, frame_idx):
    sc = br.scene("tetra")
    got = _one(dev, sc, frame_idx=frame_idx)                     # F = 1
    assert (int(got["status"]), int(got["passes"]), int(got["pairs"])) == (STARVED, 0, 0) and np.isinf(got["rmse"])
    assert np.array_equal(_bits(got["R"]), _bits(sc["R_est"].astype(np.float32)))
    ref = dr.refine(**dr.scene_args(sc, depth_obs=None, H=sc["H"], W=sc["W"]))
    assert (ref["status"], ref["passes"], ref["pairs"]) == (STARVED, 0, 0)
