"""The render family on the GPU at its tie, tile-edge, threshold and stop rules: krrn_raster_maps_f32,
krrn_bop_vsd_f32, krrn_bop_visib_u8, krrn_pose_score_f32, krrn_pose_refine_depth_f32 on the lattice scenes of
tests/lattice_ref.py, and krrn_bop_mssd_mspd_f32 at its slice edges, against the unchanged restatements
(raster_ref.render, bop_ref.vsd / mssd_mspd, bop_scene_ref.visibility, verify_ref.score, depth_refine_ref.refine).

On the lattice no number that enters a decision is rounded, so there are no margins: discrete outputs (faces,
regions, masks, counts, status, passes, pairs, indices) are compared exactly and floats bit for bit. The two
generic-scene cases (STARVED after an update, max_iter = 32) use test_gpu_depth_refine.py's comparison and its
TOL; MSSD / MSPD uses test_gpu_bop.py's MS_TOL. tests/test_lattice_host.py shows on the CPU that each case here
fails when its rule is broken.

A  rasteriser: ties_spread (640 faces, the 32 that win on both sides of every wave and chunk boundary, their
   duplicates later, 576 culled fillers between), tile_edges (vertices on a tile's first sample point and alone
   in 1-pixel partial tiles), S = 1 / 16 / 17 / 480 with NR = 1 / 256 (region ties to the lowest j), all five
   maps in guarded buffers.
B  VSD, visibility and the score on the 40 x 56 frame: poses whose boxes end on tile edges and frame borders,
   thresholds met exactly at the principal-point pixel, workspaces prefilled with 0xFF bytes and with zeros.
C  depth refiner: DEGENERATE by a zero pivot and by a zero radius, the strict gate at equality, min_pairs at
   equality, STARVED after an update, a poisoned workspace, max_iter = 32.
D  MSSD / MSPD: NS = 15 / 16 / 17 / 32 / 33, an exact tie across slices, V = 1 / 256 / 257, bad ranges and a NaN
   vertex in one batch."""
import ctypes

import numpy as np
import pytest
import torch

import bop_ref as br
import depth_refine_ref as dr
import lattice_ref as lr
import raster_ref as rr
from guarded import Guarded
from pose_estimation_amd import _lib, bop, depth_refine, verify
from test_gpu_bop import MS_TOL
from test_gpu_depth_refine import _check as refine_check, _one as refine_one
from test_gpu_raster import Launch, _compare

pytestmark = pytest.mark.gpu

P, ptr, stream_ptr = _lib.P, _lib.ptr, _lib.stream_ptr


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dt))


# ------------------------------------------------------------------------------------------------ A: rasteriser

def _launch(dev, sc):
    return Launch(dev, sc["verts"], sc["faces"], [[0, len(sc["faces"])]], np.asarray(sc["R"])[None],
                  np.asarray(sc["t"])[None], np.asarray(sc["K4"])[None], [[sc["rmin"], sc["cmin"]]], sc["S"],
                  sc["region_pts"][None])


def test_ties_spread_across_waves_and_chunks(dev):
    sc = lr.ties_spread()
    ref = lr.render_scene(sc)
    got = _launch(dev, sc).run().numpy()
    _compare(got, 0, ref, sc["rmin"], sc["cmin"], "ties_spread", exact=True)
    cov = got["face"][0] >= 0
    assert int(cov.sum()) == 1089 and (got["depth"][0][cov] == 1.0).all()
    assert np.isin(got["face"][0][cov], sc["orig"]).all()


def test_tile_edges(dev):
    sc = lr.tile_edges()
    ref = lr.render_scene(sc)
    got = _launch(dev, sc).run().numpy()
    _compare(got, 0, ref, sc["rmin"], sc["cmin"], "tile_edges", exact=True)
    cov = got["face"][0] >= 0
    for k in (16, 48):
        assert cov[k, 16:49].all() and cov[16:49, k].all(), k
    assert int(cov.sum()) == 1089


@pytest.mark.parametrize("nr", [1, 256])
@pytest.mark.parametrize("S", sorted(lr.SIZE_WINDOWS))
def test_size_edges(dev, S, nr):
    sc, ref = lr.size_scene(S, nr), lr.size_reference(S, nr)
    got = _launch(dev, sc).run().numpy()
    _compare(got, 0, ref, sc["rmin"], sc["cmin"], f"S {S} NR {nr}", exact=True)
    assert got["region"].max() <= min(nr, 128) and got["region"][0][ref["cover"]].min() >= 1


def test_raster_outputs_stay_inside_their_extents(dev):
    """B = 2, S = 17 (one whole tile and the 1-pixel partial tiles) with all five maps in guarded buffers: every
    element written (the restatement's value, never the sentinel), nothing beside them."""
    S, B = 17, 2
    scs = [lr.size_scene(17, 256), dict(lr.size_scene(17, 256), rmin=10, cmin=40)]   # the second cut by the plane's edge
    v, f = lr.plane()
    ins = [_t(v, np.float32), _t(f, np.int32), _t([[0, len(f)]] * B, np.int32),
           _t(np.stack([lr.EYE.reshape(9)] * B), np.float64), _t(np.stack([sc["t"] for sc in scs]), np.float64),
           _t(np.stack([lr.K4] * B), np.float32), _t([[sc["rmin"], sc["cmin"]] for sc in scs], np.int32),
           _t(np.stack([sc["region_pts"] for sc in scs]), np.float32)]
    vd, fd, fr, R, t, K, rc, rp = (x.to(dev) for x in ins)
    out = {"face": Guarded(dev, (B, S, S)), "depth": Guarded(dev, (B, S, S), torch.float32),
           "coord": Guarded(dev, (B, 3, S, S), torch.float32), "normal": Guarded(dev, (B, 3, S, S), torch.float32),
           "region": Guarded(dev, (B, S, S))}
    _lib.call("krrn_raster_maps_f32", ptr(vd), vd.shape[0], ptr(fd), fd.shape[0], ptr(fr), ptr(R), ptr(t), ptr(K), ptr(rc),
              S, ptr(rp), 256, B, P(out["face"].ptr), P(out["depth"].ptr), P(out["coord"].ptr), P(out["normal"].ptr),
              P(out["region"].ptr), P(0), 0, 0, stream_ptr(dev))
    torch.cuda.synchronize()
    got = {k: g.get() for k, g in out.items()}
    for b, sc in enumerate(scs):
        ref = lr.render_scene(sc)
        assert ref["cover"].any()
        for k in ("face", "region"):
            assert np.array_equal(got[k][b], ref[k]), (b, k)
        for k in ("depth", "coord", "normal"):
            assert np.array_equal(got[k][b], ref[k].astype(np.float32)), (b, k)


# ------------------------------------------------------------------------------------------ B: frame kernels

def _plane_dev(dev):
    v, f = lr.plane()
    return _t(v, np.float32).to(dev), _t(f, np.int32).to(dev)


def _ts(poses):
    return _t(np.stack([lr.t_of(p) for p in poses]), np.float64)


def _eyes(n):
    return _t(np.stack([lr.EYE] * n), np.float64)


def _vsd(dev, pairs, frames, frame_idx, delta=lr.DELTA, taus=lr.TAUS):
    """bop.vsd over (est, gt) pose-name pairs on the plane."""
    v, f = _plane_dev(dev)
    B = len(pairs)
    out = bop.vsd(v, f, _t([[0, 16]] * B, np.int32), _eyes(B), _ts([p[0] for p in pairs]), _eyes(B),
                  _ts([p[1] for p in pairs]), _t(np.stack([lr.K4] * B), np.float32), _t(frames, np.float32).to(dev),
                  _t(frame_idx, np.int32), _t([lr.DIAMETER] * B, np.float64), lr.DEPTH_SCALE, delta, taus)
    torch.cuda.synchronize()
    return out["counts"].cpu().numpy(), out["e_vsd"].cpu().numpy()


def _visib(dev, poses, frames, frame_idx, delta=lr.DELTA):
    v, f = _plane_dev(dev)
    B = len(poses)
    out = bop.visibility(v, f, _t([[0, 16]] * B, np.int32), _eyes(B), _ts(poses), _t(np.stack([lr.K4] * B), np.float32),
                         _t(frames, np.float32).to(dev), _t(frame_idx, np.int32), depth_scale=lr.DEPTH_SCALE, delta=delta)
    torch.cuda.synchronize()
    return {k: x.cpu().numpy() for k, x in out.items()}


def _score(dev, cands, frames, frame_idx, tau=lr.TAU):
    """verify.score_poses: crop b scores the candidates cands[b] (pose names) on frame frame_idx[b]; mask = the
    z1 silhouette on every frame, no box."""
    v, f = _plane_dev(dev)
    B, C = len(cands), len(cands[0])
    frames = np.asarray(frames, np.float32)
    sil = (lr.plane_depth("z1", *frames.shape[1:]) > 0.0).astype(np.uint8)
    out = verify.score_poses(v, f, _t([[0, 16]] * B, np.int32), _t(np.stack([[lr.EYE] * C] * B), np.float64),
                             _t(np.stack([[lr.t_of(p) for p in c] for c in cands]), np.float64),
                             _t(np.stack([lr.K4] * B), np.float32), _t(frames, np.float32).to(dev), _t(frame_idx, np.int32),
                             tau=tau, mask=_t(np.stack([sil] * len(frames)), np.uint8).to(dev), box=None,
                             depth_scale=lr.DEPTH_SCALE)
    torch.cuda.synchronize()
    return {k: x.cpu().numpy() for k, x in out.items()}


def _check_vsd(tag, counts, e, ref):
    print(f"{tag}: counts {counts.tolist()}  e_vsd {e.tolist()}")
    assert np.array_equal(counts, ref["counts"]), (tag, counts.tolist(), ref["counts"].tolist())
    assert np.array_equal(_bits(e), _bits(ref["e_vsd"])), tag


def _check_visib(tag, got, b, ref):
    print(f"{tag}: info {got['info'][b].tolist()}  visib_fract {got['visib_fract'][b]!r}")
    assert np.array_equal(got["mask"][b], ref["mask"].astype(np.uint8)), tag
    assert np.array_equal(got["mask_visib"][b], ref["mask_visib"].astype(np.uint8)), tag
    assert np.array_equal(got["info"][b], ref["info"]), (tag, got["info"][b].tolist(), ref["info"].tolist())
    assert np.array_equal(_bits(got["visib_fract"][b]), _bits(np.float64(ref["visib_fract"]))), tag


def _check_score(tag, got, b, ref):
    print(f"{tag}: counts {got['counts'][b].tolist()}  score {got['score'][b].tolist()}  best {got['best'][b]}")
    assert np.array_equal(got["counts"][b], ref["counts"]), (tag, got["counts"][b].tolist(), ref["counts"].tolist())
    assert np.array_equal(_bits(got["score"][b]), _bits(ref["score"])), tag
    assert int(got["best"][b]) == ref["best"], tag


VSD_PAIRS = (("near", "z1"), ("shift", "z1"), ("z1", "shift"), ("z1", "near"), ("z1", "z1"))


def test_vsd_cull_at_tile_edges_and_borders(dev):
    obs = lr.observed("z1")
    counts, e = _vsd(dev, VSD_PAIRS, obs[None], [0] * len(VSD_PAIRS))
    for b, (est, gt) in enumerate(VSD_PAIRS):
        _check_vsd(f"est {est} gt {gt}", counts[b], e[b], lr.vsd(est, gt, obs))
    assert counts[4].tolist() == [561, 561, 0, 0, 0] and not e[4].any()


def test_visibility_cull_and_both_store_paths(dev):
    """W = 56: rows of 56 bytes, every other one 16-byte aligned, and an 8-wide last tile column (per-pixel stores);
    W = 64: the same scene with every row on the 16-byte row-store path."""
    poses = ("z1", "near", "shift")
    obs = lr.observed("z1")
    got = _visib(dev, poses, obs[None], [0] * 3)
    for b, p in enumerate(poses):
        _check_visib(p, got, b, lr.visibility(p, obs))
    assert got["info"][0].tolist() == [561, 561, 561, 16, 16, 32, 16, 16, 16, 32, 16] and got["visib_fract"][0] == 1.0
    assert got["mask"][0][16:33, 48].all() and not got["mask"][0][:, 49:].any() and not got["mask"][0][:, :16].any()
    obs64 = lr.observed("z1", h=40, w=64)
    wide = _visib(dev, poses, obs64[None], [0] * 3)
    for b, p in enumerate(poses):
        _check_visib(f"{p} (W = 64)", wide, b, lr.visibility(p, obs64))
    for k in ("mask", "mask_visib"):                         # z1 lies inside both frames: the same columns
        assert np.array_equal(wide[k][0][:, :56], got[k][0]) and not wide[k][0][:, 56:].any(), k
    assert np.array_equal(wide["info"][0], got["info"][0])


def test_score_cull_at_tile_edges_and_borders(dev):
    obs = lr.observed("z1")
    cands = ("z1", "near", "shift", "z2")
    got = _score(dev, [cands], obs[None], [0])
    _check_score("z1 near shift z2", got, 0, lr.score(cands, obs))
    assert got["counts"][0].tolist() == [[561] * 6, [1536, 1536, 561, 561, 0, 1536], [408, 408, 561, 289, 289, 680],
                                         [153, 0, 561, 0, 0, 561]]


def _step(x, to):
    return float(np.nextafter(np.float64(x), to))


def test_vsd_threshold_equalities(dev):
    """At PX ray == 1: cost == 0.25 == taus[1] exactly (counted: >=) and, with raw 768 observed there, model - obs
    == delta exactly (visible: <=). One step on either threshold flips exactly that pixel."""
    flat, dip = lr.observed("z1"), lr.observed("z1", at=768.0)
    frames, pair = np.stack([dip, flat]), [("z2", "z1")] * 2
    counts, e = _vsd(dev, pair, frames, [0, 1])
    for b, obs in enumerate(frames):
        _check_vsd(f"equal, frame {b}", counts[b], e[b], lr.vsd("z2", "z1", obs))
        assert counts[b].tolist() == [561, 153, 153, 153, 0]
    taus = (0.125, _step(0.25, np.inf), 0.5)
    counts, e = _vsd(dev, pair, frames, [0, 1], taus=taus)
    for b, obs in enumerate(frames):
        _check_vsd(f"tau one step up, frame {b}", counts[b], e[b], lr.vsd("z2", "z1", obs, taus=taus))
        assert counts[b].tolist() == [561, 153, 153, 152, 0]
    delta = _step(0.25, -np.inf)
    counts, e = _vsd(dev, pair, frames, [0, 1], delta=delta)
    for b, obs in enumerate(frames):
        _check_vsd(f"delta one step down, frame {b}", counts[b], e[b], lr.vsd("z2", "z1", obs, delta=delta))
    assert counts[0].tolist() == [560, 152, 152, 152, 0] and counts[1].tolist() == [561, 153, 153, 153, 0]


def test_visibility_threshold_equality(dev):
    dip = lr.observed("z1", at=768.0)
    got = _visib(dev, ["z1"], dip[None], [0])
    _check_visib("equal", got, 0, lr.visibility("z1", dip))
    assert got["info"][0][:3].tolist() == [561, 561, 561] and got["mask_visib"][0][lr.PX[1], lr.PX[0]] == 1
    delta = _step(0.25, -np.inf)
    got = _visib(dev, ["z1"], dip[None], [0], delta=delta)
    _check_visib("delta one step down", got, 0, lr.visibility("z1", dip, delta=delta))
    assert got["info"][0][:3].tolist() == [561, 561, 560] and got["mask_visib"][0][lr.PX[1], lr.PX[0]] == 0


def test_score_threshold_equalities(dev):
    """diff == tau (raw 768) and diff == -tau (raw 1280) at PX are claimed inliers; one f32 step further out the
    near sample is occluded (claim, both, inter drop) and the far sample is claimed but no inlier (inter drops)."""
    f32 = np.float32
    raws = (768.0, 1280.0, np.nextafter(f32(768.0), f32(0.0)), np.nextafter(f32(1280.0), f32(np.inf)),
            np.nextafter(f32(768.0), f32(np.inf)), np.nextafter(f32(1280.0), f32(0.0)))
    frames = np.stack([lr.observed("z1", at=r) for r in raws])
    got = _score(dev, [("z1",)] * len(raws), frames, list(range(len(raws))))
    hand = [[561] * 6, [561] * 6, [561, 560, 561, 560, 560, 561], [561, 561, 561, 561, 560, 561], [561] * 6, [561] * 6]
    for b, obs in enumerate(frames):
        _check_score(f"raw {raws[b]!r}", got, b, lr.score(("z1",), obs))
        assert got["counts"][b, 0].tolist() == hand[b], b
    assert got["score"][:, 0].tolist() == [1.0, 1.0, 560 / 561, 560 / 561, 1.0, 1.0]
    tau = _step(0.25, -np.inf)                               # the samples on the threshold, tau one step down
    got = _score(dev, [("z1",)] * 2, frames[:2], [0, 1], tau=tau)
    for b in range(2):
        _check_score(f"tau one step down, raw {raws[b]}", got, b, lr.score(("z1",), frames[b], tau=tau))
        assert got["counts"][b, 0].tolist() == hand[2 + b], b


def _filled(dev, shape, byte):
    """A guarded int32 buffer whose view holds `byte` in every byte."""
    g = Guarded(dev, shape)
    g.view.fill_(-1 if byte else 0)
    return g


@pytest.fixture(scope="module")
def frame_operands(dev):
    """The operands the three raw frame-kernel calls share: B = 4 crops on two 40 x 56 frames."""
    v, f = _plane_dev(dev)
    B = 4
    frames = np.stack([lr.observed("z1"), lr.observed("z1", at=768.0)])
    return dict(v=v, f=f, B=B, fr=_t([[0, 16]] * B, np.int32).to(dev), R=_eyes(B).reshape(B, 9).to(dev),
                K=_t(np.stack([lr.K4] * B), np.float32).to(dev), frames=frames, d=_t(frames, np.float32).to(dev),
                fi=_t([0, 1, 0, 1], np.int32).to(dev))


def test_vsd_workspace_hygiene_and_extents(dev, frame_operands):
    o = frame_operands
    B, T = o["B"], len(lr.TAUS)
    est, gt = ("z2", "z2", "near", "shift"), ("z1", "z1", "z1", "near")
    te, tg = _ts(est).to(dev), _ts(gt).to(dev)
    dia, taus = _t([lr.DIAMETER] * B, np.float64).to(dev), _t(lr.TAUS, np.float64).to(dev)
    runs = []
    for byte in (0xFF, 0):
        ws, counts = _filled(dev, (B, 8), byte), _filled(dev, (B, 2 + T), byte)
        e = Guarded(dev, (B, T), torch.int64)                # f64 bits in an int64 buffer
        _lib.call("krrn_bop_vsd_f32", ptr(o["v"]), o["v"].shape[0], ptr(o["f"]), o["f"].shape[0], ptr(o["fr"]), ptr(o["R"]),
                  ptr(te), ptr(o["R"]), ptr(tg), ptr(o["K"]), ptr(o["d"]), 2, lr.H, lr.W, ptr(o["fi"]), lr.DEPTH_SCALE,
                  ptr(dia), lr.DELTA, ptr(taus), T, B, P(ws.ptr), P(counts.ptr), P(e.ptr), stream_ptr(dev))
        torch.cuda.synchronize()
        ws.get()
        runs.append((counts.get(), e.get().view(np.float64)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))
    for b in range(B):
        _check_vsd(f"raw vsd {b}", runs[0][0][b], runs[0][1][b], lr.vsd(est[b], gt[b], o["frames"][b % 2]))


def test_visibility_workspace_hygiene_and_extents(dev, frame_operands):
    o = frame_operands
    B = o["B"]
    poses = ("z1", "z1", "near", "shift")
    t = _ts(poses).to(dev)
    runs = []
    for byte in (0xFF, 0):
        ws = _filled(dev, (B, bop.VISIB_WS), byte)
        mask, visib = Guarded(dev, (B, lr.H, lr.W), torch.uint8), Guarded(dev, (B, lr.H, lr.W), torch.uint8)
        info, fract = Guarded(dev, (B, 11)), Guarded(dev, (B,), torch.int64)
        _lib.call("krrn_bop_visib_u8", ptr(o["v"]), o["v"].shape[0], ptr(o["f"]), o["f"].shape[0], ptr(o["fr"]), ptr(o["R"]),
                  ptr(t), ptr(o["K"]), ptr(o["d"]), 2, lr.H, lr.W, ptr(o["fi"]), lr.DEPTH_SCALE, lr.DELTA, B, P(ws.ptr),
                  P(mask.ptr), P(visib.ptr), P(info.ptr), P(fract.ptr), stream_ptr(dev))
        torch.cuda.synchronize()
        ws.get()
        runs.append({"mask": mask.get(), "mask_visib": visib.get(), "info": info.get(),
                     "visib_fract": fract.get().view(np.float64)})
    for k in runs[0]:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), k
    for b in range(B):
        _check_visib(f"raw visib {b}", runs[0], b, lr.visibility(poses[b], o["frames"][b % 2]))


def test_score_workspace_hygiene(dev, frame_operands):
    o = frame_operands
    B, C = o["B"], 3
    cands = [("z1", "near", "shift"), ("z1", "z2", "near"), ("shift", "z1", "z1"), ("z2", "near", "z1")]
    R = _t(np.stack([[lr.EYE] * C] * B), np.float64).reshape(B, C, 9).to(dev)
    t = _t(np.stack([[lr.t_of(p) for p in c] for c in cands]), np.float64).to(dev)
    sil = (lr.plane_depth("z1") > 0.0).astype(np.uint8)
    m = _t(np.stack([sil] * 2), np.uint8).to(dev)
    tau = _t([lr.TAU] * B, np.float64).to(dev)
    runs = []
    for byte in (0xFF, 0):
        ws, counts = _filled(dev, (B, C, 4), byte), _filled(dev, (B, C, 6), byte)
        score, best = Guarded(dev, (B, C), torch.int64), Guarded(dev, (B,))
        Rsel, tsel = Guarded(dev, (B, 9), torch.float32), Guarded(dev, (B, 3), torch.float32)
        _lib.call("krrn_pose_score_f32", ptr(o["v"]), o["v"].shape[0], ptr(o["f"]), o["f"].shape[0], ptr(o["fr"]), ptr(R),
                  ptr(t), C, ptr(o["K"]), ptr(o["d"]), ptr(m), 2, lr.H, lr.W, ptr(o["fi"]), P(0), lr.DEPTH_SCALE, ptr(tau),
                  B, P(ws.ptr), P(counts.ptr), P(score.ptr), P(best.ptr), P(Rsel.ptr), P(tsel.ptr), stream_ptr(dev))
        torch.cuda.synchronize()
        ws.get()
        runs.append({"counts": counts.get(), "score": score.get().view(np.float64), "best": best.get(),
                     "R": Rsel.get(), "t": tsel.get()})
    for k in runs[0]:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), k
    for b in range(B):
        ref = lr.score(cands[b], o["frames"][b % 2])
        _check_score(f"raw score {b}", runs[0], b, ref)
        assert np.array_equal(_bits(runs[0]["t"][b]), _bits(lr.t_of(cands[b][ref["best"]]).astype(np.float32))), b


# -------------------------------------------------------------------------------------------- C: depth refiner

def _refine(dev, a, B=1, radius=None, **kw):
    """depth_refine.refine on lattice_ref.refine_args `a`, the crop repeated B times (radius: per-crop values)."""
    v, f = _plane_dev(dev)
    opt = {k: a[k] for k in ("max_iter", "tol", "min_pairs", "damp") if k in a}
    opt.update(kw)
    rho = a["radius"] if radius is None else _t(radius, np.float64)
    Rn, tn, info = depth_refine.refine(
        v, f, _t([[0, 16]] * B, np.int32), _t(np.stack([a["R0"]] * B), np.float32), _t(np.stack([a["t0"]] * B), np.float32),
        _t(np.stack([a["K4"]] * B), np.float32), _t(a["depth_obs"][None], np.float32).to(dev), _t([0] * B, np.int32),
        a["max_dist"], rho, depth_scale=a["depth_scale"], return_info=True, **opt)
    torch.cuda.synchronize()
    out = {k: x.cpu().numpy() for k, x in info.items()}
    out.update(R=Rn.cpu().numpy(), t=tn.cpu().numpy())
    return out


@pytest.mark.parametrize("case", sorted(lr.REFINE_CASES))
def test_refiner_stops_on_the_lattice(dev, case):
    a, ref = lr.refine_args(case), lr.refine_reference(case)
    got = _refine(dev, a)
    status, passes, pairs, rmse = lr.REFINE_EXPECTED[case]
    spp = (int(got["status"][0]), int(got["passes"][0]), int(got["pairs"][0]))
    print(f"{case}: status {dr.STATUS[spp[0]]} passes {spp[1]} pairs {spp[2]} rmse {float(got['rmse'][0])!r}")
    assert (dr.STATUS[spp[0]],) + spp[1:] == (status, passes, pairs)
    assert spp == (ref["status"], ref["passes"], ref["pairs"])
    assert np.array_equal(_bits(got["rmse"][0]), _bits(np.float32(rmse)))
    assert np.array_equal(_bits(got["rmse"][0]), _bits(ref["rmse"]))
    assert np.array_equal(_bits(got["R"][0]), _bits(np.eye(3, dtype=np.float32)))          # the input's own bits
    assert np.array_equal(_bits(got["t"][0]), _bits(np.array([0, 0, 1], np.float32)))


def test_refiner_zero_radius_beside_a_sound_crop(dev):
    """radius = (0, 1) in one batch: crop 0 is DEGENERATE in pass 0 (a non-finite J), crop 1 is what it is alone."""
    a = lr.refine_args()
    both, alone = _refine(dev, a, B=2, radius=[0.0, 1.0]), _refine(dev, a)
    assert (dr.STATUS[int(both["status"][0])], int(both["passes"][0]), int(both["pairs"][0])) == ("DEGENERATE", 0, 561)
    assert np.array_equal(_bits(both["R"][0]), _bits(np.eye(3, dtype=np.float32)))
    assert np.array_equal(_bits(both["t"][0]), _bits(np.array([0, 0, 1], np.float32)))
    assert np.array_equal(_bits(both["rmse"][0]), _bits(np.float32(lr.GAP)))
    assert dr.STATUS[int(alone["status"][0])] != "DEGENERATE" and int(alone["passes"][0]) >= 1   # it did update
    for k in alone:
        assert np.array_equal(_bits(both[k][1]), _bits(alone[k][0])), k


def test_refiner_starved_after_an_update(dev):
    """The outputs of a stop in pass >= 1 are cast from the f64 state: STARVED with passes = 1 on bop_ref's tetra
    under a mask that keeps 126 pixels in pass 0 and 124 in pass 1, min_pairs = 125."""
    sc, ref = br.scene("tetra"), lr.starve_reference()
    got = refine_one(dev, sc, mask=lr.starve_mask(), min_pairs=lr.STARVE_MIN_PAIRS)
    refine_check("tetra, starved in pass 1", got, ref)
    assert (dr.STATUS[int(got["status"])], int(got["passes"]), int(got["pairs"])) == ("STARVED", 1, 124)
    assert not np.array_equal(_bits(got["R"]), _bits(np.asarray(sc["R_est"], np.float32)))


def test_refiner_max_iter_32_stops_where_10_does(dev):
    sc = br.scene("tetra")
    ten, most = refine_one(dev, sc, max_iter=10), refine_one(dev, sc, max_iter=32)
    refine_check("tetra, max_iter 32", most, dr.reference("tetra"))
    for k in ten:
        assert np.array_equal(_bits(ten[k]), _bits(most[k])), k


def test_refiner_poisoned_workspace_and_extents(dev):
    """The raw entry point on bop_ref's mixed batch with the workspace prefilled with 0xFF bytes (a set `final`
    flag, NaN state and slots) and with zeros: the six outputs are the same bits both times, written in full inside
    their guards, and equal the restatement as test_gpu_depth_refine.py compares them."""
    bt, crops, frames = br.mixed()
    B = len(crops)
    dia = np.array([c["diameter"] for c in crops])
    ins = [_t(bt["verts"], np.float32), _t(bt["faces"], np.int32), _t(bt["face_range"], np.int32),
           _t(np.stack([c["R_est"] for c in crops]).reshape(B, 9), np.float32),
           _t(np.stack([c["t_est"] for c in crops]), np.float32),
           _t(np.stack([c["K4"] for c in crops]), np.float32), _t(frames, np.float32), _t(np.arange(B), np.int32),
           _t(dr.DIST_FRAC * dia, np.float64), _t(dia / 2.0, np.float64)]
    v, f, fr, R0, t0, K, d, fi, md, rho = (x.to(dev) for x in ins)
    F, H, W = d.shape
    n_bytes = ctypes.c_longlong(0)
    _lib.call("krrn_pose_refine_depth_ws", B, H, W, ctypes.byref(n_bytes))
    runs = []
    for byte in (0xFF, 0):
        ws = Guarded(dev, (n_bytes.value,), torch.uint8)
        ws.view.fill_(byte)
        out = {"R": Guarded(dev, (B, 9), torch.float32), "t": Guarded(dev, (B, 3), torch.float32),
               "passes": Guarded(dev, (B,)), "pairs": Guarded(dev, (B,)), "rmse": Guarded(dev, (B,), torch.float32),
               "status": Guarded(dev, (B,))}
        assert ws.ptr % 8 == 0
        _lib.call("krrn_pose_refine_depth_f32", ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(fr), ptr(R0), ptr(t0), ptr(K),
                  ptr(d), P(0), F, H, W, ptr(fi), float(br.DEPTH_SCALE), ptr(md), ptr(rho), dr.MAX_ITER, dr.TOL,
                  dr.MIN_PAIRS, dr.DAMP, B, P(ws.ptr), P(out["R"].ptr), P(out["t"].ptr), P(out["passes"].ptr),
                  P(out["pairs"].ptr), P(out["rmse"].ptr), P(out["status"].ptr), stream_ptr(dev))
        torch.cuda.synchronize()
        ws.get()
        runs.append({k: g.get() for k, g in out.items()})
    for k in runs[0]:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), k
        assert not (runs[0][k] == -7777).any(), k            # every element written (guarded.SENTINELS)
    for b in range(B):
        got = {k: x[b].reshape(3, 3) if k == "R" else x[b] for k, x in runs[0].items()}
        refine_check(f"raw mixed[{b}]", got, dr.mixed_reference(b))


# ------------------------------------------------------------------------------------------- D: MSSD / MSPD

def _mssd(dev, verts, vert_range, cases, syms, sym_range):
    st = lambda k, dt: _t(np.stack([np.asarray(c[k], np.float64).reshape(-1) for c in cases]), dt)  # noqa: E731
    K4 = np.tile(np.asarray(rr.LM_K4, np.float32), (len(cases), 1))
    out = bop.mssd_mspd(_t(verts, np.float32).to(dev), _t(vert_range, np.int32), st("R_est", np.float64),
                        st("t_est", np.float64), st("R_gt", np.float64), st("t_gt", np.float64), _t(K4, np.float32),
                        _t(syms, np.float64), _t(sym_range, np.int32))
    torch.cuda.synchronize()
    return {k: x.cpu().numpy() for k, x in out.items()}


def _check_ms(tag, got, b, ref):
    m3, m2, i3, i2 = ref[:4]
    r3, r2 = abs(got["mssd"][b] - m3) / m3, abs(got["mspd"][b] - m2) / m2
    print(f"{tag}: mssd {got['mssd'][b]:.6e} (rel diff {r3:.1e}, sym {got['sym_idx'][b, 0]})  mspd {got['mspd'][b]:.6e} "
          f"(rel diff {r2:.1e}, sym {got['sym_idx'][b, 1]})")
    assert r3 <= MS_TOL and r2 <= MS_TOL, (tag, r3, r2)
    assert got["sym_idx"][b].tolist() == [i3, i2], (tag, got["sym_idx"][b].tolist(), i3, i2)


def test_mssd_mspd_slice_edges_ties_and_vertex_counts(dev):
    """One launch: NS = 15, 16, 17, 32, 33 (the arg-min in the last non-empty slice or in slice 0), the two exact
    ties across slices, and V = 1, 256, 257 cut out of the 642-vertex mesh through vert_range."""
    cases = lr.ms_cases()
    names = [f"ns{ns}" for ns in lr.MS_TARGET] + ["tie_low", "tie_zero", "v1", "v256", "v257"]
    small, big = lr.ms_mesh(), lr.ms_mesh(3)
    verts = np.concatenate([small, big])
    soff = np.cumsum([0] + [len(cases[n]["syms"]) for n in names])
    vr = [[len(small) + cases[n]["first"], len(cases[n]["verts"])] if "first" in cases[n] else [0, len(small)]
          for n in names]
    sr = [[int(soff[i]), len(cases[n]["syms"])] for i, n in enumerate(names)]
    got = _mssd(dev, verts, vr, [cases[n] for n in names], np.concatenate([cases[n]["syms"] for n in names]), sr)
    for b, n in enumerate(names):
        _check_ms(n, got, b, lr.ms_reference(cases[n]))
    idx = {n: got["sym_idx"][b].tolist() for b, n in enumerate(names)}
    for ns, k in lr.MS_TARGET.items():
        assert idx[f"ns{ns}"] == [k, k], ns
    assert idx["tie_low"] == [5, 5] and idx["tie_zero"] == [0, 0]


def test_mssd_mspd_bad_ranges_and_nan_in_one_batch(dev):
    """B = 6: an empty vertex range, an empty symmetry range, a vertex range cut at Vtot, a negative first vertex,
    a vertex set with one NaN vertex, and a sound crop whose result is what it is alone, bit for bit."""
    c = lr.ms_cases()["ns17"]
    mesh, syms = lr.ms_mesh(), c["syms"]
    bad = mesh[:8].copy()
    bad[3, 1] = np.nan
    verts = np.concatenate([bad, mesh])                      # Vtot = 170
    Vtot = len(verts)
    vr = [[8, 0], [8, 162], [Vtot - 10, 100], [-3, 4], [0, 8], [8, 162]]
    sr = [[0, 17], [5, 0], [0, 17], [0, 17], [0, 17], [0, 17]]
    got = _mssd(dev, verts, vr, [c] * 6, syms, sr)
    for b in (0, 1, 3, 4):
        assert np.isposinf(got["mssd"][b]) and np.isposinf(got["mspd"][b]) and got["sym_idx"][b].tolist() == [-1, -1], b
    nan_ref = lr.ms_reference(dict(c, verts=bad))
    assert np.isposinf(nan_ref[0]) and np.isposinf(nan_ref[1]) and nan_ref[2:4] == (-1, -1)
    _check_ms("cut at Vtot", got, 2, lr.ms_reference(dict(c, verts=mesh[-10:])))
    _check_ms("sound", got, 5, lr.ms_reference(c))
    alone = _mssd(dev, verts, vr[5:], [c], syms, sr[5:])
    for k in got:
        assert np.array_equal(_bits(got[k][5]), _bits(alone[k][0])), k
