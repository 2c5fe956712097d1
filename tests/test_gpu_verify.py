"""The pose-candidate score on the GPU (krrn_pose_score_f32 through verify.score_poses) against its numpy f64
restatement (tests/verify_ref.py).

The integer counts (render, claim, evid, both, inter, union) are compared exactly, which the restatement's margins
license (verify_ref.check_conditions: no undecided pixel in any case); score is one f64 division of those
integers, so bit equality is asserted; best is an index. Scenes (frame, faces, what it pins): tetra (480 x 640, 4),
layers (4: occlusion inside the mesh), degenerate (87: skipped faces), small (90 x 120, 320: partial tiles, the
object cut by two frame borders, a box that leaves the frame), empty_obs (320: an all-zero observed frame), gross
(80: a candidate that misses the mask), mixed (B = 5 over one concatenated mesh, one empty face range)."""
import numpy as np
import pytest
import torch

import bop_ref as br
import raster_ref as rr
import verify_ref as vr
from guarded import Guarded
from pose_estimation_amd import _lib, verify

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dt))


def _score(dev, verts, faces, face_range, cases, frames, masks, frame_idx, box=True, tau=vr.TAU):
    """verify.score_poses over `cases` (verify_ref case dicts: their candidates, K4, box); the rest as given."""
    out = verify.score_poses(
        _t(verts, np.float32).to(dev), _t(faces, np.int32).reshape(-1, 3).to(dev), _t(face_range, np.int32),
        _t(np.stack([c["Rs"] for c in cases]), np.float64), _t(np.stack([c["ts"] for c in cases]), np.float64),
        _t(np.stack([c["K4"] for c in cases]), np.float32), _t(frames, np.float32).to(dev), _t(frame_idx, np.int32),
        tau=tau, mask=None if masks is None else _t(masks, np.uint8).to(dev),
        box=_t(np.stack([c["box"] for c in cases]), np.int32) if box else None, depth_scale=br.DEPTH_SCALE)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _one(dev, case, frame_idx=0, face_range=None, mask=True, box=True, tau=vr.TAU):
    fr = [[0, len(case["faces"])]] if face_range is None else face_range
    got = _score(dev, case["verts"], case["faces"], fr, [case], case["depth"][None],
                 case["mask"][None] if mask else None, [frame_idx], box=box, tau=tau)
    return {k: v[0] for k, v in got.items()}


def _check(tag, got, ref, case=None):
    vr.check_conditions(ref)
    print(f"{tag}: counts {got['counts'].tolist()}  score {np.round(got['score'], 4).tolist()}  best {got['best']}  "
          f"bit-equal {np.array_equal(_bits(got['score']), _bits(ref['score']))}")
    assert np.array_equal(got["counts"], ref["counts"]), (tag, got["counts"].tolist(), ref["counts"].tolist())
    assert np.array_equal(_bits(got["score"]), _bits(ref["score"])), (tag, got["score"], ref["score"])
    assert int(got["best"]) == ref["best"], (tag, got["best"], ref["best"])
    if case is not None:                                         # the selected pose: candidate best's bits, as f32
        b = ref["best"]
        assert np.array_equal(_bits(got["R"]), _bits(case["Rs"][b].astype(np.float32))), tag
        assert np.array_equal(_bits(got["t"]), _bits(case["ts"][b].astype(np.float32))), tag


@pytest.mark.parametrize("name", vr.SCENES)
def test_scene_parity(dev, name):
    case, ref = vr.scene_case(name), vr.reference(name)
    vr.check_conditions(ref)
    _check(name, _one(dev, case), ref, case)


def _clean(case):
    """`case` with an unoccluded, hole-free observed frame (the GT render over the background plane) and mask =
    the GT silhouette."""
    sc = br.scene("tetra")
    d_gt, _ = br.depth_image(sc["verts"], sc["faces"], sc["R_gt"], sc["t_gt"], sc["K4"], sc["H"], sc["W"])
    obs = (np.where(d_gt > 0.0, d_gt, 1.5) * br.DEPTH_SCALE).astype(np.float32)
    sil = d_gt > 0.0
    mask = sil.astype(np.uint8)
    return dict(case, depth=obs, mask=mask, box=vr.square_box(mask, sc["H"], sc["W"])), int(sil.sum())


def test_known_answers(dev):
    base = vr.scene_case("tetra")
    clean, n_sil = _clean(base)
    R_gt, t_gt = base["Rs"][1], base["ts"][1]
    nan_R = np.full((3, 3), np.nan)
    off_t = t_gt + np.array([5.0, 0.0, 0.0])                     # five metres to the right: projected off the frame
    behind_t = t_gt * np.array([1.0, 1.0, -1.0])
    # the GT pose alone: the f32 observed depth moves |diff| by < 1e-7 m, far inside tau, so every silhouette
    # pixel is claimed, evident and an inlier
    got = _one(dev, dict(clean, Rs=R_gt[None], ts=t_gt[None]))
    c = got["counts"][0]
    assert c[0] == c[1] == c[2] == c[3] == c[4] == c[5] == n_sil > 0 and got["score"][0] == 1.0 and got["best"] == 0
    # off the frame, NaN, behind the camera: all zeros but the candidate-free evidence count; never best
    Rs = np.stack([R_gt, nan_R, R_gt, R_gt])
    ts = np.stack([off_t, t_gt, behind_t, t_gt])
    case = dict(clean, Rs=Rs, ts=ts)
    got = _one(dev, case)
    for k in range(3):
        assert got["counts"][k].tolist() == [0, 0, n_sil, 0, 0, n_sil] and got["score"][k] == 0.0, (k, got["counts"][k])
    assert got["best"] == 3 and got["score"][3] == 1.0
    assert np.array_equal(_bits(got["R"]), _bits(R_gt.astype(np.float32)))
    assert np.array_equal(_bits(got["t"]), _bits(t_gt.astype(np.float32)))
    _check("known", got, vr.case_score(case), case)
    # every candidate scores zero: best = 0, and the selected pose is candidate 0's bits (NaN included)
    case0 = dict(clean, Rs=Rs[[1, 0, 2]], ts=ts[[1, 0, 2]])
    got = _one(dev, case0)
    assert not got["score"].any() and got["best"] == 0
    assert np.array_equal(_bits(got["R"]), _bits(nan_R.astype(np.float32)))
    # without a mask, an off-frame candidate has no count at all
    got = _one(dev, dict(clean, Rs=R_gt[None], ts=off_t[None]), mask=False)
    assert not got["counts"].any() and got["score"][0] == 0.0 and got["best"] == 0
    # the same pose twice: the first wins the tie
    twice = dict(base, Rs=base["Rs"][[2, 1, 1]], ts=base["ts"][[2, 1, 1]])
    got = _one(dev, twice)
    assert np.array_equal(got["counts"][1], got["counts"][2]) and got["score"][1] == got["score"][2] > got["score"][0]
    assert got["best"] == 1
    _check("twice", got, vr.case_score(twice), twice)


def test_guards(dev):
    case = vr.scene_case("tetra")
    for fi in (-1, 1, 7):                                        # a frame index outside [0, F): nothing observed
        _check(f"frame {fi}", _one(dev, case, frame_idx=fi), vr.case_score(case, depth=None))
    for bad in ([[0, 0]], [[-1, 4]], [[0, -4]], [[5, 4]]):       # an empty or bad face range: only evidence
        got = _one(dev, case, face_range=bad)
        _check(f"range {bad}", got, vr.case_score(case, faces=case["faces"][:0]))
        assert not got["counts"][:, [0, 1, 3, 4]].any() and not got["score"].any() and got["best"] == 0
    _check("cut range", _one(dev, case, face_range=[[2, 100]]), vr.case_score(case, faces=case["faces"][2:]))
    got = _one(dev, case, mask=False)                            # mask NULL: no evidence, union == claim
    _check("no mask", got, vr.case_score(case, mask=None))
    assert not got["counts"][:, [2, 3, 4]].any() and np.array_equal(got["counts"][:, 5], got["counts"][:, 1])
    whole = dict(case, box=np.array([0, case["H"], 0, case["W"]], np.int32))
    a, b = _one(dev, case, box=False), _one(dev, whole)          # box NULL = a box covering the frame
    _check("no box", a, vr.case_score(case, box=None))
    assert all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)
    for box in ([10, 10, 0, 640], [300, 200, 0, 640], [-50, -1, 0, 640], [0, 480, 700, 900]):   # empty boxes
        got = _one(dev, dict(case, box=np.array(box, np.int32)))
        _check(f"box {box}", got, vr.case_score(case, box=box))
        assert not got["counts"][:, 2].any()
    per_tau = _one(dev, case, tau=torch.tensor([0.004], dtype=torch.float64))     # tau as a [B] tensor
    ref = vr.case_score(case, tau=0.004)
    vr.check_conditions(ref)
    _check("tau 4 mm", per_tau, ref)


def test_candidate_count_and_order(dev):
    """C = 1 and C = 8; a candidate's counts do not depend on C or on the other candidates; permuting the
    candidates permutes the counts and moves best accordingly."""
    case, ref = vr.scene_case("small"), vr.reference("small")
    full = _one(dev, case)
    for c in range(3):
        got = _one(dev, dict(case, Rs=case["Rs"][c:c + 1], ts=case["ts"][c:c + 1]))
        assert np.array_equal(got["counts"][0], full["counts"][c]) and got["best"] == 0, c
        assert np.array_equal(_bits(got["score"][0]), _bits(full["score"][c])), c
    order = [2, 0, 1, 1, 2, 0, 2, 1]                             # C = 8
    eight = dict(case, Rs=case["Rs"][order], ts=case["ts"][order])
    got = _one(dev, eight)
    assert np.array_equal(got["counts"], ref["counts"][order])
    assert np.array_equal(_bits(got["score"]), _bits(ref["score"][order]))
    assert got["best"] == order.index(ref["best"])
    for perm in ([1, 2, 0], [2, 1, 0]):
        p = _one(dev, dict(case, Rs=case["Rs"][perm], ts=case["ts"][perm]))
        assert np.array_equal(p["counts"], full["counts"][perm]) and p["best"] == perm.index(int(full["best"]))
        assert np.array_equal(_bits(p["R"]), _bits(full["R"])) and np.array_equal(_bits(p["t"]), _bits(full["t"]))
    v = torch.zeros((4, 3), device=dev)
    f = torch.zeros((1, 3), dtype=torch.int32, device=dev)
    for C in (0, 9):
        with pytest.raises(ValueError, match="candidates"):
            verify.score_poses(v, f, torch.tensor([[0, 1]]), torch.zeros((1, C, 3, 3)), torch.zeros((1, C, 3)),
                               torch.ones((1, 4)), torch.zeros((1, 16, 16), device=dev), torch.zeros(1))


def test_mixed_batch_invariance(dev):
    """Five crops over one concatenated mesh, C = 2, with per-crop frames, masks and boxes: each equals its own
    reference and its single-crop launch bit for bit, also with the batch permuted."""
    bt, cases, frames, masks = vr.mixed()
    B = rr.MIXED_B
    got = _score(dev, bt["verts"], bt["faces"], bt["face_range"], cases, frames, masks, list(range(B)))
    for b in range(B):
        ref = vr.mixed_reference(b)
        vr.check_conditions(ref)
        _check(f"mixed[{b}]", {k: v[b] for k, v in got.items()}, ref, cases[b])
        one = _score(dev, bt["verts"], bt["faces"], bt["face_range"][b:b + 1], [cases[b]], frames, masks, [b])
        assert all(np.array_equal(_bits(one[k][0]), _bits(got[k][b])) for k in got), b
    assert not got["counts"][3].any() and got["best"][3] == 0     # the crop with face count 0 (and an empty mask)
    perm = [3, 0, 4, 2, 1]
    p = _score(dev, bt["verts"], bt["faces"], bt["face_range"][perm], [cases[b] for b in perm], frames, masks, perm)
    assert all(np.array_equal(_bits(p[k]), _bits(got[k][perm])) for k in got)


def test_outputs_stay_inside_their_extents(dev):
    """The raw entry point writing into sentinel-guarded buffers (tests/guarded.py): B = 5, C = 3 on the mixed
    batch; every output is written in full and nothing beside it."""
    bt, cases, frames, masks = vr.mixed()
    B, C = rr.MIXED_B, 3
    Rs = np.stack([np.concatenate([c["Rs"], c["Rs"][:1]]) for c in cases])
    ts = np.stack([np.concatenate([c["ts"], c["ts"][:1]]) for c in cases])
    ins = [_t(bt["verts"], np.float32), _t(bt["faces"], np.int32), _t(bt["face_range"], np.int32), _t(Rs, np.float64),
           _t(ts, np.float64), _t(np.stack([c["K4"] for c in cases]), np.float32), _t(frames, np.float32),
           _t(masks, np.uint8), _t(np.arange(B), np.int32), _t(np.stack([c["box"] for c in cases]), np.int32),
           _t(np.full(B, vr.TAU), np.float64)]
    v, f, fr, R, t, K, d, m, fi, bx, tau = (x.to(dev) for x in ins)
    ws = Guarded(dev, (B, C, 4))
    counts = Guarded(dev, (B, C, 6))
    score = Guarded(dev, (B, C), torch.int64)                    # f64 bits in an int64 buffer
    best = Guarded(dev, (B,))
    Rsel, tsel = Guarded(dev, (B, 9), torch.float32), Guarded(dev, (B, 3), torch.float32)
    P = _lib.P
    F, H, W = d.shape
    _lib.call("krrn_pose_score_f32", _lib.ptr(v), v.shape[0], _lib.ptr(f), f.shape[0], _lib.ptr(fr), _lib.ptr(R),
              _lib.ptr(t), C, _lib.ptr(K), _lib.ptr(d), _lib.ptr(m), F, H, W, _lib.ptr(fi), _lib.ptr(bx),
              float(br.DEPTH_SCALE), _lib.ptr(tau), B, P(ws.ptr), P(counts.ptr), P(score.ptr), P(best.ptr), P(Rsel.ptr),
              P(tsel.ptr), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    got_c, got_s, got_b = counts.get(), score.get().view(np.float64), best.get()
    assert (ws.get() != ws.sentinel).all()
    for b in range(B):
        ref = vr.mixed_reference(b)
        assert np.array_equal(got_c[b, :2], ref["counts"]) and np.array_equal(got_c[b, 2], ref["counts"][0]), b
        assert np.array_equal(_bits(got_s[b, :2]), _bits(ref["score"])) and got_b[b] == ref["best"], b
        assert np.array_equal(_bits(Rsel.get()[b]), _bits(Rs[b, ref["best"]].reshape(9).astype(np.float32))), b
        assert np.array_equal(_bits(tsel.get()[b]), _bits(ts[b, ref["best"]].astype(np.float32))), b
