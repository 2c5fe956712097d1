"""krrn_pnp_ransac_f32 at the size, selection and degenerate-input edges of tests/pnp_cases.py, against the C
oracle on the same correspondences and subsets: hypothesis counts equal count for count, the same selected
hypothesis, mask and inlier count, R / t within 1e-6 (the bound of test_full_ransac_matches_oracle), every
output written in full and nothing beside it (tests/guarded.py). tests/test_pnp_cases_host.py shows on the
CPU that each row meets the condition it is named for."""
import numpy as np
import pytest
import torch

import pnp_cases as pc
from guarded import Guarded
from pose_estimation_amd import _lib, pose

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-6
WORST = {"dR": 0.0, "dt": 0.0, "hyp": 0.0}  # over the tests run so far (printed by each)


def _launch(dev, crops, subsets, c, with_mask=True):
    """One launch on the crops' own buffers; every output a guarded view of exactly its extent."""
    B, P, N = len(crops), c.P, c.N
    H = subsets.shape[1]
    st = lambda k, dt: torch.from_numpy(np.ascontiguousarray(np.stack([cr[k] for cr in crops]), dt)).to(dev)  # noqa: E731
    xyz, choose, sel = st("xyz", np.float32), st("choose", np.int64), st("sel", np.int32)
    xm, ym, K4 = st("x_map", np.float32), st("y_map", np.float32), st("K4", np.float32)
    ext, lfb = st("extent", np.float64), st("lfborder", np.float64)
    sub = torch.from_numpy(np.ascontiguousarray(subsets, np.int32)).to(dev)
    assert choose.shape == (B, N) and sel.shape == (B, P) and sub.shape == (B, H, 5)
    assert int(sel.max()) < N and int(sub.max()) < P and int(choose.max()) < xyz.shape[2] * xyz.shape[3]  # in bounds
    ws = Guarded(dev, (B * H * 13,), torch.float32)
    R, t = Guarded(dev, (B, 9), torch.float32), Guarded(dev, (B, 3), torch.float32)
    inl, mask = Guarded(dev, (B,), torch.int32), Guarded(dev, (B, P), torch.uint8)
    ptr, Pp = _lib.ptr, _lib.P
    _lib.call("krrn_pnp_ransac_f32", ptr(xyz), xyz.shape[2] * xyz.shape[3], ptr(choose), N, ptr(sel), P, ptr(xm), ptr(ym),
              ptr(K4), ptr(ext), ptr(lfb), ptr(sub), H, float(c.thr), float(c.conf), Pp(ws.ptr), Pp(R.ptr), Pp(t.ptr),
              Pp(inl.ptr), Pp(mask.ptr if with_mask else 0), B, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    w = ws.get()
    out = dict(hyp_pose=w[:B * H * 12].reshape(B, H, 12), hyp_cnt=w[B * H * 12:].view(np.int32).reshape(B, H),
               R=R.get(), t=t.get(), inl=inl.get(), mask=mask.get())
    # written in full: no sentinel left (a NaN pose of a non-finite subset is a written value)
    assert (out["hyp_cnt"] != np.float32(ws.sentinel).view(np.int32)).all() and (out["hyp_pose"] != ws.sentinel).all()
    assert (out["R"] != R.sentinel).all() and (out["t"] != t.sentinel).all() and (out["inl"] != inl.sentinel).all()
    if with_mask:
        assert (out["mask"] != mask.sentinel).all()
    else:
        assert mask.untouched()
    return out


def _check_crop(tag, got, b, ref):
    """Crop b of a launch against its oracle_crop."""
    assert np.array_equal(got["hyp_cnt"][b], ref["hyp_cnt"]), (tag, np.nonzero(got["hyp_cnt"][b] != ref["hyp_cnt"])[0][:8])
    sel_able = ref["hyp_cnt"] >= 5  # the hypotheses that can be selected: their f32 pose decides the mask
    rp = np.concatenate([ref["hyp_R"].reshape(-1, 9), ref["hyp_t"]], 1)[sel_able]
    hyp = float((np.abs(got["hyp_pose"][b][sel_able] - rp) / np.maximum(1.0, np.abs(rp))).max()) if sel_able.any() else 0.0
    assert int(got["inl"][b]) == ref["cnt"], (tag, int(got["inl"][b]), ref["cnt"])
    assert np.array_equal(got["mask"][b].astype(bool), ref["mask"]) and got["mask"][b].max() <= 1, tag
    R, t = got["R"][b].reshape(3, 3), got["t"][b]
    if ref["best_h"] < 0:
        assert got["inl"][b] == 0 and not got["mask"][b].any(), tag
        assert np.array_equal(R, np.eye(3, dtype=np.float32)) and np.array_equal(t, np.zeros(3, np.float32)), tag
    dR, dt = float(np.abs(R - ref["R"]).max()), float(np.abs(t - ref["t"]).max())
    print(f"{tag}: count {ref['cnt']} at h = {ref['best_h']}, |dR| {dR:.2e} |dt| {dt:.2e}, hypothesis poses {hyp:.2e}")
    assert hyp <= POSE_TOL, (tag, hyp)
    assert dR <= POSE_TOL and dt <= POSE_TOL, (tag, dR, dt)
    for k, v in (("dR", dR), ("dt", dt), ("hyp", hyp)):
        WORST[k] = max(WORST[k], v)


@pytest.mark.parametrize("cid", [c.id for c in pc.PNP_EDGE_CASES])
def test_edge_case_matches_oracle(dev, cid):
    c = pc.CASES[cid]
    crops, subsets = pc.build(cid)
    ref = pc.reference(cid)
    got = _launch(dev, crops, subsets, c)
    for b in range(c.B):
        _check_crop(f"{cid}[{b}] {crops[b]['kind'][0]}", got, b, ref[b])
    print(f"worst so far: |dR| {WORST['dR']:.2e} |dt| {WORST['dt']:.2e} hypothesis poses {WORST['hyp']:.2e}")


def _bits(a):
    return torch.from_numpy(np.ascontiguousarray(a)).view(torch.int32 if a.dtype.itemsize == 4 else torch.uint8)


def test_mixed_batch_equals_single_crop_launches(dev):
    """Every per-crop table (K4, extent, lfborder, sel, choose, the maps, the subsets, the workspace) is indexed by
    the crop: the B = 5 launch and five B = 1 launches give the same bits."""
    c = pc.CASES[pc.MIXED]
    crops, subsets = pc.build(c.id)
    batched = _launch(dev, crops, subsets, c)
    for b in range(c.B):
        one = _launch(dev, crops[b:b + 1], subsets[b:b + 1], c)
        for k in ("R", "t", "inl", "mask", "hyp_cnt", "hyp_pose"):
            assert torch.equal(_bits(one[k][0]), _bits(batched[k][b])), (b, k)


def test_null_inlier_mask(dev):
    c = pc.CASES[pc.NULL_MASK]
    crops, subsets = pc.build(c.id)
    full = _launch(dev, crops, subsets, c)
    bare = _launch(dev, crops, subsets, c, with_mask=False)
    for k in ("R", "t", "inl", "hyp_cnt", "hyp_pose"):
        assert torch.equal(_bits(bare[k]), _bits(full[k])), k


def test_get_pose_fewer_points_than_num_points(dev):
    """The host path with N = 37 < NUM_POINTS: P = N, a drawn sel of all 37 slots, device-drawn subsets of five
    distinct indices below 37, and the oracle's result on exactly those."""
    B, N, H = 3, 37, pose.N_HYP
    crops = [pc.make_crop((pc.noisy(0.2, 0.3), N, N), 9000 + b) for b in range(B)]
    st = lambda k: torch.from_numpy(np.stack([cr[k] for cr in crops]))  # noqa: E731
    data = {"choose": st("choose").reshape(B, 1, N), "x_map_choosed": st("x_map").reshape(B, N, 1),
            "y_map_choosed": st("y_map").reshape(B, N, 1), "intrinsic": st("K4"), "extent": st("extent"),
            "lfborder": st("lfborder")}
    R, t, info = pose.get_pose({"xyz": st("xyz").to(dev)}, data, subsets=None, return_info=True)
    torch.cuda.synchronize()
    sel, subs = info["sel"].cpu().numpy(), info["subsets"].cpu().numpy()
    assert sel.shape == (B, N) and subs.shape == (B, H, 5)
    assert all(sorted(row.tolist()) == list(range(N)) for row in sel)
    assert subs.min() >= 0 and subs.max() < N and all(len(set(row.tolist())) == 5 for row in subs.reshape(-1, 5))
    w = info["workspace"].cpu().numpy()
    got = dict(hyp_pose=w[:B * H * 12].reshape(B, H, 12), hyp_cnt=w[B * H * 12:].view(np.int32).reshape(B, H),
               R=R.cpu().numpy().reshape(B, 9), t=t.cpu().numpy(), inl=info["inliers"].cpu().numpy(),
               mask=info["mask"].cpu().numpy())
    for b in range(B):
        obj, img = pc.correspondences(dict(crops[b], sel=sel[b]))
        ref = pc.oracle_crop(obj, img, crops[b]["K4"], subs[b], pose.THRESHOLD, pose.CONFIDENCE)
        assert ref["cnt"] >= 5, b
        _check_crop(f"get_pose N = 37 [{b}]", got, b, ref)
