"""krrn_umeyama_ransac_f32 and krrn_model_points_f32 at the size, selection and degenerate-input edges of
tests/umeyama_cases.py, through the raw entry points with their inlier_frac / conf / min_ratio arguments and their
optional outputs, against the numpy restatement (tests/umeyama_ref.py) on the same points and subsets: every
hypothesis's count, the selected hypothesis, the inlier count and the mask equal; scale / R / t within 1e-6 (the f32
output format's bound, tests/test_gpu_umeyama.py's TOL); every output written in full and nothing beside it
(tests/guarded.py). tests/test_solver_cases_host.py shows on the CPU that each row meets the condition it is named
for and the margins that license the exact comparisons.

Worst differences observed on an MI355X over all rows: |ds| 5.91e-08, |dR| 2.91e-08, |dt| 4.29e-08."""
import numpy as np
import pytest
import torch

import umeyama_cases as uc
import umeyama_ref as ur
from guarded import Guarded
from pose_estimation_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 1e-6
WORST = {"ds": 0.0, "dR": 0.0, "dt": 0.0}  # over the tests run so far (printed by each)
OUTS = ("counts", "scale", "R", "t", "inliers", "best_hyp", "mask")


def _launch(dev, d, crops=None, subsets=None, with_best=True, with_mask=True):
    """One launch on crops `crops` (a slice; all of them by default) of a built row; every output a guarded view of
    exactly its extent."""
    sl = crops or slice(None)
    up = lambda a: torch.from_numpy(np.array(a[sl])).to(dev)  # noqa: E731  (a copy: the built rows are read-only)
    src, dst, sub = up(d["src"]), up(d["dst"]), up(d["subsets"] if subsets is None else subsets)
    B, N, _ = src.shape
    H = sub.shape[1]
    assert dst.shape == (B, N, 3) and sub.shape == (B, H, 5) and sub.dtype == torch.int32
    g = dict(counts=Guarded(dev, (B, H)), scale=Guarded(dev, (B,), torch.float32), R=Guarded(dev, (B, 9), torch.float32),
             t=Guarded(dev, (B, 3), torch.float32), inliers=Guarded(dev, (B,)), best_hyp=Guarded(dev, (B,)),
             mask=Guarded(dev, (B, N), torch.uint8))
    ptr, P = _lib.ptr, _lib.P
    _lib.call("krrn_umeyama_ransac_f32", ptr(src), ptr(dst), N, ptr(sub), H, d["inlier_frac"], d["conf"], d["min_ratio"],
              P(g["counts"].ptr), P(g["scale"].ptr), P(g["R"].ptr), P(g["t"].ptr), P(g["inliers"].ptr),
              P(g["best_hyp"].ptr if with_best else 0), P(g["mask"].ptr if with_mask else 0), B, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    out = {k: v.get() for k, v in g.items()}  # (both guards of every buffer checked)
    for k in OUTS:
        if (k == "best_hyp" and not with_best) or (k == "mask" and not with_mask):
            assert g[k].untouched(), k
        else:
            assert (out[k] != g[k].sentinel).all(), f"{k} not written in full"
    return out


def _check_crop(tag, got, b, ref, c, d):
    N = c.N
    cnt = got["counts"][b]
    sound = np.ones(c.H, bool)
    sound[list(c.ill)] = False
    assert np.array_equal(cnt[sound], ref["counts"][sound]), (tag, np.nonzero(cnt != ref["counts"])[0][:8])
    assert (cnt >= 0).all() and (cnt <= N).all(), tag
    # the selection on the counts the kernel itself scored (all of them the restatement's, but for the ill rows)
    sel = ur.select(cnt, N, d["conf"], d["min_ratio"])
    assert int(got["best_hyp"][b]) == sel["best_hyp"] and int(got["inliers"][b]) == sel["inliers"], (tag, sel)
    assert sel["best_hyp"] == ref["best_hyp"] and sel["inliers"] == ref["inliers"], (tag, sel, ref["best_hyp"])
    assert np.array_equal(got["mask"][b].astype(bool), ref["mask"]) and got["mask"][b].max() <= 1, tag
    assert int(got["mask"][b].sum()) == ref["inliers"], tag
    s, R, t = float(got["scale"][b]), got["R"][b].reshape(3, 3), got["t"][b]
    if ref["failed"]:
        assert s == 1.0 and np.array_equal(R, np.eye(3, dtype=np.float32)) and not t.any(), tag
        assert got["best_hyp"][b] == -1 and got["inliers"][b] == 0 and not got["mask"][b].any(), tag
    ds, dR, dt = abs(s - ref["scale"]), float(np.abs(R - ref["R"]).max()), float(np.abs(t - ref["t"]).max())
    print(f"{tag}: best {ref['best_hyp']} of {c.H} (stop {ref['stop']}), {ref['inliers']} / {N} inliers, "
          f"|ds| {ds:.2e} |dR| {dR:.2e} |dt| {dt:.2e}")
    assert ds <= TOL and dR <= TOL and dt <= TOL, (tag, ds, dR, dt)
    for k, v in (("ds", ds), ("dR", dR), ("dt", dt)):
        WORST[k] = max(WORST[k], v)


@pytest.mark.parametrize("cid", [c.id for c in uc.UMEYAMA_EDGE_CASES])
def test_edge_case_matches_restatement(dev, cid):
    c, d, refs = uc.CASES[cid], uc.build(cid), uc.reference(cid)
    got = _launch(dev, d)
    for b, ref in enumerate(refs):
        _check_crop(f"{cid}[{b}]", got, b, ref, c, d)
    print(f"worst so far: |ds| {WORST['ds']:.2e} |dR| {WORST['dR']:.2e} |dt| {WORST['dt']:.2e}")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_indices_outside_the_crop_are_clamped(dev):
    """-1, N, 2^31 - 1 and -2^31 give the outputs of the clamped subsets bit for bit (the kernel's documented clamp: no
    index leaves the crop)."""
    d = uc.build(uc.INDICES)
    raw, clamped = _launch(dev, d), _launch(dev, d, subsets=d["clamped"])
    for k in OUTS:
        assert np.array_equal(_bits(raw[k]), _bits(clamped[k])), k


def test_optional_outputs(dev):
    """best_hyp null, inlier_mask null, both null: every other output bit-equal to the full call's, the omitted buffer
    untouched (asserted in _launch)."""
    d = uc.build(uc.OPTIONAL)
    full = _launch(dev, d)
    for with_best, with_mask in ((False, True), (True, False), (False, False)):
        part = _launch(dev, d, with_best=with_best, with_mask=with_mask)
        for k in OUTS:
            if (k == "best_hyp" and not with_best) or (k == "mask" and not with_mask):
                continue
            assert np.array_equal(_bits(part[k]), _bits(full[k])), (with_best, with_mask, k)
    # and on a failing crop (the branch that writes the mask's zeros and best_hyp = -1)
    d = uc.build("min_ratio_next_above_best")
    full, bare = _launch(dev, d), _launch(dev, d, with_best=False, with_mask=False)
    assert full["best_hyp"][0] == -1 and not full["mask"].any()
    for k in ("counts", "scale", "R", "t", "inliers"):
        assert np.array_equal(_bits(bare[k]), _bits(full[k])), k


def test_batch_with_a_nan_crop_equals_single_launches(dev):
    d = uc.build(uc.BATCH)
    batched = _launch(dev, d)
    assert batched["inliers"][1] == 0 and batched["inliers"][0] > 0 and batched["inliers"][2] > 0
    for b in range(3):
        one = _launch(dev, d, crops=slice(b, b + 1))
        for k in OUTS:
            assert np.array_equal(_bits(one[k][0]), _bits(batched[k][b])), (b, k)


@pytest.mark.parametrize("B,N", uc.MODEL_POINT_ROWS)
def test_model_points(dev, B, N):
    """B N around the 256-thread block; pixels 0, HW - 1 (read) and HW, -1, 2^40 (never read: NaN); a crop's own
    extent and lfborder. Bit-equal to the torch f64 -> f32 expression."""
    m = uc.model_points_case(B, N)
    xyz, choose = torch.from_numpy(m["xyz"]), torch.from_numpy(m["choose"])
    ext, lfb = torch.from_numpy(m["extent"]), torch.from_numpy(m["lfborder"])
    inside = torch.from_numpy(~m["outside"])
    pix = torch.where(inside, choose, torch.zeros_like(choose))
    val = torch.gather(xyz, 2, pix.reshape(B, 1, N).expand(B, 3, N)).transpose(1, 2)
    want = (val.double() * ext.reshape(B, 1, 3) + lfb.reshape(B, 1, 3)).float()
    want[~inside] = float("nan")
    assert np.array_equal(want.numpy(), m["out"], equal_nan=True)
    out = Guarded(dev, (B, N, 3), torch.float32)
    dv = [a.to(dev) for a in (xyz, choose, ext, lfb)]
    _lib.call("krrn_model_points_f32", _lib.ptr(dv[0]), uc.MP_HW, _lib.ptr(dv[1]), N, _lib.ptr(dv[2]), _lib.ptr(dv[3]),
              _lib.P(out.ptr), B, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    got = out.get()
    assert (got != out.sentinel).all()
    assert np.array_equal(np.isnan(got).all(2), m["outside"]) and np.array_equal(np.isnan(got).any(2), m["outside"])
    ok = ~m["outside"]
    assert np.array_equal(got[ok].view(np.uint32), m["out"][ok].view(np.uint32))
