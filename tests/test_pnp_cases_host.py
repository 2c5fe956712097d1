"""tests/pnp_cases.py pinned on the CPU: the C oracle alone shows the condition every row of
PNP_EDGE_CASES is there for, so tests/test_gpu_pnp_edges.py cannot pass without meeting it. Letters (a)-(g)
are the conditions below; a row that stops showing its condition gets another seed, never a wider bound."""
import numpy as np
import pytest

import pnp_cases as pc
from oracle import pnp as opnp

G_BOUND = 2.5e-7  # (g): a quarter of the 1e-6 the GPU tests allow between kernel and oracle


def _rows():
    for c in pc.PNP_EDGE_CASES:
        crops, subsets = pc.build(c.id)
        for b, r in enumerate(pc.reference(c.id)):
            yield c, b, crops[b], subsets[b], r


def _scan(c, r):
    return pc.cv2_scan(r["hyp_cnt"], c.P, c.conf)


def test_table_covers_the_sizes():
    """The shapes the kernels branch on are all in the table."""
    Ps = {c.P for c in pc.PNP_EDGE_CASES}
    Hs = {c.H for c in pc.PNP_EDGE_CASES}
    assert {5, 6, 15, 16, 17, 63, 64, 65, 129, 1000, 1024} <= Ps
    assert {1, 2, 3, 5, 63, 65, 129, 130, 258, 4095} <= Hs and {h % 4 for h in Hs} == {0, 1, 2, 3}
    assert {c.conf for c in pc.PNP_EDGE_CASES} >= {0.0, 0.5, 1.0} and {c.thr for c in pc.PNP_EDGE_CASES} >= {0.25, 3.0}
    assert pc.CASES["p1024_h65_full_sel"].N == 1024 and pc.CASES["h4095_p64"].B == 1
    assert all(c.N == c.P + 13 for c in pc.PNP_EDGE_CASES if c.P != 1024)
    mixed = pc.CASES[pc.MIXED]
    assert mixed.B == 5 and [k[0] for k in mixed.kinds] == ["clean", "noisy", "planar", "pure_noise", "nonfinite"]


def test_crops_are_what_make_crop_promises():
    for c in pc.PNP_EDGE_CASES:
        crops, subsets = pc.build(c.id)
        assert subsets.dtype == np.int32 and subsets.min() >= 0 and subsets.max() < c.P
        if c.subsets == "random":
            assert all(len(set(row.tolist())) == 5 for row in subsets.reshape(-1, 5))
        for crop in crops:
            _, Hm, Wm = crop["xyz"].shape
            assert Hm != Wm and Hm * Wm >= c.N
            ch, sel = crop["choose"], crop["sel"]
            assert ch.shape == (c.N,) and len(set(ch.tolist())) == c.N and ch.min() == 0 and ch.max() == Hm * Wm - 1
            assert sel.shape == (c.P,) and len(set(sel.tolist())) == c.P and 0 <= sel.min() and sel.max() < c.N
            assert not np.array_equal(sel, np.arange(c.P))
            assert {0, Hm * Wm - 1} <= set(ch[sel].tolist())      # the map's first and last pixel are read
            assert np.abs(crop["K4"] / pc.K4_LINEMOD - 1).max() <= 0.1 + 1e-6
        # the crops of a batch differ in every per-crop parameter
        for a in range(c.B):
            for b in range(a + 1, c.B):
                assert not np.array_equal(crops[a]["K4"], crops[b]["K4"])
                if (b - a) % len(pc.OBJECTS):
                    assert not np.array_equal(crops[a]["extent"], crops[b]["extent"])
                    assert not np.array_equal(crops[a]["lfborder"], crops[b]["lfborder"])
    crops, _ = pc.build(pc.MIXED)
    assert len({tuple(cr["extent"]) for cr in crops}) == len(pc.OBJECTS)
    planar = pc.correspondences(crops[2])[0]
    assert np.ptp(planar[:, 2]) == 0 and np.ptp(planar[:, 0]) > 0
    for cr in crops[4:]:
        obj, img = pc.correspondences(cr)
        nf = cr["nonfinite"]
        assert np.isnan(obj[nf["nan"]]).any(axis=1).all() and np.isinf(img[nf["inf"]]).any(axis=1).all()
        assert np.isfinite(obj).all(axis=1).sum() == len(obj) - 2 and np.isfinite(img).all(axis=1).sum() == len(img) - 1


def test_oracle_is_deterministic_and_finite():
    for c, b, crop, subs, r in _rows():
        again = pc.oracle_crop(*pc.correspondences(crop), crop["K4"], subs, c.thr, c.conf)
        for k in r:
            assert np.array_equal(np.asarray(again[k]), np.asarray(r[k]), equal_nan=True), (c.id, b, k)
        assert np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all(), (c.id, b)
        assert r["cnt"] == (int(r["hyp_cnt"][r["best_h"]]) if r["best_h"] >= 0 else 0) == int(r["mask"].sum()), (c.id, b)
        assert _scan(c, r)[0] == r["best_h"], (c.id, b)


def test_a_stop_cuts_off_a_better_hypothesis():
    cut = [c.id for c, b, _, _, r in _rows() if 0 < r["cnt"] < r["hyp_cnt"].max()]
    assert "p1000_h101_cutoff" in cut, cut


def test_b_scan_crosses_chunks():
    def one(cid):
        c = pc.CASES[cid]
        r = pc.reference(cid)[0]
        return (c, r) + _scan(c, r)
    c, r, best, niters = one("scan_h129_stop_in_chunk1")
    assert 0 <= best < 64 < niters < c.H, (best, niters)
    c, r, best, niters = one("p1000_h101_cutoff")
    assert 0 <= best < 64 < niters < c.H, (best, niters)
    _, _, best, _ = one("scan_h130_best_in_chunk1")
    assert 64 <= best < 128, best
    _, _, best, _ = one("scan_h258_best_past_192")
    assert best >= 192, best
    _, _, best, niters = one("h4095_p64")
    assert best >= 1024 and niters > best, (best, niters)


@pytest.mark.parametrize("cid", ["tie_p6_h9", "tie_p16_h63"])
def test_c_ties_first_wins(cid):
    r = pc.reference(cid)[0]
    at = np.nonzero(r["hyp_cnt"] == r["cnt"])[0]
    assert r["cnt"] >= 5 and len(at) >= 2 and r["best_h"] == at[0], (r["cnt"], at, r["best_h"])


def test_d_selection_threshold_and_failures():
    r = pc.reference("max_count_exactly_4")[0]
    assert r["hyp_cnt"].max() == 4 and r["best_h"] == -1 and r["cnt"] == 0 and not r["mask"].any()
    assert np.array_equal(r["R"], np.eye(3, dtype=np.float32)) and not r["t"].any()
    r = pc.reference("max_count_exactly_5")[0]
    assert r["hyp_cnt"].max() == 5 and r["best_h"] >= 0 and r["cnt"] == 5
    r = pc.reference("conf0_p200_h50")[0]  # conf = 0: the first accepted hypothesis ends the loop
    assert r["best_h"] == np.nonzero(r["hyp_cnt"] >= 5)[0][0] and r["cnt"] < r["hyp_cnt"].max()
    c = pc.CASES["conf1_p200_h50"]
    r = pc.reference(c.id)[0]                 # conf = 1: never stops early
    assert _scan(c, r)[1] == c.H and r["cnt"] == r["hyp_cnt"].max()
    noise = [(c.id, b, r) for c, b, crop, _, r in _rows() if crop["kind"][0] == "pure_noise"]
    assert noise
    for cid, b, r in noise:
        assert r["best_h"] == -1 and r["cnt"] == 0, (cid, b)
    # thr is used: the same scene at 0.25 px and at 3 px
    assert pc.reference("thr025_p200_h50")[0]["cnt"] < pc.reference("thr3_p200_h50")[0]["cnt"]


def test_e_all_inlier_rows():
    seen = set()
    for c, b, crop, _, r in _rows():
        if crop["kind"][0] in ("clean", "planar"):
            assert r["cnt"] == c.P and r["mask"].all(), (c.id, b)
            seen.add(c.P)
    assert {5, 65, 129, 77} <= seen


def test_f_nonfinite_and_degenerate():
    seen = 0
    for c, b, crop, _, r in _rows():
        nf = crop["nonfinite"]["nan"] + crop["nonfinite"]["inf"]
        if nf:
            seen += 1
            assert len(nf) == 3 and not r["mask"][nf].any() and r["cnt"] >= 5, (c.id, b)
    assert seen == 2
    r = pc.reference("degenerate_p77")[0]
    assert (r["hyp_cnt"][pc.DEG_UNSOUND] < 5).all(), r["hyp_cnt"]
    assert r["cnt"] >= 5 and r["best_h"] not in pc.DEG_UNSOUND
    obj, img = pc.correspondences(pc.build("degenerate_p77")[0][0])
    line = obj[pc.DEG_COLLINEAR].astype(np.float64)
    assert np.linalg.svd(line - line.mean(0), compute_uv=False)[1] < 1e-8   # collinear to f32 rounding
    plane = obj[pc.DEG_COPLANAR].astype(np.float64)
    sv = np.linalg.svd(plane - plane.mean(0), compute_uv=False)
    assert sv[2] < 1e-8 < 1e-3 < sv[1]                                       # coplanar, not collinear
    a, b = pc.DEG_COINCIDENT
    assert np.array_equal(obj[a], obj[b]) and np.array_equal(img[a], img[b])


def test_g_conditioning():
    """The refit in the wave's summation order (pnp_ransac) and in sequential order (epnp on the masked
    points, f64) agree to G_BOUND on every crop that succeeds: the cases are well conditioned, so the
    GPU's 1e-6 bound against the oracle is a bound on errors, not on the scene."""
    worst = 0.0
    for c, b, crop, _, r in _rows():
        if r["best_h"] < 0:
            continue
        obj, img = pc.correspondences(crop)
        with np.errstate(invalid="ignore"):
            R2, t2, _ = opnp.epnp(obj[r["mask"]], img[r["mask"]], crop["K4"])
        g = max(float(np.abs(R2 - r["R"]).max()), float(np.abs(t2 - r["t"]).max()))
        assert g <= G_BOUND, (c.id, b, g)
        worst = max(worst, g)
    print(f"wave-order vs sequential refit: worst {worst:.2e}")
