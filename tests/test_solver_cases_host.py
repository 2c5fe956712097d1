"""The case tables of the 3D-3D solvers without a GPU: every row of tests/umeyama_cases.py and tests/icp_cases.py
shows, by the numpy restatements alone, the condition it is named for, and meets the restatement's
check_conditions (so that a bit-different f64 evaluation, the kernel's, must reach the same discrete decisions).

Two of check_conditions' limits are waived, each exactly where the comparison is decided without rounding:
  - the Umeyama stop margin |e - conf| (umeyama_ref.select): at conf = 1 the loop never stops, since
    e = 1 - (1 - r^5)^i <= 1 whatever the rounding; at i = 0 and while the best count is 0, e = 1 - 1 is exactly 0, never
    above a conf >= 0 (that is what makes the conf = 0 row stop at i = 1 and not at i = 0);
  - the ICP rejection margin |d^2 - max_dist^2| (icp_ref.icp): max_dist = 0 keeps nothing (d^2 < 0 never holds) and
    max_dist = +inf keeps every finite d^2.
The two ill-conditioned Umeyama hypotheses (umeyama_cases.ILL) are named in the table and left out of the margins;
nothing else is."""
import numpy as np
import pytest

import icp_cases as ic
import icp_ref as ir
import umeyama_cases as uc
import umeyama_ref as ur


# ---- umeyama_ref.select -------------------------------------------------------------------------------------------

def test_select_reports_failure_without_a_positive_count():
    """The kernel's best_h >= 0: no hypothesis with a positive count is a failure whatever min_ratio is."""
    for mr in (0.0, -1.0, 0.1):
        s = ur.select(np.zeros(7, np.int64), 50, 0.99, mr)
        assert s["failed"] and s["best_hyp"] == -1 and s["inliers"] == 0 and s["stop"] == 6
    s = ur.select(np.array([0, 0, 3, 3, 2]), 50, 1.0, 0.0)
    assert not s["failed"] and s["best_hyp"] == 2 and s["inliers"] == 3 and s["stop_margin"] == np.inf


def test_select_stop_margin_waivers():
    cnt = np.array([10, 30, 30, 45, 20])
    assert ur.select(cnt, 50, 1.0)["stop"] == 4 and ur.select(cnt, 50, 1.0)["stop_margin"] == np.inf
    s = ur.select(cnt, 50, 0.0)
    assert s["stop"] == 1 and 0.0 < s["stop_margin"] == 1 - (1 - 0.6 ** 5) ** 1
    s = ur.select(np.array([0, 0, 10, 0]), 50, 0.0)   # e stays exactly 0 until a count is positive
    assert s["stop"] == 2 and s["stop_margin"] == 1 - (1 - 0.2 ** 5) ** 2 > 0.0


def test_ransac_counts_a_non_finite_sample_zero():
    src, dst, _ = uc.synth(1, 40, out_frac=0.0)
    dst = dst.copy()
    dst[3, 0] = np.nan
    sub = np.array([[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]])
    r = ur.ransac(src, dst, sub)
    assert r["counts"][0] == 0 and r["counts"][1] == 39 and not r["margins"]["finite"] and not r["mask"][3]


# ---- krrn_umeyama_ransac_f32 rows ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", [c.id for c in uc.UMEYAMA_EDGE_CASES])
def test_umeyama_row_meets_conditions(cid):
    c, d = uc.CASES[cid], uc.build(cid)
    for b, r in enumerate(uc.reference(cid)):
        print(cid, b, "best", r["best_hyp"], "inliers", r["inliers"], "stop", r["stop"], r["margins"])
        ur.check_conditions(r, allow_degenerate=c.allow)
        assert c.allow or r["margins"]["finite"]
    assert d["src"].dtype == np.float32 and d["dst"].dtype == np.float32 and d["subsets"].dtype == np.int32
    if "clamped" not in d:
        assert d["subsets"].min() >= 0 and d["subsets"].max() < c.N  # every index a row passes is in range


def _one(cid):
    return uc.CASES[cid], uc.build(cid), uc.reference(cid)[0]


def test_umeyama_size_rows():
    want = uc.SIZES + [(4096, 8192)]
    got = [(c.N, c.H) for c in uc.UMEYAMA_EDGE_CASES[:len(want)]]
    assert got == want
    for N, H in want[:-1]:
        c, d, r = _one(f"n{N}_h{H}")
        assert not r["failed"] and (d["conf"], d["min_ratio"], d["inlier_frac"]) == (0.99, 0.1, 0.1)
    assert _one("n5_h1")[2]["inliers"] == 5
    # ragged 16-hypothesis waves and 64-hypothesis blocks on either side
    assert {H % 16 for _, H in want} >= {0, 1, 15} and {H % 64 for _, H in want} >= {0, 1, 63}
    c, d, r = _one(uc.BIG)
    assert d["conf"] == 1.0 and r["stop"] == c.H - 1 and r["best_hyp"] == uc.BIG_BEST and not r["failed"]
    assert (r["counts"][:uc.BIG_BEST] < r["inliers"]).all()  # only a scan that reads that far finds it


def test_umeyama_selection_rows():
    _, d0, r0 = _one("sel_conf0_stops_at_1_and_fails")
    assert r0["stop"] == 1 and r0["failed"] and (0 < r0["counts"][:2]).all() and (r0["counts"][:2] < 0.1 * uc.SEL_N).all()
    _, _, r05 = _one("sel_conf05")
    _, _, r99 = _one("sel_conf099_better_after_stop")
    c, _, r1 = _one("sel_conf1_finds_the_late_best")
    assert np.array_equal(r0["counts"], r1["counts"]) and np.array_equal(r05["counts"], r99["counts"])  # one scene
    assert 1 < r05["stop"] < r99["stop"] < uc.SEL_LATE and not r05["failed"] and not r99["failed"]
    assert r05["best_hyp"] <= r05["stop"] and r05["best_hyp"] < r99["best_hyp"] <= r99["stop"]
    assert r1["stop"] == c.H - 1 and r1["best_hyp"] == uc.SEL_LATE
    # the better hypothesis lies after the stop and does not win
    assert r99["counts"][uc.SEL_LATE] > r99["inliers"] == r99["counts"][:r99["stop"] + 1].max()
    c, d, rt = _one("sel_tie_lower_index_wins")
    tie = c.args["tie"]
    assert np.array_equal(d["subsets"][0, tie], d["subsets"][0, uc.SEL_LATE]) and rt["best_hyp"] == tie
    assert rt["counts"][tie] == rt["counts"][uc.SEL_LATE] == rt["counts"].max() and rt["stop"] == c.H - 1
    for i in uc.STOPS:
        _, d, r = _one(f"stop_at_{i}")
        assert r["stop"] == i and 0.99 < d["conf"] < 1.0 and not r["failed"]


def test_umeyama_parameter_rows():
    _, d, r = _one("min_ratio_equal_best")
    _, d2, r2 = _one("min_ratio_next_above_best")
    assert d["min_ratio"] == r["inliers"] / 257 and not r["failed"]
    assert d2["min_ratio"] == np.nextafter(d["min_ratio"], 2.0) and r2["failed"] and r2["counts"].max() == r["inliers"]
    _, d, r = _one("min_ratio_0_all_counts_0")
    assert d["min_ratio"] == 0.0 and not r["counts"].any() and r["failed"] and r["best_hyp"] == -1 and r["inliers"] == 0
    assert r["scale"] == 1.0 and np.array_equal(r["R"], np.eye(3)) and not r["t"].any() and not r["mask"].any()
    assert all(len(set(row)) == 1 for row in d["subsets"][0].tolist())
    base = _one("n257_h65")[2]
    for cid, frac in (("inlier_frac_005", 0.05), ("inlier_frac_03", 0.3)):
        _, d, r = _one(cid)
        assert d["inlier_frac"] == frac and not r["failed"]
        assert not np.array_equal(r["counts"], base["counts"])  # the same scene at 0.1 counts differently


def test_umeyama_input_rows():
    c, d, r = _one(uc.INDICES)
    raw, cl = d["subsets"][0].astype(np.int64), d["clamped"][0]
    assert sorted(raw[(raw < 0) | (raw >= c.N)].tolist()) == sorted([-1, c.N, uc.INT_MAX, uc.INT_MIN] * 2)
    assert cl.min() == 0 and cl.max() == c.N - 1 and np.array_equal(cl, np.clip(raw, 0, c.N - 1))
    assert r["stop"] > 4 and not r["failed"]  # the five rows with such indices are inside the scan
    c, d, r = _one("five_identical_indices")
    assert len(set(d["subsets"][0, 3].tolist())) == 1 and r["counts"][3] == 0 and not r["failed"]
    c, d, r = _one("src_nan_fails")
    assert np.isnan(d["src"]).sum() == 1 and not r["counts"].any() and r["failed"]
    c, d, r = _one("dst_nan_inf_point")
    p = uc.NONFINITE_POINT
    assert np.isnan(d["dst"][0, p, 0]) and np.isinf(d["dst"][0, p, 1])
    holds = (d["subsets"][0] == p).any(1)
    assert sorted(np.nonzero(holds)[0].tolist()) == sorted(uc.DST_ROWS_HOLDING) and not r["counts"][holds].any()
    far = d["dst"][0].copy()
    far[p] = uc.FAR
    rf = ur.ransac(d["src"][0], far, d["subsets"][0])
    assert np.array_equal(r["counts"][~holds], rf["counts"][~holds]) and (r["counts"][~holds] > 0).mean() > 0.8
    assert min(uc.DST_ROWS_HOLDING) <= r["stop"] and not r["failed"] and not r["mask"][p]
    c, d, r = _one("planar_object")
    assert np.ptp(d["src"][0, :, 2]) == 0.0 and not r["failed"]
    c, d, refs = uc.CASES[uc.BATCH], uc.build(uc.BATCH), uc.reference(uc.BATCH)
    assert d["src"].shape[0] == 3 and [x["failed"] for x in refs] == [False, True, False]
    assert np.isnan(d["src"][1]).any() and np.isfinite(d["src"][[0, 2]]).all()


def test_umeyama_ill_rows_are_the_only_exemption():
    c, d, r = _one(uc.ILL)
    assert len(c.ill) == 2 and sum(len(x.ill) for x in uc.UMEYAMA_EDGE_CASES) == 2
    for h in c.ill:
        assert len(set(d["subsets"][0, h].tolist())) == 2
        assert h <= r["stop"]  # inside the scan: their counts take part in the kernel's selection
    strict = ur.ransac(d["src"][0], d["dst"][0], d["subsets"][0])  # without the exemption the row is refused
    with pytest.raises(AssertionError):
        ur.check_conditions(strict)
    assert r["best_hyp"] not in c.ill and r["inliers"] > 0.5 * c.N


@pytest.mark.parametrize("B,N", uc.MODEL_POINT_ROWS)
def test_model_point_rows(B, N):
    m = uc.model_points_case(B, N)
    assert sorted({b * n for b, n in uc.MODEL_POINT_ROWS}) == [1, 255, 256, 257]
    nan = np.isnan(m["out"])
    assert np.array_equal(nan.all(2), m["outside"]) and np.array_equal(nan.any(2), m["outside"])
    ch = set(m["choose"].ravel().tolist())
    assert uc.MP_HW - 1 in ch and (N < 5 or {0, uc.MP_HW, -1, 2 ** 40} <= ch)
    assert B == 1 or not np.array_equal(m["extent"][0], m["extent"][1])


# ---- krrn_icp_refine_f32 rows -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", [c.id for c in ic.ICP_EDGE_CASES])
def test_icp_row_meets_conditions(cid):
    c, r = ic.CASES[cid], ic.reference(cid)
    print(cid, "status", r["status"], "passes", r["passes"], "pairs", r["pairs"], r["margins"])
    ir.check_conditions(r)
    for k, v in c.expect.items():
        assert r[k] == v, (k, r[k], v)
    sc = ic.build(cid)
    assert sc["cloud"].shape == (c.N, 3) and sc["model"].shape == (c.M, 3)


def test_icp_slot_rows_cover_every_switch_case():
    Ns = [ic.CASES[i].N for i in ic.SLOT_ROWS]
    assert Ns == [3, 511, 512, 513, 1024, 1025, 1537, 2049, 2561, 3073, 3585, 4096]
    assert sorted({-(-n // 512) for n in Ns}) == [1, 2, 3, 4, 5, 6, 7, 8]
    assert all(ic.CASES[i].seed == 7000 + ic.CASES[i].N and ic.CASES[i].M == 67 for i in ic.SLOT_ROWS)
    for i in ic.SLOT_ROWS:  # the last slot holds kept pairs: dropping it changes the result
        r = ic.reference(i)
        last = (ic.CASES[i].N - 1) // 512 * 512
        assert (r["nn_idx"][last:] >= 0).any() and r["status"] == ir.CONVERGED
    assert -(-ic.CASES[ic.NULL_NN].N // 512) == 2
    tails = ("m1_degenerate", "m2_score_only", "m3", "m4", "m5")
    assert [ic.CASES[i].M for i in tails] == [1, 2, 3, 4, 5] and all(ic.CASES[i].N == 64 for i in tails)


def test_icp_stop_rows():
    sc, r = ic.build("starved_after_update"), ic.reference("starved_after_update")
    assert (r["nn_prev"] >= 0).sum() == 52 and r["pairs"] == 50  # 52 pairs in pass 0, 50 in pass 1
    assert np.abs(r["R"] - sc["R0"]).max() > 1e-4  # the pose handed back is the updated one
    assert ic.reference("min_pairs_51")["passes"] == 2 and ic.reference("min_pairs_50_continues")["passes"] == 3
    r = ic.reference("tol0_fixed_point")
    assert 2 < r["passes"] < 65 and np.array_equal(r["nn_idx"], r["nn_prev"])  # the last two pair sets are equal
    assert r["margins"]["conv_gap"] == np.inf  # tol 0: no margin to keep, the stop is err == err_prev exactly
    for cid in ("m1_degenerate", "degenerate_identical_cloud", "degenerate_x_axis"):
        sc, r = ic.build(cid), ic.reference(cid)
        assert r["status"] == ir.DEGENERATE and r["passes"] == 1 and r["pairs"] >= ir.MIN_PAIRS and np.isfinite(r["rmse"])
        assert np.array_equal(r["R"], sc["R0"].astype(np.float64)) and np.array_equal(r["t"], sc["t0"].astype(np.float64))
        assert (r["nn_idx"] >= 0).sum() == r["pairs"]
    sc, r = ic.build("degenerate_after_update"), ic.reference("degenerate_after_update")
    assert (r["nn_prev"] >= 0).sum() == ic.CLUSTER_A + ic.CLUSTER_B and (r["nn_idx"][:ic.CLUSTER_A] == -1).all()
    assert (r["nn_idx"][ic.CLUSTER_A:] == 0).all() and (sc["cloud"][ic.CLUSTER_A:] == sc["cloud"][ic.CLUSTER_A]).all()
    assert np.abs(r["R"] - sc["R0"]).max() > 1e-2 and np.isfinite(r["R"]).all()  # the pose of the one update that worked
    sc = ic.build("degenerate_identical_cloud")
    assert (sc["cloud"] == sc["cloud"][0]).all()
    sc = ic.build("degenerate_x_axis")
    assert not sc["cloud"][:, 1:].any() and not sc["model"][:, 1:].any() and np.array_equal(sc["R0"], np.eye(3))


def test_icp_input_rows():
    sc, r = ic.build("cloud_nan_inf"), ic.reference("cloud_nan_inf")
    bad = [ic.CLOUD_NAN, ic.CLOUD_INF, ic.CLOUD_NINF]
    assert (~np.isfinite(sc["cloud"])).any(1).nonzero()[0].tolist() == bad
    assert (r["nn_idx"][bad] == -1).all() and r["pairs"] == 257 - 3 and r["status"] == ir.CONVERGED
    sc, r = ic.build("model_nan"), ic.reference("model_nan")
    assert np.isnan(sc["model"][ic.MODEL_NAN, 0]) and not (r["nn_idx"] == ic.MODEL_NAN).any()
    without = np.delete(sc["model"], ic.MODEL_NAN, axis=0)
    w = ir.icp(sc["R0"], sc["t0"], sc["cloud"], without, sc["max_dist"])
    shifted = np.where(r["nn_idx"] > ic.MODEL_NAN, r["nn_idx"] - 1, r["nn_idx"])
    assert np.array_equal(shifted, w["nn_idx"]) and np.array_equal(r["R"], w["R"]) and r["passes"] == w["passes"]
    sc, r = ic.build("max_dist_inf"), ic.reference("max_dist_inf")
    assert sc["max_dist"] == np.inf and r["pairs"] == 300 and (r["nn_idx"] >= 0).all() and r["rmse"] > 0.02
    sc, r = ic.build("max_dist_0"), ic.reference("max_dist_0")
    assert r["rmse"] == np.inf and (r["nn_idx"] == -1).all()
    assert np.array_equal(r["R"], sc["R0"].astype(np.float64)) and np.array_equal(r["t"], sc["t0"].astype(np.float64))


def test_icp_batch_shows_all_four_statuses():
    scs, md, refs = ic.batch()
    for r in refs:
        ir.check_conditions(r)
    assert len(refs) == 6 and {r["status"] for r in refs} == {ir.CONVERGED, ir.MAX_ITER_HIT, ir.STARVED, ir.DEGENERATE}
    assert len(set(md.tolist())) == 3


def test_nearest_never_picks_a_nan_distance():
    Q = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [1.0, 1.0, 1.0]])
    Mo = np.array([[np.nan, 0.0, 0.0], [0.5, 0.0, 0.0], [1.0, 1.0, 0.9]])
    j, d2, _ = ir.nearest(Q, Mo)
    assert j.tolist()[0] == 1 and j.tolist()[2] == 2 and d2[0] == 0.25 and d2[1] == np.inf
