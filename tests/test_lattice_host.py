"""The lattice scenes of tests/lattice_ref.py on the restatements alone. No GPU.

Two kinds of assertion. Exactness: the projections are integers, the depths exactly 0.5 / 1 / 2, the counts and
boxes the ones worked out by hand, so the cases really sit on the tile edges and thresholds they are meant to
sit on. Discriminators: for every rule that tests/test_gpu_render_edges.py pins, the expected answer changes when
the rule is broken (another visiting order of the face list, a threshold moved by one np.nextafter step, the
highest index on ties), so a kernel that broke the rule would fail the GPU case."""
import numpy as np
import pytest

import bop_ref as br
import depth_refine_ref as dr
import lattice_ref as lr
import raster_ref as rr

UP, DOWN = np.inf, -np.inf


def _step(x, to):
    return float(np.nextafter(np.float64(x), to))


# ------------------------------------------------------------------------------------------------ the plane

@pytest.mark.parametrize("pose", sorted(lr.POSES))
def test_plane_projects_to_integer_pixels_and_exact_depth(pose):
    v, _ = lr.plane()
    t = lr.t_of(pose)
    c = v.astype(np.float64) + t
    u, w = 512.0 * c[:, 0] / c[:, 2] + 24.0, 512.0 * c[:, 1] / c[:, 2] + 24.0
    assert np.array_equal(u, np.round(u)) and np.array_equal(w, np.round(w))
    n, x0, x1, y0, y1, z = lr.COVER[pose]
    # the projected box before the frame cuts it: floor / ceil of these are the values themselves
    full = {"z1": (16, 48, 16, 32), "z2": (20, 36, 20, 28), "near": (8, 72, 8, 40), "shift": (32, 64, 16, 32)}[pose]
    assert (u.min(), u.max(), w.min(), w.max()) == full
    d = lr.plane_depth(pose)
    ys, xs = np.nonzero(d > 0.0)
    assert len(ys) == n and (xs.min(), xs.max(), ys.min(), ys.max()) == (x0, x1, y0, y1)
    assert n == (x1 - x0 + 1) * (y1 - y0 + 1)                # a full rectangle
    assert (d[d > 0.0] == z).all()


def test_frame_and_tile_geometry():
    assert (lr.H, lr.W) == (40, 56) and lr.H % 16 == 8 and lr.W % 16 == 8       # 2.5 x 3.5 tiles
    n, x0, x1, y0, y1, _ = lr.COVER["z1"]
    assert x0 % 16 == 0 and x0 - 1 == 15     # tile column 0 ends at 15: culled by `box lo <= tile hi` at 16 > 15 only
    assert x1 == 48 and x1 % 16 == 0 and x1 + 8 == lr.W      # column 48: the first sample of the 8-wide partial tile
    assert y0 % 16 == 0 and y1 % 16 == 0                     # rows 16 and 32: first samples of tile rows 1 and 2
    ray = lr.ray_image()
    assert ray[lr.PX[1], lr.PX[0]] == 1.0
    others = np.sort(ray.reshape(-1))[1]
    assert others > 1.0 and 4.7e-7 < others * 0.25 - 0.25 < 4.9e-7 and others * 0.25 - 0.25 > 100 * rr.MARGIN


# ------------------------------------------------------------------------------------------------ A

def test_ties_spread_expected_map_and_order_discriminators():
    sc = lr.ties_spread()
    F = len(sc["faces"])
    assert F == 640 and len(set(lr.TIES_ORIG)) == 32
    for edge in (64, 128, 192, 256, 320, 384, 448, 512, 576):           # both sides of every wave / chunk boundary
        assert edge - 1 in lr.TIES_ORIG and edge in lr.TIES_ORIG, edge
    ref = lr.render_scene(sc)
    cov = ref["cover"]
    assert int(cov.sum()) == 1089 and (ref["depth"][cov] == 1.0).all()
    assert np.isin(ref["face"][cov], sc["orig"]).all() and len(np.unique(ref["face"][cov])) == 32
    # the survivors of the cull are the 64 cell faces and their duplicates: sparse among 576 culled faces
    u = 512.0 * sc["verts"][sc["faces"]][..., 0].astype(np.float64) + 64.0
    assert int((u.min(1) <= 99.0).sum()) == 64
    same = np.array_equal(lr.face_map_in_order(sc, np.arange(F)), ref["face"])
    assert same                                                          # the helper itself
    # every covered pixel is covered by a face and its duplicate: the reversed walk changes every winner
    rev = lr.face_map_in_order(sc, np.arange(F)[::-1])
    assert int((rev != ref["face"]).sum()) == 1089
    for name, order in (("waves", lr.wave_reversed_order(F)), ("chunks", lr.chunk_reversed_order(F))):
        assert sorted(order.tolist()) == list(range(F))
        other = lr.face_map_in_order(sc, order)
        n = int((other != ref["face"]).sum())
        print(name, n)
        assert n > 0, name
        assert np.array_equal(other >= 0, cov)


def test_tile_edges_reference():
    sc = lr.tile_edges()
    ref = lr.render_scene(sc)
    assert sc["S"] == 49 and int(ref["cover"].sum()) == 1089
    for k in (16, 48):
        assert ref["cover"][k, 16:49].all() and ref["cover"][16:49, k].all(), k
    assert not ref["cover"][:16].any() and not ref["cover"][:, :16].any()
    assert (ref["depth"][ref["cover"]] == 1.0).all()


@pytest.mark.parametrize("S", sorted(lr.SIZE_WINDOWS))
def test_size_references(S):
    one, many = lr.size_reference(S, 1), lr.size_reference(S, 256)
    covered = {1: 1, 16: 9 * 13, 17: 17 * 17, 480: 561}[S]
    assert int(one["cover"].sum()) == int(many["cover"].sum()) == covered
    assert (one["region"][one["cover"]] == 1).all() and not one["region"][~one["cover"]].any()
    reg = many["region"][many["cover"]]
    assert reg.min() >= 1 and reg.max() <= 128
    # every region point has a bit-copy 128 places on: the highest j on ties would give an index above 128
    rp = lr.region_points(256)
    assert np.array_equal(rp[:128], rp[128:]) and len(np.unique(rp[:128], axis=0)) == 128


# ------------------------------------------------------------------------------------------------ B

def test_cull_invariance_references():
    obs = lr.observed("z1")
    assert (obs[lr.plane_depth("z1") > 0.0] == 1024.0).all() and int((obs == 3072.0).sum()) == 40 * 56 - 561
    vis = lr.visibility("z1", obs)
    assert vis["info"].tolist() == [561, 561, 561, 16, 16, 32, 16, 16, 16, 32, 16] and vis["visib_fract"] == 1.0
    assert vis["mask"][16:33, 48].all() and not vis["mask"][:, 49:].any() and not vis["mask"][:, :16].any()
    near = lr.visibility("near", obs)
    assert near["info"][0] == 1536 and near["info"][3:7].tolist() == [8, 8, 47, 31]
    shift = lr.visibility("shift", obs)
    assert shift["info"][0] == 408 and shift["info"][3:7].tolist() == [32, 16, 23, 16]
    wide = lr.visibility("z1", lr.observed("z1", h=40, w=64))
    assert np.array_equal(wide["mask"][:, :56], vis["mask"]) and not wide["mask"][:, 56:].any()
    assert np.array_equal(wide["info"], vis["info"])


def test_vsd_threshold_equalities():
    """GT at z = 1, estimate at z = 2, diameter 4: at PX the cost is exactly 0.25; with raw 768 observed there,
    model - obs is exactly delta = 0.25."""
    flat, dip = lr.observed("z1"), lr.observed("z1", at=768.0)
    for obs in (flat, dip):
        assert lr.vsd("z2", "z1", obs)["counts"].tolist() == [561, 153, 153, 153, 0]
    taus = (0.125, _step(0.25, UP), 0.5)                     # `cost >= tau`: one step up loses exactly PX
    for obs in (flat, dip):
        assert lr.vsd("z2", "z1", obs, taus=taus)["counts"].tolist() == [561, 153, 153, 152, 0]
    # `(model - obs) <= delta`: one step down and PX is not visible under the GT pose, nor under the estimate
    assert lr.vsd("z2", "z1", dip, delta=_step(0.25, DOWN))["counts"].tolist() == [560, 152, 152, 152, 0]
    assert lr.vsd("z2", "z1", flat, delta=_step(0.25, DOWN))["counts"].tolist() == [561, 153, 153, 153, 0]
    e = lr.vsd("z2", "z1", dip)["e_vsd"]
    assert e.tolist() == [(153 + 408) / 561, (153 + 408) / 561, 408 / 561]
    vis = lr.visibility("z1", dip)
    assert vis["info"][:3].tolist() == [561, 561, 561]
    assert lr.visibility("z1", dip, delta=_step(0.25, DOWN))["info"][:3].tolist() == [561, 561, 560]


def _f32_step(x, to):
    return np.nextafter(np.float32(x), np.float32(to))


def test_score_threshold_equalities():
    """A candidate at z = 1, tau = 0.25: raw 768 at PX is diff == tau, raw 1280 is diff == -tau; both are
    claimed inliers. One f32 step further out: the near side is occluded (claim and inter drop), the far side
    stays claimed but is no inlier (inter drops)."""
    full = [561] * 6
    for raw in (768.0, 1280.0):
        res = lr.score(["z1"], lr.observed("z1", at=raw))
        assert res["counts"][0].tolist() == full and res["score"][0] == 1.0, raw
    near = lr.score(["z1"], lr.observed("z1", at=_f32_step(768.0, 0.0)))
    assert near["counts"][0].tolist() == [561, 560, 561, 560, 560, 561] and near["score"][0] == 560 / 561
    far = lr.score(["z1"], lr.observed("z1", at=_f32_step(1280.0, np.inf)))
    assert far["counts"][0].tolist() == [561, 561, 561, 561, 560, 561] and far["score"][0] == 560 / 561
    # the same flips with the samples on the threshold and tau one step down
    tau = _step(0.25, DOWN)
    assert lr.score(["z1"], lr.observed("z1", at=768.0), tau=tau)["counts"][0].tolist() == near["counts"][0].tolist()
    assert lr.score(["z1"], lr.observed("z1", at=1280.0), tau=tau)["counts"][0].tolist() == far["counts"][0].tolist()
    # and one step inside changes nothing
    for raw in (_f32_step(768.0, np.inf), _f32_step(1280.0, 0.0)):
        assert lr.score(["z1"], lr.observed("z1", at=raw))["counts"][0].tolist() == full


def test_score_cull_references():
    obs = lr.observed("z1")
    res = lr.score(["z1", "near", "shift", "z2"], obs)
    # near: 0.5 m in front of everything (diff < -tau: claimed, no inlier); shift: on the plane where they overlap
    # (x 32..48), 2 m in front of the background elsewhere; z2: 1 m behind the plane (occluded, neutral)
    assert res["counts"].tolist() == [[561] * 6, [1536, 1536, 561, 561, 0, 1536], [408, 408, 561, 289, 289, 680],
                                      [153, 0, 561, 0, 0, 561]]
    assert res["best"] == 0


# ------------------------------------------------------------------------------------------------ C

@pytest.mark.parametrize("case", sorted(lr.REFINE_CASES))
def test_refiner_table(case):
    res = lr.refine_reference(case)
    status, passes, pairs, rmse = lr.REFINE_EXPECTED[case]
    assert (dr.STATUS[res["status"]], res["passes"], res["pairs"]) == (status, passes, pairs), case
    assert res["rmse"] == np.float32(rmse)                   # 2^-7 exactly, or +inf
    assert res["R"].tobytes() == np.eye(3, dtype=np.float32).tobytes()
    assert res["t"].tobytes() == np.array([0, 0, 1], np.float32).tobytes()
    assert res["trace"][0]["err"] == (lr.GAP ** 2 if pairs else np.inf)


def test_refiner_discriminators():
    # the gate is strict: at equality nothing is kept, one step above everything is
    assert lr.refine_reference("gate_equal")["pairs"] == 0 and lr.refine_reference("gate_above")["pairs"] == 561
    assert _step(lr.GAP, UP) == lr.GAP * (1.0 + 2.0 ** -52)
    below = dr.refine(**lr.refine_args(max_dist=_step(lr.GAP, DOWN), max_iter=0))
    assert (dr.STATUS[below["status"]], below["pairs"]) == ("STARVED", 0)
    # K < min_pairs is strict the other way: 561 pairs pass min_pairs = 561 and starve at 562
    assert lr.refine_reference("pairs_561")["status"] != lr.refine_reference("pairs_562")["status"]
    # the zero pivot is the damping's absence: with the default damp the same frame takes a step
    damped = dr.refine(**lr.refine_args(max_iter=1))
    assert damped["passes"] == 1 and dr.STATUS[damped["status"]] != "DEGENERATE"
    assert abs(damped["t64"][2] - (1.0 + lr.GAP)) < 1e-5      # onto the observed plane
    piv = lr.refine_reference("pivot")["trace"][0]["margins"]["pivot"]
    assert piv == 0.0                                        # exactly: rows 2..4 of A are zero


def test_starved_after_an_update_is_decided():
    res = lr.starve_reference()
    dr.check_conditions(res)
    assert (dr.STATUS[res["status"]], res["passes"], res["pairs"]) == ("STARVED", 1, 124)
    assert [s["K"] for s in res["trace"]] == [126, 124]
    assert 6.2e-5 < float(res["rmse"]) < 6.4e-5
    sc = br.scene("tetra")
    assert res["R"].tobytes() != np.asarray(sc["R_est"], np.float32).tobytes()
    assert np.array_equal(res["R"], res["R64"].astype(np.float32))       # cast from the f64 state


# ------------------------------------------------------------------------------------------------ D

def test_mssd_slice_edges():
    cases = lr.ms_cases()
    last = {}
    for ns, k in lr.MS_TARGET.items():
        c = cases[f"ns{ns}"]
        assert len(c["verts"]) == 162 and len(c["syms"]) == ns
        assert len(np.unique(c["syms"], axis=0)) == ns
        _, _, i3, i2, m3, m2 = lr.ms_reference(c)
        assert i3 == i2 == k, (ns, i3, i2)
        two3, two2 = np.sort(m3)[:2], np.sort(m2)[:2]
        assert two3[1] > 2 * two3[0] and two2[1] > 2 * two2[0]           # no near tie
        per = -(-ns // lr.SYM_SPLIT)
        last[ns] = (lr.slice_of(k, ns), (ns - 1) // per)
    assert last[15] == (14, 14) and last[17] == (8, 8) and last[33] == (10, 10)  # the last non-empty slice
    assert last[16][0] == 0 and last[32][0] == 0                                 # slice 0


def test_mssd_cross_slice_ties():
    cases = lr.ms_cases()
    for name, low, high in (("tie_low", 5, 16), ("tie_zero", 0, 16)):
        c = cases[name]
        _, _, i3, i2, m3, m2 = lr.ms_reference(c)
        assert m3[low] == m3[high] == m3.min() and m2[low] == m2[high] == m2.min(), name
        assert i3 == i2 == low, name
        assert lr.slice_of(low, 17) != lr.slice_of(high, 17)
        highest = len(m3) - 1 - int(np.argmin(m3[::-1]))                 # "highest on ties" gives another index
        assert highest == high != i3, name


def test_mssd_vertex_counts():
    cases = lr.ms_cases()
    assert [len(cases[k]["verts"]) for k in ("v1", "v256", "v257")] == [1, 256, 257]
    assert len(lr.ms_mesh(3)) == 642
    for k in ("v1", "v256", "v257"):
        m3, m2, i3, i2, _, _ = lr.ms_reference(cases[k])
        assert np.isfinite(m3) and np.isfinite(m2) and i3 == i2 == 2, k
