"""ICP pose refinement without a GPU: the numpy restatement (tests/icp_ref.py) on the shared scene
family (its decision margins, its nearest neighbours against a k-d tree, the known answer of the
noise-free scene, ADD before and after), the host-side argument checks of krrn_icp_refine_f32 (they
run before any HIP call) and the Python entry points' errors."""
import ctypes

import numpy as np
import pytest
import torch

import icp_ref as ir
from pose_estimation_amd import _lib


@pytest.mark.parametrize("name", ir.SCENES)
def test_scene_conditions(name):
    """Every scene decides its nearest neighbours, its rejections and its stop with room to spare."""
    res = ir.reference(name)
    print(name, res["passes"], res["pairs"], res["status"], res["margins"])
    ir.check_conditions(res)


def test_mixed_batch_conditions():
    scs, md = ir.mixed_batch()
    res = [ir.icp(s["R0"], s["t0"], s["cloud"], s["model"], m) for s, m in zip(scs, md)]
    for r in res:
        ir.check_conditions(r)
    assert res[2]["status"] == ir.STARVED and res[2]["passes"] == 1
    assert res[3]["passes"] < min(res[0]["passes"], ir.MAX_ITER + 1)  # the noise-free crop stops early


def test_scene_properties():
    """What each scene pins (the table in icp_ref.SPECS)."""
    r = {n: ir.reference(n) for n in ir.SCENES}
    assert r["outl"]["pairs"] < 300 and (r["outl"]["nn_idx"] == -1).sum() == 300 - r["outl"]["pairs"]
    assert r["work"]["pairs"] == 1000
    assert r["max"]["passes"] == 6 and r["max"]["status"] == ir.MAX_ITER_HIT
    assert r["tiny"]["status"] == ir.CONVERGED and r["tiny"]["pairs"] == 8
    far, sc = r["far"], ir.scene("far")
    assert far["status"] == ir.STARVED and far["passes"] == 1 and far["pairs"] == 0 and far["rmse"] == np.inf
    assert np.array_equal(far["R"], sc["R0"].astype(np.float64)) and np.array_equal(far["t"], sc["t0"].astype(np.float64))
    assert (far["nn_idx"] == -1).all()


def test_duplicated_model_points_tie_to_the_first_copy():
    sc, res = ir.scene("dup"), ir.reference("dup")
    assert res["nn_idx"].max() < 65 and res["nn_idx"].min() >= 0
    one = ir.icp(sc["R0"], sc["t0"], sc["cloud"], sc["model65"], sc["max_dist"])
    for k in ("R", "t", "nn_idx"):
        assert np.array_equal(one[k], res[k]), k
    assert (one["passes"], one["pairs"], one["rmse"], one["status"]) == \
        (res["passes"], res["pairs"], res["rmse"], res["status"])


def test_nearest_matches_kdtree():
    """The brute-force argmin against scipy's k-d tree on the `odd` scene, at the start pose and at the result."""
    spatial = pytest.importorskip("scipy.spatial")
    sc, res = ir.scene("odd"), ir.reference("odd")
    P, Mo = sc["cloud"].astype(np.float64), sc["model"].astype(np.float64)
    tree = spatial.cKDTree(Mo)
    for R, t in ((sc["R0"].astype(np.float64), sc["t0"].astype(np.float64)), (res["R"], res["t"])):
        Q = (P - t) @ R
        j, d2, _ = ir.nearest(Q, Mo)
        dist, jt = tree.query(Q)
        assert np.array_equal(j, jt)
        assert np.abs(np.sqrt(d2) - dist).max() < 1e-12
    keep = res["nn_idx"] >= 0
    assert np.array_equal(res["nn_idx"][keep], jt[keep])


def test_exact_scene_recovers_ground_truth():
    """Noise-free cloud: the f32 rounding of the inputs is all that separates the result from the truth."""
    sc, res = ir.scene("exact"), ir.reference("exact")
    eR, et = np.abs(res["R"] - sc["R_gt"]).max(), np.abs(res["t"] - sc["t_gt"]).max()
    print(f"|R - R_gt| {eR:.2e}  |t - t_gt| {et:.2e} m  passes {res['passes']}")
    assert res["status"] == ir.CONVERGED and res["pairs"] == 64
    assert np.array_equal(res["nn_idx"], sc["pick"])
    assert eR <= 1e-6 and et <= 1e-6


@pytest.mark.parametrize("name", ir.NOISY)
def test_refinement_lowers_add(name):
    sc, res = ir.scene(name), ir.reference(name)
    before = ir.add(sc["R0"], sc["t0"].astype(np.float64), sc["R_gt"], sc["t_gt"], sc["model"])
    after = ir.add(res["R"], res["t"], sc["R_gt"], sc["t_gt"], sc["model"])
    print(f"{name}: ADD {before * 1e3:.3f} mm -> {after * 1e3:.3f} mm")
    assert after < before


def test_host_side_errors():
    fn = _lib.lib().krrn_icp_refine_f32
    N = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(16)
    D = ctypes.c_double
    names = ("R0", "t0", "cloud", "model", "max_dist", "R", "t", "passes", "pairs", "rmse", "status", "nn_idx")

    def call(n=64, m=64, it=20, mp=6, b=1, **null):
        p = {k: (N if k in null else fake) for k in names}
        return fn(p["R0"], p["t0"], p["cloud"], n, p["model"], m, p["max_dist"], it, D(1e-4), mp, p["R"], p["t"],
                  p["passes"], p["pairs"], p["rmse"], p["status"], p["nn_idx"], b, N)

    for k in names[:-1]:  # every required pointer; nn_idx is optional
        assert call(**{k: True}) == -1, k
    assert call(n=2) == -2 and call(n=4097) == -2
    assert call(m=0) == -2 and call(m=4097) == -2
    assert call(it=-1) == -2 and call(it=65) == -2
    assert call(mp=2) == -2
    assert call(b=0) == -2
    assert call(n=2, R0=True) == -1  # pointers are checked first


def test_cpu_tensors_raise():
    from pose_estimation_amd import icp, pose
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP path only"):
        icp.refine(z(3, 3), z(3), z(8, 3), z(8, 3), 0.02)
    with pytest.raises(RuntimeError, match="HIP path only"):
        pose.refine_pose_icp(z(1, 3, 3), z(1, 3), {"cloud": z(1, 8, 3), "model_points": z(1, 8, 3)}, diameter=0.1)


def test_defaults_are_the_documented_ones():
    from pose_estimation_amd import icp
    assert (icp.MAX_ITER, icp.TOL, icp.MIN_PAIRS, icp.DIST_FRAC) == (20, 1e-4, 6, 0.1)
    assert icp.STATUS == ("CONVERGED", "MAX_ITER", "STARVED", "DEGENERATE")
    assert (ir.MAX_ITER, ir.TOL, ir.MIN_PAIRS) == (icp.MAX_ITER, icp.TOL, icp.MIN_PAIRS)


def test_evaluate_rejects_unknown_refine():
    from pose_estimation_amd.evaluate import eval_records
    with pytest.raises(ValueError, match="refine"):
        eval_records(None, None, {}, 1, "cpu", refine="gicp")
