"""The depth refiner's numpy restatement (tests/depth_refine_ref.py) on its own, the host-side refusals of
krrn_pose_refine_depth_f32 and the eval loop's argument checks. No GPU.

The restatement must (a) leave no decision of any pass within raster_ref.MARGIN of flipping on bop_ref's seven
scenes and on its mixed batch, which is what licenses the exact comparison of passes / pairs / status in
test_gpu_depth_refine.py; (b) reproduce the numpy prototype's statuses and pass counts; and
(c) pull the generic scenes' perturbed estimates onto the GT pose: at least 100 x closer in translation and 50 x in
rotation angle (the prototype's worst ratio is 300 x in rotation: a start rounded to f32 is orthonormal to 1e-7
only, which the angle measure reads as 0.008 degrees)."""
import ctypes

import numpy as np
import pytest

import bop_ref as br
import depth_refine_ref as dr

# scene: (status, the k at the stop)
EXPECTED = {"tetra": ("CONVERGED", 5), "degenerate": ("CONVERGED", 9), "small": ("CONVERGED", 10),
            "layers": ("CONVERGED", 4), "sphere": ("MAX_ITER", 10), "gross": ("STARVED", 0),
            "empty_obs": ("STARVED", 0)}
KNOWN = ("tetra", "degenerate", "small")


@pytest.mark.parametrize("name", br.SCENES)
def test_scene_is_decided_and_stops_as_the_prototype(name):
    res = dr.reference(name)
    dr.check_conditions(res)
    print(name, dr.STATUS[res["status"]], res["passes"], [s["K"] for s in res["trace"]], float(res["rmse"]))
    assert (dr.STATUS[res["status"]], res["passes"]) == EXPECTED[name]
    assert res["pairs"] == res["trace"][-1]["K"] and len(res["trace"]) == res["passes"] + 1
    if EXPECTED[name][0] == "STARVED":
        sc = br.scene(name)
        assert res["pairs"] == 0 and np.isinf(res["rmse"])
        assert res["R"].tobytes() == np.asarray(sc["R_est"], np.float32).tobytes()
        assert res["t"].tobytes() == np.asarray(sc["t_est"], np.float32).tobytes()
    else:
        Ks = [s["K"] for s in res["trace"]]
        assert all(b >= a for a, b in zip(Ks, Ks[1:])), Ks      # the kept pixels never drop
        R = res["R"].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6


@pytest.mark.parametrize("b", range(5))
def test_mixed_batch_is_decided(b):
    res = dr.mixed_reference(b)
    dr.check_conditions(res)
    if b == 3:                                                   # the empty face range
        assert (dr.STATUS[res["status"]], res["passes"], res["pairs"]) == ("STARVED", 0, 0)
    else:
        assert res["status"] in (0, 1) and res["pairs"] > 100


@pytest.mark.parametrize("name", KNOWN)
def test_known_answer(name):
    sc, res = br.scene(name), dr.reference(name)
    t_start, t_end = np.linalg.norm(sc["t_est"] - sc["t_gt"]), np.linalg.norm(res["t64"] - sc["t_gt"])
    r_start, r_end = dr.angle_deg(sc["R_est"], sc["R_gt"]), dr.angle_deg(res["R64"], sc["R_gt"])
    print(name, "t", t_start, t_end, "rot", r_start, r_end)
    assert t_end * 100.0 <= t_start
    assert r_end * 50.0 <= r_start


def test_max_iter_zero_and_layers_slide():
    sc = br.scene("tetra")
    res = dr.refine(**dr.scene_args(sc, max_iter=0))
    assert (dr.STATUS[res["status"]], res["passes"], res["pairs"]) == ("MAX_ITER", 0, dr.reference("tetra")["trace"][0]["K"])
    assert res["R"].tobytes() == np.asarray(sc["R_est"], np.float32).tobytes()
    lay, ref = br.scene("layers"), dr.reference("layers")      # planar faces: the in-plane slide is unobservable
    assert np.linalg.norm(ref["t64"] - lay["t_gt"]) < 1e-3 and [s["K"] for s in ref["trace"]][:2] == [247, 249]


def test_cholesky_refuses_what_the_kernel_refuses():
    A = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 0.0])
    assert dr.cholesky_solve(A, np.ones(6))[0] is None                       # a zero pivot
    assert dr.cholesky_solve(np.full((6, 6), np.nan), np.ones(6))[0] is None
    assert dr.cholesky_solve(np.eye(6), np.array([1.0, 2, 3, 4, 5, np.inf]))[0] is None
    M = np.random.default_rng(0).standard_normal((6, 6))
    A = M @ M.T + np.eye(6)
    xi, piv = dr.cholesky_solve(A, np.arange(6.0))
    assert np.allclose(A @ xi, np.arange(6.0), rtol=0, atol=1e-12) and min(piv) > 0


def test_host_side_refusals():
    from pose_estimation_amd import _lib
    lib = _lib.lib()
    N, D = ctypes.c_void_p(0), ctypes.c_double
    n_bytes = ctypes.c_longlong(-1)
    ws = lib.krrn_pose_refine_depth_ws
    assert ws(1, 480, 640, N) == -1
    assert ws(0, 480, 640, ctypes.byref(n_bytes)) == -2 and ws(1, 0, 640, ctypes.byref(n_bytes)) == -2
    assert ws(1, 480, 0, ctypes.byref(n_bytes)) == -2
    assert ws(2, 90, 120, ctypes.byref(n_bytes)) == 0
    tiles = 6 * 8
    assert n_bytes.value == 2 * (16 * 8 + 8 * 4 + tiles * (28 * 8 + 4))
    fn = lib.krrn_pose_refine_depth_f32
    names = ("verts", "faces", "face_range", "R0", "t0", "K4", "depth", "mask", "frame", "max_dist", "radius", "ws",
             "R", "t", "passes", "pairs", "rmse", "status")
    spread = {k: ctypes.c_void_p(1 << (24 + i)) for i, k in enumerate(names)}   # far apart: nothing overlaps

    def call(B=1, H=90, W=120, it=10, tol=1e-4, mp=6, damp=1e-4, F=1, Vtot=4, Ftot=4, scale=1000.0, ptrs=spread,
             **null):
        p = {k: (N if k in null else ptrs[k]) for k in names}
        return fn(p["verts"], Vtot, p["faces"], Ftot, p["face_range"], p["R0"], p["t0"], p["K4"], p["depth"], p["mask"],
                  F, H, W, p["frame"], D(scale), p["max_dist"], p["radius"], it, D(tol), mp, D(damp), B, p["ws"],
                  p["R"], p["t"], p["passes"], p["pairs"], p["rmse"], p["status"], N)

    for k in names:
        if k != "mask":                                          # the mask is optional
            assert call(**{k: True}) == -1, k
    for bad in (dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-3), dict(it=-1), dict(it=33), dict(mp=5),
                dict(mp=0), dict(tol=-1e-9), dict(tol=float("nan")), dict(tol=float("inf")), dict(damp=-1.0),
                dict(damp=float("nan")), dict(damp=float("inf")), dict(F=0), dict(Vtot=0), dict(Ftot=-1),
                dict(scale=0.0)):
        assert call(**bad) == -2, bad
    assert call(B=0, R0=True) == -1                              # pointers are checked first
    same = dict(spread, R=spread["R0"])                          # an output on an input
    assert call(ptrs=same) == -1
    inside = dict(spread, status=ctypes.c_void_p(spread["ws"].value + 64))   # an output inside the workspace
    assert call(ptrs=inside) == -1
    # nothing above reached a launch: every accepted combination would need real memory


def test_python_layer_refuses_early():
    import torch
    from pose_estimation_amd import depth_refine, icp, pose
    from pose_estimation_amd.evaluate import eval_records
    assert (depth_refine.MAX_ITER, depth_refine.TOL, depth_refine.MIN_PAIRS, depth_refine.DIST_FRAC,
            depth_refine.DAMP, depth_refine.RADIUS_FRAC) == (10, 1e-4, 6, 0.2, 1e-4, 0.5)
    assert (dr.MAX_ITER, dr.TOL, dr.MIN_PAIRS, dr.DIST_FRAC, dr.DAMP) == (10, 1e-4, 6, 0.2, 1e-4)
    assert depth_refine.STATUS == icp.STATUS == dr.STATUS
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP path only"):
        depth_refine.refine(z(4, 3), z(4, 3, dtype=torch.int32), z(1, 2, dtype=torch.int32), z(1, 3, 3), z(1, 3),
                            z(1, 4), z(1, 8, 8), z(1, dtype=torch.int32), 0.01, 0.05)
    with pytest.raises(ValueError, match="verify=True"):
        pose.refine_pose_depth(z(1, 3, 3), z(1, 3), {"bop_depth": z(1, 8, 8)}, None, 0.1)
    with pytest.raises(ValueError, match="refine"):
        eval_records(None, None, {}, 1, "cpu", refine="gicp")
    with pytest.raises(ValueError, match="meshes=True"):
        eval_records(None, None, {}, 1, "cpu", refine="depth")

    class NoMeshes:
        meshes = False

    with pytest.raises(ValueError, match="refine='depth'.*meshes=True"):
        eval_records(None, NoMeshes(), {}, 1, "cpu", refine="depth")
