"""Umeyama-RANSAC without a GPU: the numpy restatement (tests/umeyama_ref.py) against the results
recorded from the reference's own estimateSimilarityTransform (tests/golden/umeyama_scenes.npz,
written by tests/golden/make_umeyama_golden.py), and the host-side argument checks of the two
entry points (they run before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import umeyama_ref as ur
from pose_estimation_amd import _lib
from pose_estimation_amd.umeyama import estimateSimilarityTransform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "umeyama_scenes.npz")
SCENES = ("exact", "tail", "long", "planar", "scaled", "fail")


def test_fixture_holds_the_six_scenes():
    z = np.load(GOLDEN)
    assert tuple(z["names"].tolist()) == SCENES
    assert os.path.getsize(GOLDEN) < 300 * 1024
    for n in SCENES:
        assert z[f"{n}_src"].dtype == np.float32 and z[f"{n}_dst"].dtype == np.float32
        assert z[f"{n}_subsets"].shape == (128, 5)
    assert bool(z["fail_failed"]) and not any(bool(z[f"{n}_failed"]) for n in SCENES[:-1])


@pytest.mark.parametrize("name", SCENES)
def test_restatement_reproduces_reference(name):
    z = np.load(GOLDEN)
    res = ur.ransac(z[f"{name}_src"], z[f"{name}_dst"], z[f"{name}_subsets"])
    ur.check_conditions(res)
    assert res["failed"] == bool(z[f"{name}_failed"])
    if res["failed"]:
        assert res["inliers"] == 0 and res["best_hyp"] == -1
        return
    assert abs(res["scale"] - float(z[f"{name}_scale"])) <= 1e-12
    assert np.abs(res["R"] - z[f"{name}_R"]).max() <= 1e-12
    assert np.abs(res["t"] - z[f"{name}_t"]).max() <= 1e-12
    assert abs(np.linalg.det(res["R"]) - 1.0) < 1e-12


def test_scene_properties():
    """What each scene pins (the issue's table): early stop at i = 1, a point past a 256 block with
    duplicate indices in samples, a deep run, rank-2 model points, a scale away from 1."""
    z = np.load(GOLDEN)
    r = {n: ur.ransac(z[f"{n}_src"], z[f"{n}_dst"], z[f"{n}_subsets"]) for n in SCENES}
    assert r["exact"]["stop"] == 1 and r["exact"]["inliers"] == 64
    assert z["tail_src"].shape[0] == 257
    assert any(len(set(row)) < 5 for row in z["tail_subsets"].tolist())
    assert r["long"]["stop"] >= 100
    assert np.ptp(z["planar_src"][:, 2]) == 0.0
    assert abs(r["scaled"]["scale"] - 1.7) < 0.01


def test_host_side_errors():
    lib = _lib.lib()
    N = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(16)
    D = ctypes.c_double
    ume = lib.krrn_umeyama_ransac_f32

    names = ("src", "dst", "subsets", "hyp_counts", "scale", "R", "t", "inliers")

    def call(n=64, h=128, b=1, **null):
        p = {k: (N if k in null else fake) for k in names}
        return ume(p["src"], p["dst"], n, p["subsets"], h, D(0.1), D(0.99), D(0.1), p["hyp_counts"], p["scale"], p["R"],
                   p["t"], p["inliers"], N, N, b, N)

    for k in names:  # every required pointer; best_hyp and inlier_mask are optional (null in every call here)
        assert call(**{k: True}) == -1, k
    assert call(n=4) == -2
    assert call(n=4097) == -2
    assert call(h=0) == -2
    assert call(h=8193) == -2
    assert call(b=0) == -2
    assert call(n=4, src=True) == -1  # pointers are checked first
    mp = lib.krrn_model_points_f32
    assert mp(N, 16, fake, 8, fake, fake, fake, 1, N) == -1
    assert mp(fake, 16, fake, 8, fake, fake, N, 1, N) == -1
    assert mp(fake, 16, fake, 0, fake, fake, fake, 1, N) == -2
    assert mp(fake, 16, fake, 8, fake, fake, fake, 0, N) == -2


def test_cpu_tensors_raise():
    with pytest.raises(RuntimeError, match="HIP path only"):
        estimateSimilarityTransform(torch.zeros(8, 3), torch.zeros(8, 3))
    from pose_estimation_amd.pose import get_pose_umeyama
    with pytest.raises(RuntimeError, match="HIP path only"):
        get_pose_umeyama({"xyz": torch.zeros(1, 3, 4, 4)}, {})


def test_evaluate_rejects_unknown_solver():
    from pose_estimation_amd.evaluate import eval_records
    with pytest.raises(ValueError, match="pose_solver"):
        eval_records(None, None, {}, 1, "cpu", pose_solver="icp")
