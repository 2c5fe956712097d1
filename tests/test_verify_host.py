"""No-GPU checks of the pose-candidate score: the numpy restatement's own conditions and known answers
(tests/verify_ref.py; every GPU parity case must be decided before any GPU run), the host-side rejections of
krrn_pose_score_f32 (they run before any HIP call), and the errors of the python layers above it."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import bop_ref as br
import raster_ref as rr
import verify_ref as vr
from pose_estimation_amd import _lib, bop, verify
from pose_estimation_amd.dataset import PoseDataset


# ------------------------------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("name", vr.SCENES)
def test_reference_scenes_are_decided(name):
    ref = vr.reference(name)
    vr.check_conditions(ref)
    c = ref["counts"]
    assert c.shape == (3, 6) and (c[:, 5] == c[:, 1] + c[:, 2] - c[:, 3]).all()
    assert (c[:, 4] <= c[:, 3]).all() and (c[:, 3] <= np.minimum(c[:, 1], c[:, 2])).all() and (c[:, 1] <= c[:, 0]).all()
    assert (c[:, 2] == c[0, 2]).all()                            # the evidence does not depend on the candidate
    assert ((ref["score"] >= 0.0) & (ref["score"] <= 1.0)).all()
    if name == "empty_obs":
        assert not c[:, 1:].any() and ref["best"] == 0 and (c[:, 0] > 0).all()
    if name == "gross":                                          # the estimate misses the mask altogether
        assert ref["score"][0] == 0.0 and ref["best"] == 1
    if name not in ("empty_obs", "tetra"):                       # GT beats the coarse perturbation everywhere; on the
        assert ref["best"] == 1                                  # 4-face tetra the 3-degree estimate ties it closely
    assert ref["score"][2] <= ref["score"][1]


def test_reference_mixed_batch_is_decided():
    for b in range(rr.MIXED_B):
        ref = vr.mixed_reference(b)
        vr.check_conditions(ref)
        assert ref["best"] == (0 if b == 3 else 1)
    assert not vr.mixed_reference(3)["counts"].any()


def test_reference_known_answers():
    case = vr.scene_case("tetra")
    sil = vr.silhouette(case)
    d_gt, _ = br.depth_image(case["verts"], case["faces"], case["R_gt"], case["t_gt"], case["K4"], case["H"], case["W"])
    clean = dict(case, depth=(np.where(sil, d_gt, 1.5) * br.DEPTH_SCALE).astype(np.float32), mask=sil.astype(np.uint8))
    n = int(sil.sum())
    nan = np.full((3, 3), np.nan)
    ref = vr.case_score(dict(clean, Rs=np.stack([nan, case["R_gt"], case["R_gt"]]),
                             ts=np.stack([case["t_gt"], case["t_gt"] + [5.0, 0.0, 0.0], case["t_gt"]])))
    vr.check_conditions(ref)
    assert ref["counts"].tolist() == [[0, 0, n, 0, 0, n], [0, 0, n, 0, 0, n], [n] * 6]
    assert ref["score"].tolist() == [0.0, 0.0, 1.0] and ref["best"] == 2
    assert vr.case_score(dict(clean, Rs=nan[None], ts=case["t_gt"][None]))["best"] == 0


# ------------------------------------------------------------------------------------------ host checks

def _fakes(names):
    """Distinct, far-apart non-null pointers (never dereferenced: the checks fail before any launch)."""
    return {k: ctypes.c_void_p((i + 1) << 36) for i, k in enumerate(names)}


def test_score_host_side_errors():
    fn = _lib.lib().krrn_pose_score_f32
    N, D = ctypes.c_void_p(0), ctypes.c_double
    names = ("verts", "faces", "face_range", "R", "t", "K4", "depth", "mask", "frame", "box", "tau", "ws", "counts",
             "score", "best", "R_sel", "t_sel")
    optional = ("mask", "box", "R_sel", "t_sel")
    EARG, ESHAPE = -1, -2

    def call(V=10, Ft=4, C=3, F=2, H=48, W=64, scale=1.0, B=2, **over):
        p = _fakes(names)
        p.update(over)
        return fn(p["verts"], V, p["faces"], Ft, p["face_range"], p["R"], p["t"], C, p["K4"], p["depth"], p["mask"], F, H,
                  W, p["frame"], p["box"], D(scale), p["tau"], B, p["ws"], p["counts"], p["score"], p["best"], p["R_sel"],
                  p["t_sel"], N)

    for k in names:
        if k not in optional:
            assert call(**{k: N}) == EARG, k
    f = _fakes(names)
    off = lambda k, n: ctypes.c_void_p(f[k].value + n)  # noqa: E731
    B, C = 2, 3
    assert call(counts=f["score"]) == EARG                       # two outputs on one buffer
    assert call(score=off("counts", 24 * B * C - 4)) == EARG     # the last count
    assert call(best=off("score", 8 * B * C - 8)) == EARG        # the last score
    assert call(counts=off("ws", 16 * B * C - 4)) == EARG        # the last ws int
    assert call(R_sel=off("best", 4 * B - 4)) == EARG and call(t_sel=off("R_sel", 36 * B - 4)) == EARG
    assert call(best=off("t_sel", 12 * B - 4)) == EARG
    assert call(counts=f["R"]) == EARG and call(score=f["tau"]) == EARG and call(ws=f["frame"]) == EARG   # on an input
    assert call(best=off("mask", 2 * 48 * 64 - 1)) == EARG       # the last mask byte
    assert call(R_sel=off("t", 24 * B * C - 4)) == EARG and call(t_sel=off("box", 16 * B - 4)) == EARG
    assert call(C=0) == ESHAPE and call(C=9) == ESHAPE and call(C=-1) == ESHAPE
    assert call(B=0) == ESHAPE and call(B=-1) == ESHAPE and call(B=65536) == ESHAPE
    assert call(V=0) == ESHAPE and call(Ft=-1) == ESHAPE and call(F=0) == ESHAPE and call(H=0) == ESHAPE
    assert call(W=0) == ESHAPE
    assert call(scale=0.0) == ESHAPE and call(scale=-1.0) == ESHAPE and call(scale=float("nan")) == ESHAPE
    assert call(C=9, score=N) == EARG                            # pointers are checked first
    n = ctypes.c_longlong(0)
    ws = _lib.lib().krrn_pose_score_ws
    assert ws(3, 8, ctypes.byref(n)) == 0 and n.value == 3 * 8 * 4
    assert ws(3, 1, ctypes.byref(n)) == 0 and n.value == 12
    assert ws(0, 2, ctypes.byref(n)) == ESHAPE and ws(3, 0, ctypes.byref(n)) == ESHAPE
    assert ws(3, 9, ctypes.byref(n)) == ESHAPE and ws(3, 2, N) == EARG


def test_abi_lists_the_entry_points():
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert _lib.SIGNATURES["krrn_pose_score_f32"] == ([P, I, P, I, P, P, P, I, P, P, P, I, I, I, P, P, D, P, I] + [P] * 7)
    assert _lib.SIGNATURES["krrn_pose_score_ws"] == [I, I, P]
    assert verify.TAU == bop.DELTA == 0.015 and verify.MAX_C == 8 and verify.COUNTS == vr.COUNTS


# ------------------------------------------------------------------------------------------ python layers

def test_python_layer_errors(tmp_path):
    import mesh_tree
    from pose_estimation_amd import pose
    from pose_estimation_amd.evaluate import POSE_REC, REC, SEL_REC, eval_records
    from pose_estimation_amd.evaluate import test_epoch as run_epoch
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP path only"):
        verify.score_poses(z(4, 3), z(2, 3, dtype=torch.int32), z(1, 2, dtype=torch.int32), z(1, 2, 3, 3), z(1, 2, 3),
                           z(1, 4), z(1, 8, 8), z(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="verify=True"):
        pose.select_pose([(z(1, 3, 3), z(1, 3))], {"bop_depth": z(1, 8, 8)}, None)
    with pytest.raises(ValueError, match="at least one"):
        pose.select_pose([], {"verify_mask": z(1, 8, 8)}, None)
    assert SEL_REC == ("crop", "cand", "score", "inter", "union", "valid")
    assert len(REC) == 12 and len(POSE_REC) == 13 and len(bop.BOP_REC) == 15      # the other tables keep their shape
    sig = inspect.signature(PoseDataset.batch).parameters
    assert sig["verify"].default is False and sig["bop"].default is False
    assert inspect.signature(run_epoch).parameters["select"].default is None
    assert inspect.signature(eval_records).parameters["select"].default is None

    plain = PoseDataset("test", 500, False, None, 0.0, 8, cls_type="cat", num_frames=2)   # synthetic: no meshes
    with pytest.raises(ValueError, match="meshes"):
        plain.batch([0], "cpu", verify=True)
    root = str(tmp_path / "tree")
    mesh_tree.write_tree(root, objs=(6,), per_obj=(1,))
    meshed = PoseDataset("test", 100, False, root, 0.0, 8, cls_type="cat", n_model_pts=100, meshes=True)
    # the epoch's checks run before the model or the device is touched
    for fn in (lambda **kw: eval_records(None, kw.pop("ds"), {}, 2, "cpu", **kw),
               lambda **kw: run_epoch(None, kw.pop("ds"), bs=2, device="cpu", **kw)):
        with pytest.raises(ValueError, match="opt_pose"):
            fn(ds=meshed, select="depth", opt_pose=False)
        with pytest.raises(ValueError, match="meshes"):
            fn(ds=plain, select="depth")
        with pytest.raises(ValueError, match="select must be"):
            fn(ds=meshed, select="icp")
