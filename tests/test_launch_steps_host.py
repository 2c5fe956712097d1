"""The solver steps' single statement of each launch (pose.pnp_step / model_points_step,
umeyama.ransac_step, icp.refine_step), driven on the CPU through a recording context and checked
against include/krrn_hip.h: argument count, a c_void_p at every pointer position and a Python number at
every scalar position. The same functions make the eager calls (runtime.Immediate) and the plan ops
(runtime.Plan), so this covers both. Plus a source check: the stream pointer and the status check are
spelled in _lib.py / runtime.py only."""
import ctypes
import glob
import os

import torch

from pose_estimation_amd import _lib, icp, pose, umeyama
from pose_estimation_amd.runtime import RngStream

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pose_estimation_amd")
B, N, P, H, M, S = 2, 40, 16, 8, 12, 10


class Recorder:
    """Plan's two verbs on the CPU: buffers are host tensors, launches are written down."""

    def __init__(self):
        self.launches = []

    def buf(self, shape, dtype=torch.float32):
        return torch.empty(tuple(shape), dtype=dtype)

    def add(self, name, *args):
        self.launches.append((name, args))


def _check(rec, names):
    assert [n for n, _ in rec.launches] == names
    for name, args in rec.launches:
        sig = _lib.SIGNATURES[name]
        assert len(args) + 1 == len(sig), name  # the context appends the stream
        assert sig[-1] is ctypes.c_void_p
        for i, (a, ty) in enumerate(zip(args, sig)):
            if ty is ctypes.c_void_p:
                assert isinstance(a, ctypes.c_void_p), (name, i, a)
            elif ty in (ctypes.c_float, ctypes.c_double):
                assert isinstance(a, (int, float)) and not isinstance(a, bool), (name, i, a)
            else:
                assert isinstance(a, int) and not isinstance(a, bool), (name, i, a)


def _pnp_inputs():
    f32, f64 = torch.float32, torch.float64
    return dict(xyz=torch.zeros((B, 3, S, S), dtype=f32), choose=torch.zeros((B, N), dtype=torch.int64), B=B, N=N,
                xm=torch.zeros((B, N), dtype=f32), ym=torch.zeros((B, N), dtype=f32),
                K4=torch.zeros((B, 4), dtype=f32), ext=torch.zeros((B, 3), dtype=f64),
                lfb=torch.zeros((B, 3), dtype=f64), P_=P, n_hyp=H)


SEED = torch.zeros(1, dtype=torch.int64)


def test_pnp_step():
    drawn = Recorder()
    R, t, inl, info = pose.pnp_step(drawn, **_pnp_inputs(), seed=SEED, sel_stream=RngStream.PNP_PLAN_SEL,
                                    subsets_stream=RngStream.PNP_PLAN_SUBSETS)
    _check(drawn, ["krrn_randperm_i32", "krrn_ransac_subsets", "krrn_pnp_ransac_f32"])
    assert drawn.launches[0][1][1] == 5 and drawn.launches[1][1][1] == 6
    assert (R.shape, t.shape, inl.shape) == ((B, 3, 3), (B, 3), (B,))
    assert info["sel"].shape == (B, P) and info["subsets"].shape == (B, H, 5) and info["mask"].shape == (B, P)
    assert info["workspace"].numel() == B * H * 13
    # the eager form: sel given (CPU generator), subsets drawn
    half = Recorder()
    sel = torch.zeros((B, P), dtype=torch.int32)
    pose.pnp_step(half, **_pnp_inputs(), sel=sel, seed=SEED, subsets_stream=RngStream.PNP_SUBSETS)
    _check(half, ["krrn_ransac_subsets", "krrn_pnp_ransac_f32"])
    assert half.launches[0][1][1] == 7
    given = Recorder()
    subsets = torch.zeros((B, H, 5), dtype=torch.int32)
    _, _, _, info = pose.pnp_step(given, **_pnp_inputs(), sel=sel, subsets=subsets)
    _check(given, ["krrn_pnp_ransac_f32"])
    assert info["sel"] is sel and info["subsets"] is subsets
    # drawn and given differ by the draw launches only: the solver launch has the same scalars
    scal = lambda a: [x for x in a if not isinstance(x, ctypes.c_void_p)]  # noqa: E731
    assert scal(drawn.launches[-1][1]) == scal(half.launches[-1][1]) == scal(given.launches[-1][1])
    assert given.launches[-1][1][4].value == sel.data_ptr() and given.launches[-1][1][11].value == subsets.data_ptr()


def test_model_points_step():
    rec = Recorder()
    i = _pnp_inputs()
    src = pose.model_points_step(rec, i["xyz"], i["choose"], B, N, i["ext"], i["lfb"])
    _check(rec, ["krrn_model_points_f32"])
    assert src.shape == (B, N, 3) and rec.launches[0][1][1] == S * S


def test_umeyama_step():
    src, dst = torch.zeros((B, N, 3)), torch.zeros((B, N, 3))
    drawn = Recorder()
    scale, R, t, info = umeyama.ransac_step(drawn, src, dst, B, N, H, seed=SEED, stream_id=RngStream.UMEYAMA_PLAN)
    _check(drawn, ["krrn_ransac_subsets", "krrn_umeyama_ransac_f32"])
    assert drawn.launches[0][1][1] == 10
    assert (scale.shape, R.shape, t.shape) == ((B,), (B, 3, 3), (B, 3))
    assert info["hyp_counts"].shape == (B, H) and info["mask"].shape == (B, N) and info["subsets"].shape == (B, H, 5)
    assert info["inliers"].shape == info["best_hyp"].shape == (B,)
    given = Recorder()
    subsets = torch.zeros((B, H, 5), dtype=torch.int32)
    _, _, _, info = umeyama.ransac_step(given, src, dst, B, N, H, subsets)
    _check(given, ["krrn_umeyama_ransac_f32"])
    assert info["subsets"] is subsets and given.launches[0][1][3].value == subsets.data_ptr()
    scal = lambda a: [x for x in a if not isinstance(x, ctypes.c_void_p)]  # noqa: E731
    assert scal(drawn.launches[-1][1]) == scal(given.launches[-1][1])


def test_icp_step():
    R0, t0, md = torch.zeros((B, 3, 3)), torch.zeros((B, 3)), torch.zeros((B,))
    cloud, model = torch.zeros((B, N, 3)), torch.zeros((B, M, 3))
    rec = Recorder()
    R, t, info = icp.refine_step(rec, R0, t0, cloud, model, md, B, N, M)
    _check(rec, ["krrn_icp_refine_f32"])
    assert info["nn_idx"].shape == (B, N) and rec.launches[0][1][16].value == info["nn_idx"].data_ptr()
    assert sorted(info) == ["nn_idx", "pairs", "passes", "rmse", "status"]
    bare = Recorder()
    _, _, info = icp.refine_step(bare, R0, t0, cloud, model, md, B, N, M, with_nn=False)
    _check(bare, ["krrn_icp_refine_f32"])
    assert info["nn_idx"] is None and not bare.launches[0][1][16].value  # the null nn_idx


def test_stream_ids_are_distinct():
    ids = list(RngStream.POOL) + [RngStream.PNP_PLAN_SEL, RngStream.PNP_PLAN_SUBSETS, RngStream.PNP_SUBSETS,
                                  RngStream.UMEYAMA_OWN, RngStream.UMEYAMA_POSE, RngStream.UMEYAMA_PLAN]
    assert ids == list(range(11))


def test_stream_pointer_and_status_check_live_in_two_modules():
    home = {"_lib.py", "runtime.py"}
    for p in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        with open(p) as fh:
            s = fh.read()
        if os.path.basename(p) not in home:
            assert "cuda_stream" not in s, p
            assert "_lib.check(" not in s, p
