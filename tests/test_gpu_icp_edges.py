"""krrn_icp_refine_f32 at the slot, model-tail, stop and degenerate-input edges of tests/icp_cases.py, through the raw
entry point, against the numpy restatement (tests/icp_ref.py): passes, pairs, status and every nearest-neighbour
index equal; R / t / rmse within 1e-6 (the f32 output format's bound, tests/test_gpu_icp.py's TOL); every output
written in full and nothing beside it (tests/guarded.py). tests/test_solver_cases_host.py shows on the CPU that each
row meets the condition it is named for and the margins that license the exact comparisons.

Worst differences observed on an MI355X over all rows: |dR| 2.98e-08, |dt| 2.95e-08, |drmse| 5.76e-09."""
import numpy as np
import pytest
import torch

import icp_cases as ic
import icp_ref as ir
from guarded import Guarded
from pose_estimation_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 1e-6
WORST = {"dR": 0.0, "dt": 0.0, "drmse": 0.0}  # over the tests run so far (printed by each)
OUTS = ("R", "t", "passes", "pairs", "rmse", "status", "nn_idx")
STATUS = ("CONVERGED", "MAX_ITER", "STARVED", "DEGENERATE")


def _launch(dev, scs, max_dist, with_nn=True, max_iter=ir.MAX_ITER, tol=ir.TOL, min_pairs=ir.MIN_PAIRS):
    """One launch on scenes of one shape; every output a guarded view of exactly its extent."""
    up = lambda k: torch.from_numpy(np.ascontiguousarray(np.stack([s[k] for s in scs]))).to(dev)  # noqa: E731
    R0, t0, cloud, model = up("R0"), up("t0"), up("cloud"), up("model")
    B, N, M = cloud.shape[0], cloud.shape[1], model.shape[1]
    md = torch.from_numpy(np.broadcast_to(np.asarray(max_dist, np.float32), (B,)).copy()).to(dev)
    assert R0.shape == (B, 3, 3) and t0.shape == (B, 3) and model.shape == (B, M, 3) and R0.dtype == torch.float32
    f32 = torch.float32
    g = dict(R=Guarded(dev, (B, 9), f32), t=Guarded(dev, (B, 3), f32), passes=Guarded(dev, (B,)), pairs=Guarded(dev, (B,)),
             rmse=Guarded(dev, (B,), f32), status=Guarded(dev, (B,)), nn_idx=Guarded(dev, (B, N)))
    ptr, P = _lib.ptr, _lib.P
    _lib.call("krrn_icp_refine_f32", ptr(R0), ptr(t0), ptr(cloud), N, ptr(model), M, ptr(md), int(max_iter), float(tol),
              int(min_pairs), P(g["R"].ptr), P(g["t"].ptr), P(g["passes"].ptr), P(g["pairs"].ptr), P(g["rmse"].ptr),
              P(g["status"].ptr), P(g["nn_idx"].ptr if with_nn else 0), B, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    out = {k: v.get() for k, v in g.items()}  # (both guards of every buffer checked)
    for k in OUTS:
        if k == "nn_idx" and not with_nn:
            assert g[k].untouched()
        else:
            assert (out[k] != g[k].sentinel).all(), f"{k} not written in full"
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _check_crop(tag, got, b, ref, sc):
    assert int(got["status"][b]) == ref["status"], (tag, got["status"][b], ref["status"])
    assert int(got["passes"][b]) == ref["passes"], (tag, got["passes"][b], ref["passes"])
    assert int(got["pairs"][b]) == ref["pairs"], (tag, got["pairs"][b], ref["pairs"])
    assert np.array_equal(got["nn_idx"][b], ref["nn_idx"]), (tag, np.nonzero(got["nn_idx"][b] != ref["nn_idx"])[0][:8])
    R, t, rmse = got["R"][b].reshape(3, 3), got["t"][b], float(got["rmse"][b])
    if ref["passes"] == 1:  # a stop in pass 0 hands the input back bit for bit
        assert np.array_equal(_bits(R), _bits(sc["R0"])) and np.array_equal(_bits(t), _bits(sc["t0"])), tag
    dR, dt = float(np.abs(R - ref["R"]).max()), float(np.abs(t - ref["t"]).max())
    dr = 0.0 if np.isinf(ref["rmse"]) and rmse == np.inf else abs(rmse - ref["rmse"])
    print(f"{tag}: {STATUS[ref['status']]} after {ref['passes']} passes, {ref['pairs']} pairs, "
          f"|dR| {dR:.2e} |dt| {dt:.2e} |drmse| {dr:.2e}")
    assert dR <= TOL and dt <= TOL and dr <= TOL, (tag, dR, dt, dr)
    for k, v in (("dR", dR), ("dt", dt), ("drmse", dr)):
        WORST[k] = max(WORST[k], v)


@pytest.mark.parametrize("cid", [c.id for c in ic.ICP_EDGE_CASES])
def test_edge_case_matches_restatement(dev, cid):
    sc, ref = ic.build(cid), ic.reference(cid)
    got = _launch(dev, [sc], sc["max_dist"], **sc["kw"])
    _check_crop(cid, got, 0, ref, sc)
    if cid == "starved_after_update":  # the pose handed back is the updated one, not the input
        assert got["passes"][0] == 2 and np.abs(got["R"][0].reshape(3, 3) - sc["R0"]).max() > 1e-4
    if cid == "degenerate_after_update":  # the pose from before the failed update: finite, and not the input
        assert got["passes"][0] == 2 and np.isfinite(got["R"][0]).all() and np.isfinite(got["t"][0]).all()
        assert np.abs(got["R"][0].reshape(3, 3) - sc["R0"]).max() > 1e-2
    if ref["status"] == ir.DEGENERATE:
        assert got["pairs"][0] >= ir.MIN_PAIRS and np.isfinite(got["rmse"][0])
    print(f"worst so far: |dR| {WORST['dR']:.2e} |dt| {WORST['dt']:.2e} |drmse| {WORST['drmse']:.2e}")


def test_null_nn_idx_on_two_slots(dev):
    """Without the optional nn_idx buffer at N = 513: every other output bit-equal, the buffer untouched."""
    sc = ic.build(ic.NULL_NN)
    full = _launch(dev, [sc], sc["max_dist"], **sc["kw"])
    bare = _launch(dev, [sc], sc["max_dist"], with_nn=False, **sc["kw"])
    for k in OUTS[:-1]:
        assert np.array_equal(_bits(bare[k]), _bits(full[k])), k


def test_batch_of_all_statuses_equals_single_launches(dev):
    """Six crops with their own max_dist and all four statuses: each equals the restatement and, bit for bit, its
    own B = 1 launch."""
    scs, md, refs = ic.batch()
    batched = _launch(dev, scs, md, **ic.BATCH_KW)
    assert set(batched["status"].tolist()) == {0, 1, 2, 3}
    for b in range(len(scs)):
        _check_crop(f"batch[{b}]", batched, b, refs[b], scs[b])
        one = _launch(dev, scs[b:b + 1], md[b:b + 1], **ic.BATCH_KW)
        for k in OUTS:
            assert np.array_equal(_bits(one[k][0]), _bits(batched[k][b])), (b, k)
