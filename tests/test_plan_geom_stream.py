"""The fusion's geometry stream (KRRN_GEOM_EARLY), checked on a CPU build of the plan: the launches that
read only p9 and the perms run on plan stream fusion.GEOM_SID, every launch on another stream that
reads one of their outputs is ordered after the producing launch through a chain of syncs that starts
on the geometry stream, and the stream is joined into stream 0 before the plan ends. With the knob off
no launch is on that stream and the same launches are emitted."""
import ctypes

import torch

from pose_estimation_amd import KRRN, fusion, make_config
from pose_estimation_amd.krrn import KRRNPlan
from pose_estimation_amd.runtime import Sync
from pose_estimation_amd.synthetic import init_weights

from write_audit import header_pointer_params

GEOM_BUFS = ("pool_v", "pool_x", "pool_n", "V1", "PV1", "idx1", "nn1", "pool2", "PV2", "idx2", "nn2")


def _plan(monkeypatch, geom):
    monkeypatch.setattr(fusion, "GEOM_EARLY", geom)
    torch.manual_seed(0)
    m = KRRN(cfg=make_config(num_cls=1, backbone="w18"))
    init_weights(m, 0)
    m.eval()
    return KRRNPlan(m, 2, 64, 256, True, torch.device("cpu"))


def _ranges(kp):
    bufs = {k: kp.fusion_bufs[k] for k in GEOM_BUFS}
    bufs.update({k: kp.tbase_bufs[k] for k in ("cnt", "pa", "pb", "slot")})
    return {k: (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for k, t in bufs.items()}


def _touched(op, ranges, params):
    """(buffers the op may write, buffers it only reads), by its pointer arguments' header constness."""
    w_idx, _ = params[op.name]
    wr, rd = set(), set()
    for pos, a in enumerate(op.args[:-1]):
        if not isinstance(a, ctypes.c_void_p) or not a.value:
            continue
        for k, (lo, hi) in ranges.items():
            if lo <= a.value < hi:
                (wr if pos in w_idx else rd).add(k)
    return wr, rd - wr


def test_geometry_launches_are_ordered_through_their_stream(monkeypatch):
    kp = _plan(monkeypatch, True)
    G = fusion.GEOM_SID
    ranges, params = _ranges(kp), header_pointer_params()
    ns = kp.plan.nstreams
    # seen[s][t]: index of the last op of stream t that stream s's next op is ordered after
    seen = [[-1] * ns for _ in range(ns)]
    last = [-1] * ns
    producer, consumers, geom_ops = {}, 0, []
    for k, op in enumerate(kp.plan.ops):
        if isinstance(op, Sync):
            src = list(seen[op.src])
            src[op.src] = last[op.src]
            seen[op.dst] = [max(a, b) for a, b in zip(seen[op.dst], src)]
            continue
        wr, rd = _touched(op, ranges, params)
        for name in rd:
            assert name in producer, (k, op.name, name, "read before any launch wrote it")
            if op.sid != G:
                consumers += 1
                assert seen[op.sid][G] >= producer[name], (k, op.name, op.sid, name, "no sync from the geometry stream")
        for name in wr:
            assert op.sid == G, (k, op.name, name, "written off the geometry stream")
            producer[name] = k
        if op.sid == G:
            geom_ops.append(op.name)
        last[op.sid] = k
    assert set(producer) == set(ranges)
    # 3 pool kNNs + 3 + 1 vertex gathers, idx1, nn1, the pool-2 kNN + gather, idx2, nn2, the pair compaction
    assert sorted(geom_ops) == sorted(["krrn_knn_f32"] * 8 + ["krrn_gather_rows_f32"] * 5 + ["krrn_pair_compact_i32"])
    assert geom_ops[-1] == "krrn_pair_compact_i32"
    assert consumers >= 12  # pool_max x4, the level-1 / level-2 gather-convs, TBase's conv2 and tail
    assert seen[0][G] == last[G] and last[G] > 0, "the geometry stream is not joined before the plan ends"
    # it forks inside the last stage (after the points gather), so both pipeline cuts stay joined
    first = min(k for k, op in enumerate(kp.plan.ops) if not isinstance(op, Sync) and op.sid == G)
    assert first > kp.heads_end > kp.split


def test_knob_off_keeps_the_launches_off_that_stream(monkeypatch):
    on = _plan(monkeypatch, True)
    off = _plan(monkeypatch, False)
    assert not any(op.sid == fusion.GEOM_SID for op in off.plan.ops)
    launches = lambda kp: sorted(op.name for op in kp.plan.ops if not isinstance(op, Sync))  # noqa: E731
    assert launches(on) == launches(off)
    # the pair compaction then follows nn2 on stream 3, which is joined before TBase's conv2 reads the pairs
    ops = off.plan.ops
    k = next(i for i, op in enumerate(ops) if op.name == "krrn_pair_compact_i32")
    assert ops[k].sid == 3 and ops[k - 1].name == "krrn_knn_f32" and ops[k - 1].sid == 3
    c2 = next(i for i, op in enumerate(ops) if op.name == "krrn_gemm_x3_gather_live_f32")
    assert any(isinstance(op, Sync) and (op.src, op.dst) == (3, 0) for op in ops[k:c2])
