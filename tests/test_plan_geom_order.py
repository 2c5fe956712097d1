"""The ordering of the fusion's geometry launches (the ones that read only p9 and the perms: pool kNNs,
sampled-vertex gathers, idx1, idx2, nn1, nn2) and of TBase's pair compaction behind them, checked on a
CPU build of the plan: every launch that reads one of their outputs is ordered after every launch that
wrote it, on its own stream or through a chain of syncs, and every stream they ran on is joined into
stream 0 before the plan ends."""
import ctypes

import torch

from pose_estimation_amd import KRRN, make_config
from pose_estimation_amd.krrn import KRRNPlan
from pose_estimation_amd.runtime import Sync
from pose_estimation_amd.synthetic import init_weights

from write_audit import header_pointer_params

GEOM_BUFS = ("pool_v", "pool_x", "pool_n", "V1", "PV1", "idx1", "nn1", "pool2", "PV2", "idx2", "nn2")


def _plan():
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


def test_geometry_launches_are_ordered_before_their_readers():
    kp = _plan()
    ranges, params = _ranges(kp), header_pointer_params()
    ns = kp.plan.nstreams
    # seen[s][t]: index of the last op of stream t that stream s's next op is ordered after
    seen = [[-1] * ns for _ in range(ns)]
    last = [-1] * ns
    producers, consumers = {}, 0
    for k, op in enumerate(kp.plan.ops):
        if isinstance(op, Sync):
            src = list(seen[op.src])
            src[op.src] = last[op.src]
            seen[op.dst] = [max(a, b) for a, b in zip(seen[op.dst], src)]
            continue
        wr, rd = _touched(op, ranges, params)
        for name in rd:
            assert name in producers, (k, op.name, name, "read before any launch wrote it")
            consumers += not wr  # the launches outside the geometry set
            for pk, psid in producers[name]:  # V1 has one writer per branch stream
                # the same stream runs in order; another stream's writer needs a chain of syncs
                assert psid == op.sid or seen[op.sid][psid] >= pk, \
                    (k, op.name, op.sid, name, f"no sync from its writer {pk} on stream {psid}")
        for name in wr:
            producers.setdefault(name, []).append((k, op.sid))
        last[op.sid] = k
    assert set(producers) == set(ranges)
    assert consumers >= 12  # pool_max x4, the level-1 / level-2 gather-convs, TBase's conv2 and tail
    for sid in {psid for ws in producers.values() for _, psid in ws}:
        assert sid == 0 or (seen[0][sid] == last[sid] and last[sid] > 0), (sid, "not joined before the plan ends")
    # they start inside the last stage (after the points gather), so both pipeline cuts stay joined
    first = min(pk for ws in producers.values() for pk, _ in ws)
    assert first > kp.heads_end > kp.split


def test_pair_compaction_follows_nn2_on_its_stream():
    ops = _plan().plan.ops
    # the pair compaction follows nn2 on stream 3, which is joined before TBase's conv2 reads the pairs
    k = next(i for i, op in enumerate(ops) if op.name == "krrn_pair_compact_i32")
    assert ops[k].sid == 3 and ops[k - 1].name == "krrn_knn_f32" and ops[k - 1].sid == 3
    c2 = next(i for i, op in enumerate(ops) if op.name == "krrn_gemm_x3_gather_live_f32")
    assert any(isinstance(op, Sync) and (op.src, op.dst) == (3, 0) for op in ops[k:c2])
