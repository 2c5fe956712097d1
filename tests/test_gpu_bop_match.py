"""krrn_bop_match_f64 on the GPU against its numpy restatement (tests/bop_match_ref.py) on the kernel's own inputs.
The matching is discrete: every comparison is exact. One call holds groups of (n_est, n_gt) = (1, 1), (0, 2), (2, 0),
(0, 0), (3, 2), (2, 3), (5, 5), (65, 63) (a second wave of estimates, instances around the 64-bit word of the matched
set) and (128, 128) (both limits), at C x NT = 3 x 1, 12 x 10 and 18 x 16 cells (fewer cells than a wave, fewer
than a block, more than a block's 256 threads). Errors, thresholds and scores come from small value sets, so error
ties, score ties and error == threshold occur all over; NaN, +inf and -inf errors, a NaN score and an inf threshold
are among them. Outputs sit in sentinel buffers (tests/guarded.py): an element the call leaves unwritten, or a
write outside the extent, shows."""
import functools

import numpy as np
import pytest
import torch

import bop_match_ref as mr
from guarded import Guarded
from pose_estimation_amd import _lib, bop
from pose_estimation_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (0, 2), (2, 0), (0, 0), (3, 2), (2, 3), (5, 5), (65, 63), (128, 128))
N_TOP = (1, 2, 1, 0, 2, 0, 3, 63, -1)                     # below, at and above n_est, and "all"
CELLS = ((3, 1), (12, 10), (18, 16))
ERR = np.array([0.0, 0.05, 0.1, 0.1, 0.2, 0.3, 0.5, 0.7, np.nan, np.inf, -np.inf])
THR = np.array([0.05, 0.1, 0.2, 0.3, 0.5, np.inf])
SCORE = np.array([0.1, 0.5, 0.5, 0.9, 0.9, 1.0, np.nan, -1.0])
SENTINEL = -7777


@functools.lru_cache(maxsize=None)
def inputs(C, NT):
    rng = np.random.default_rng(100 * C + NT)
    ne, ng = np.array([s[0] for s in SHAPES]), np.array([s[1] for s in SHAPES])
    e0, g0 = np.concatenate([[0], np.cumsum(ne)]), np.concatenate([[0], np.cumsum(ng)])
    p0 = np.concatenate([[0], np.cumsum(ne * ng)])
    a = {"score": SCORE[rng.integers(0, len(SCORE), e0[-1])], "err": ERR[rng.integers(0, len(ERR), (p0[-1], C))],
         "est_range": np.stack([e0[:-1], ne], 1).astype(np.int32), "gt_range": np.stack([g0[:-1], ng], 1).astype(np.int32),
         "pair_off": p0[:-1].astype(np.int32), "thr": THR[rng.integers(0, len(THR), (len(SHAPES), C, NT))],
         "n_top": np.array(N_TOP, np.int32), "n_inst": int(g0[-1])}
    assert np.isnan(a["score"]).any() and len(set(a["score"][~np.isnan(a["score"])])) < e0[-1]
    assert np.isnan(a["err"]).any() and np.isinf(a["err"]).any()
    for v in a.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(C, NT):
    a = inputs(C, NT)
    match, tp = mr.match_poses(a["score"], a["err"], a["est_range"], a["gt_range"], a["pair_off"], a["thr"], a["n_top"],
                               a["n_inst"], fill=SENTINEL)
    match.setflags(write=False), tp.setflags(write=False)
    return match, tp


def _raw(dev, a, max_est=128, max_gt=128):
    """The entry point itself, both outputs guarded: (match, tp) as host arrays."""
    G, C, NT = a["thr"].shape
    t = {k: torch.tensor(a[k]).to(dev) for k in ("score", "err", "est_range", "gt_range",
                                                                           "pair_off", "thr", "n_top")}
    match, tp = Guarded(dev, (a["n_inst"], C, NT), torch.int32), Guarded(dev, (G, C, NT), torch.int32)
    _lib.call("krrn_bop_match_f64", ptr(t["score"]), len(a["score"]), ptr(t["err"]), len(a["err"]), C,
              ptr(t["est_range"]), ptr(t["gt_range"]), ptr(t["pair_off"]), ptr(t["thr"]), NT, ptr(t["n_top"]), G,
              a["n_inst"], max_est, max_gt, match.ptr, tp.ptr, stream_ptr(dev))
    torch.cuda.synchronize()
    return match.get(), tp.get()


def _group(a, g):
    """Group g of `a` as a call of its own."""
    (e0, ne), (g0, ng), p0 = a["est_range"][g], a["gt_range"][g], a["pair_off"][g]
    return {"score": a["score"][e0:e0 + ne], "err": a["err"][p0:p0 + ne * ng],
            "est_range": np.array([[0, ne]], np.int32), "gt_range": np.array([[0, ng]], np.int32),
            "pair_off": np.zeros(1, np.int32), "thr": a["thr"][g:g + 1], "n_top": a["n_top"][g:g + 1], "n_inst": int(ng)}


@pytest.mark.parametrize("C,NT", CELLS)
def test_kernel_equals_restatement(dev, C, NT):
    a = inputs(C, NT)
    match, tp = _raw(dev, a)
    want_m, want_t = reference(C, NT)
    print(f"C {C} NT {NT}: tp sum {int(tp.sum())} (ref {int(want_t.sum())}), match diff {int((match != want_m).sum())}, "
          f"tp diff {int((tp != want_t).sum())}")
    assert (match != SENTINEL).all() and (tp != SENTINEL).all()          # every element is written
    assert np.array_equal(tp, want_t) and np.array_equal(match, want_m)
    assert 0 < tp[-1].max() <= 128 and tp[1].max() == 0 and tp[2].max() == 0 and (match[1:3] == -1).all()


def test_batch_independence(dev):
    """Each group alone equals its slice of the batched run; permuting the groups permutes tp and leaves every
    instance's row where its range puts it."""
    C, NT = 12, 10
    a = inputs(C, NT)
    match, tp = reference(C, NT)
    for g in range(len(SHAPES)):
        m1, t1 = _raw(dev, _group(a, g))
        g0, ng = a["gt_range"][g]
        assert np.array_equal(t1[0], tp[g]), g
        e0 = a["est_range"][g][0]
        assert np.array_equal(np.where(m1 >= 0, m1 + e0, -1), match[g0:g0 + ng]), g
    perm = np.random.default_rng(9).permutation(len(SHAPES))
    b = dict(a, **{k: a[k][perm] for k in ("est_range", "gt_range", "pair_off", "thr", "n_top")})
    m2, t2 = _raw(dev, b)
    assert np.array_equal(t2, tp[perm]) and np.array_equal(m2, match)


def test_stated_limits_and_bad_ranges(dev):
    """max_est / max_gt below a group's sizes, estimates past Etot, pair rows past Ptot, negative ranges: such a group is
    matched as one without estimates; an instance range that leaves [0, GTtot) owns nothing. Nothing outside the
    buffers is written (the guards) and the rest of the batch is untouched."""
    C, NT = 12, 10
    a = inputs(C, NT)
    for kw in (dict(max_est=4, max_gt=128), dict(max_est=128, max_gt=4), dict(max_est=0, max_gt=0)):
        want_m, want_t = mr.match_poses(a["score"], a["err"], a["est_range"], a["gt_range"], a["pair_off"], a["thr"],
                                        a["n_top"], a["n_inst"], fill=SENTINEL, **kw)
        m, t = _raw(dev, a, **kw)
        assert np.array_equal(m, want_m) and np.array_equal(t, want_t), kw
        assert t[-1].max() == 0 and (kw["max_est"] == 0 or t[4].max() > 0)
    b = dict(a, est_range=a["est_range"].copy(), gt_range=a["gt_range"].copy(), pair_off=a["pair_off"].copy())
    b["est_range"][4] = (len(a["score"]) - 1, 3)         # past Etot
    b["pair_off"][5] = len(a["err"]) - 2                 # its 6 rows end past Ptot
    b["est_range"][6] = (-1, 5)
    b["gt_range"][7] = (a["n_inst"] - 10, 63)            # leaves the instance axis: owns nothing
    b["gt_range"][0] = (0, -1)
    b["pair_off"][8] = -1
    want_m, want_t = mr.match_poses(b["score"], b["err"], b["est_range"], b["gt_range"], b["pair_off"], b["thr"], b["n_top"],
                                    b["n_inst"], fill=SENTINEL)
    m, t = _raw(dev, b)
    assert np.array_equal(m, want_m) and np.array_equal(t, want_t)
    assert not t[[0, 4, 5, 6, 7, 8]].any() and (m[0] == SENTINEL).all()


def test_wrapper(dev):
    """bop.match_poses on host tensors: the same outputs, on the device; the instance axis is the caller's."""
    C, NT = 3, 1
    a = inputs(C, NT)
    want_m, want_t = reference(C, NT)
    host = {k: torch.tensor(a[k]) for k in ("score", "err", "est_range", "gt_range", "pair_off",
                                                                     "thr", "n_top")}
    out = bop.match_poses(**host, n_inst=a["n_inst"], device=dev)
    assert out["match"].is_cuda and out["match"].dtype == torch.int32 and out["tp"].shape == (len(SHAPES), C, NT)
    assert np.array_equal(out["match"].cpu().numpy(), want_m) and np.array_equal(out["tp"].cpu().numpy(), want_t)
    on_dev = bop.match_poses(**{k: v.to(dev) for k, v in host.items()}, n_inst=a["n_inst"])
    assert torch.equal(on_dev["match"], out["match"]) and torch.equal(on_dev["tp"], out["tp"])
    with pytest.raises(RuntimeError, match="HIP path only"):
        bop.match_poses(**host, n_inst=a["n_inst"])
