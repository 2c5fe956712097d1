"""The device draws (csrc/rng.hip: krrn_randperm_i32, krrn_randperm_multi_i32, krrn_ransac_subsets,
krrn_rng_advance) against their host restatement tests/draws_ref.py, bit for bit: every kernel here is integer
exact, so there is no tolerance anywhere. Outputs live inside larger sentinel-filled buffers whose elements
before and after the declared extent must come back unchanged."""
import ctypes

import numpy as np
import pytest
import torch

from pose_estimation_amd import _lib
from pose_estimation_amd._lib import P, ptr, stream_ptr
from tests import draws_ref as D
from tests.guarded import Guarded as _Guarded

pytestmark = pytest.mark.gpu

EARG, ESHAPE = -1, -2
NULL = P(0)


class Guarded(_Guarded):
    """int32 [*shape] outputs between sentinel guards; `.ptr` as the ctypes pointer argument."""

    def __init__(self, dev, *shape):
        super().__init__(dev, shape, torch.int32)
        self.ptr = P(self.ptr)


def _seed(dev, value):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def _lib_fn(name):
    return getattr(_lib.lib(), name)


SEEDS = (0, 123, -1)
STREAMS = (0, 5, 2 ** 32 - 1)


@pytest.mark.parametrize("n,k,rows", [(1, 1, 1), (2, 2, 3), (64, 64, 1), (65, 10, 2), (1000, 250, 4), (250, 62, 1),
                                      (1024, 1024, 1), (1025, 1, 1), (4095, 4095, 1), (4096, 4096, 2)])
def test_randperm_matches_restatement(dev, n, k, rows):
    fn, st = _lib_fn("krrn_randperm_i32"), stream_ptr(dev)
    runs = []
    for seed in SEEDS:
        sd = _seed(dev, seed)
        for stream in STREAMS:
            out = Guarded(dev, rows, k)
            assert fn(ptr(sd), stream, n, k, rows, out.ptr, st) == 0
            runs.append((seed, stream, out, sd))
    torch.cuda.synchronize()
    for seed, stream, out, _ in runs:
        got = out.get()
        ref = D.randperm_rows(seed, stream, n, k, rows)
        assert np.array_equal(got, ref), (seed, stream)
        if k == n:
            assert all(sorted(r.tolist()) == list(range(n)) for r in got)


MULTI = [(0, 1000, 250), (1, 1000, 250), (2, 1000, 250), (3, 1000, 250), (4, 250, 62), (7, 4096, 1)]


def _multi_args(draws, outs):
    c = len(draws)
    return ((ctypes.c_uint * c)(*[d[0] for d in draws]), (ctypes.c_int * c)(*[d[1] for d in draws]),
            (ctypes.c_int * c)(*[d[2] for d in draws]), (ctypes.c_void_p * c)(*[o.view.data_ptr() for o in outs]))


def test_randperm_multi_matches_restatement_and_single(dev):
    seed_v = 987654321
    seed, st = _seed(dev, seed_v), stream_ptr(dev)
    singles = [Guarded(dev, k) for _, _, k in MULTI]
    for (sid, n, k), o in zip(MULTI, singles):
        assert _lib_fn("krrn_randperm_i32")(ptr(seed), sid, n, k, 1, o.ptr, st) == 0
    multi = [Guarded(dev, k) for _, _, k in MULTI]
    sids, ns, ks, outs = _multi_args(MULTI, multi)
    assert _lib_fn("krrn_randperm_multi_i32")(ptr(seed), len(MULTI), sids, ns, ks, outs, st) == 0
    torch.cuda.synchronize()
    for (sid, n, k), a, b in zip(MULTI, singles, multi):
        ref = D.randperm(seed_v, sid, 0, n, k)
        assert np.array_equal(b.get(), ref), (sid, n, k)
        assert np.array_equal(a.get(), ref), (sid, n, k)


@pytest.mark.parametrize("B,H,P_", [(1, 1, 5), (3, 100, 256), (2, 257, 6), (1, 300, 4096)])
def test_ransac_subsets_match_restatement(dev, B, H, P_):
    st = stream_ptr(dev)
    runs = []
    for seed, stream in [(0, 0), (123, 1), (-1, 2 ** 32 - 1)]:
        sd = _seed(dev, seed)
        out = Guarded(dev, B, H, 5)
        assert _lib_fn("krrn_ransac_subsets")(ptr(sd), stream, B, H, P_, out.ptr, st) == 0
        runs.append((seed, stream, out, sd))
    torch.cuda.synchronize()
    for seed, stream, out, _ in runs:
        got = out.get()
        assert np.array_equal(got, D.ransac_subsets(seed, stream, B, H, P_)), (seed, stream)
        if P_ == 5:
            assert all(sorted(r.tolist()) == [0, 1, 2, 3, 4] for r in got.reshape(-1, 5))


def test_ransac_subsets_p5_rows_are_permutations(dev):
    """P = 5 leaves the rejection loop no choice: every one of B*H = 600 rows (a partial last block of 256) is
    a permutation of 0..4, and equals the restatement's."""
    sd, out = _seed(dev, 42), Guarded(dev, 2, 300, 5)
    assert _lib_fn("krrn_ransac_subsets")(ptr(sd), 6, 2, 300, 5, out.ptr, stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    got = out.get()
    assert all(sorted(r.tolist()) == [0, 1, 2, 3, 4] for r in got.reshape(-1, 5))
    assert np.array_equal(got, D.ransac_subsets(42, 6, 2, 300, 5))


@pytest.mark.parametrize("seed", [41, -1, 2 ** 63 - 1])
def test_rng_advance(dev, seed):
    """After one advance the draws are the restatement's at seed + 1 (modulo 2^64: -1 advances to 0)."""
    sd, st = _seed(dev, seed), stream_ptr(dev)
    assert _lib_fn("krrn_rng_advance")(ptr(sd), st) == 0
    perm, subs = Guarded(dev, 2, 10), Guarded(dev, 1, 20, 5)
    assert _lib_fn("krrn_randperm_i32")(ptr(sd), 3, 65, 10, 2, perm.ptr, st) == 0
    assert _lib_fn("krrn_ransac_subsets")(ptr(sd), 4, 1, 20, 50, subs.ptr, st) == 0
    torch.cuda.synchronize()
    nxt = D.advance(seed)
    assert int(sd.item()) == nxt
    if seed == -1:
        assert nxt == 0
    assert np.array_equal(perm.get(), D.randperm_rows(nxt, 3, 65, 10, 2))
    assert np.array_equal(subs.get(), D.ransac_subsets(nxt, 4, 1, 20, 50))


def test_graph_replay_draws_consecutive_seeds(dev):
    """A linear single-stream [randperm, subsets, advance] captured once: replay r draws the restatement at
    seed + r, and the seed ends at seed + 3."""
    seed0 = -2  # the replays cross -1 -> 0
    sd = _seed(dev, seed0)
    perm, subs = Guarded(dev, 2, 250), Guarded(dev, 2, 40, 5)

    def step():
        st = stream_ptr(dev)
        assert _lib_fn("krrn_randperm_i32")(ptr(sd), 0, 1000, 250, 2, perm.ptr, st) == 0
        assert _lib_fn("krrn_ransac_subsets")(ptr(sd), 6, 2, 40, 250, subs.ptr, st) == 0
        assert _lib_fn("krrn_rng_advance")(ptr(sd), st) == 0

    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert int(sd.item()) == seed0  # capturing runs nothing
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        sv = D.advance(seed0, r)
        assert np.array_equal(perm.get(), D.randperm_rows(sv, 0, 1000, 250, 2)), r
        assert np.array_equal(subs.get(), D.ransac_subsets(sv, 6, 2, 40, 250)), r
        assert int(sd.item()) == D.advance(seed0, r + 1)
    assert int(sd.item()) == seed0 + 3


def test_host_rejects_leave_outputs_untouched(dev):
    """Arguments out of range are refused on the host with the header's codes (KRRN_EARG null pointer,
    KRRN_ESHAPE size), before any launch: the output keeps its sentinel."""
    sd, st = _seed(dev, 5), stream_ptr(dev)
    out = Guarded(dev, 4096 * 2)
    rp, sub, adv = _lib_fn("krrn_randperm_i32"), _lib_fn("krrn_ransac_subsets"), _lib_fn("krrn_rng_advance")
    for n, k, rows in [(0, 1, 1), (4097, 1, 1), (10, 0, 1), (10, 11, 1), (10, 5, 0), (-1, 1, 1), (10, 5, -1)]:
        assert rp(ptr(sd), 0, n, k, rows, out.ptr, st) == ESHAPE, (n, k, rows)
    assert rp(NULL, 0, 10, 5, 1, out.ptr, st) == EARG
    assert rp(ptr(sd), 0, 10, 5, 1, NULL, st) == EARG
    for B, H, P_ in [(1, 1, 4), (0, 1, 5), (1, 0, 5), (-1, 1, 5), (1, 1, 0)]:
        assert sub(ptr(sd), 0, B, H, P_, out.ptr, st) == ESHAPE, (B, H, P_)
    assert sub(NULL, 0, 1, 1, 5, out.ptr, st) == EARG
    assert sub(ptr(sd), 0, 1, 1, 5, NULL, st) == EARG
    assert adv(NULL, st) == EARG

    multi = _lib_fn("krrn_randperm_multi_i32")
    draws = [(0, 100, 10), (1, 50, 50)]
    outs_g = [Guarded(dev, 10), Guarded(dev, 50)]
    sids, ns, ks, outs = _multi_args(draws, outs_g)
    assert multi(ptr(sd), 0, sids, ns, ks, outs, st) == ESHAPE
    nine = [(q, 10, 5) for q in range(9)]
    nine_g = [Guarded(dev, 5) for _ in nine]
    assert multi(ptr(sd), 9, *_multi_args(nine, nine_g), st) == ESHAPE
    for bad in [(0, 0, 1), (0, 4097, 1), (0, 10, 0), (0, 10, 11)]:
        assert multi(ptr(sd), 2, *_multi_args([draws[0], bad], outs_g), st) == ESHAPE, bad
    null_out = (ctypes.c_void_p * 2)(outs_g[0].view.data_ptr(), None)
    assert multi(ptr(sd), 2, sids, ns, ks, null_out, st) == EARG
    for i in range(5):
        args = [ptr(sd), sids, ns, ks, outs]
        args[i] = NULL
        assert multi(args[0], 2, *args[1:], st) == EARG, i
    torch.cuda.synchronize()
    assert out.untouched() and all(o.untouched() for o in outs_g + nine_g)
    assert int(sd.item()) == 5
