"""Run-length encoded masks without a GPU: the compressed string codec of pose_estimation_amd/rle.py against the
two literal vectors and against the independent codec of tests/rle_ref.py, encode / box_counts against the numpy
restatement, every refusal of rle.decode (raised before a device is touched, so no GPU is needed), and the
host-side argument checks and ABI signature of krrn_rle_decode_u8."""
import ctypes

import numpy as np
import pytest

import rle_ref as rf
from pose_estimation_amd import _lib, rle


@pytest.mark.parametrize("counts,text", rf.VECTORS)
def test_string_vectors(counts, text):
    assert rle.counts_to_string(counts) == text and rle.counts_from_string(text) == counts
    assert rf.to_string(counts) == text and rf.from_string(text) == counts     # the restatement agrees on them


def test_string_round_trips():
    """Counts >= 16 take two characters, >= 512 three; from the fourth value on a delta may be negative."""
    assert [len(rle.counts_to_string([v])) for v in (0, 15, 16, 511, 512, 16383, 16384)] == [1, 1, 2, 2, 3, 3, 4]
    assert len(rle.counts_to_string([5, 5, 5, 1000, 5, 2])) == 3 + 3 + 1 + 3   # 5 5 5, then +995, 0, -998
    seen = 0
    for H, W in rf.SIZES[:5]:
        for name, c in rf.cases(H, W):
            s = rle.counts_to_string(c)
            assert s == rf.to_string(c), (H, W, name)
            assert rle.counts_from_string(s) == c == rf.from_string(s), (H, W, name)
            assert all(48 <= ord(ch) < 112 for ch in s)
            seen += 1
    assert seen >= 35
    rng = np.random.default_rng(3)
    for _ in range(50):
        c = [int(v) for v in rng.integers(0, 2 ** int(rng.integers(1, 31)), size=int(rng.integers(1, 40)))]
        assert rle.counts_from_string(rle.counts_to_string(c)) == c and rle.counts_to_string(c) == rf.to_string(c)
    with pytest.raises(ValueError, match="ends inside"):
        rle.counts_from_string("61X")                    # 'X' announces another character
    with pytest.raises(ValueError, match="outside"):
        rle.counts_from_string("6 1")


def test_encode_and_box_counts():
    for H, W in rf.SIZES[:5]:
        for name, c in rf.cases(H, W):
            plane = rf.decode(c, H, W)
            got = rle.encode(plane)
            assert got == rf.encode(plane), (H, W, name)
            assert np.array_equal(rf.decode(got, H, W), plane) and 0 not in got[1:]    # no interior zero run is made
    assert rle.encode(np.zeros((4, 3))) == [12] and rle.encode(np.ones((4, 3), bool)) == [0, 12]
    assert rle.encode(np.array([[0, 7], [255, 0]], np.uint8)) == [1, 2, 1]             # column-major; non-zero = set
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        rle.encode(np.zeros((2, 2, 2)))
    H, W = 21, 37
    for x, y, w, h in ((3, 4, 10, 6), (-5, -2, 9, 30), (30, 15, 20, 20), (0, 0, 37, 21), (2.4, 3.6, 4.2, 1.0)):
        ref = np.zeros((H, W), np.uint8)
        x0, x1 = max(0, int(round(x))), min(W, int(round(x + w)))
        y0, y1 = max(0, int(round(y))), min(H, int(round(y + h)))
        ref[y0:y1, x0:x1] = 1
        assert ref.any()
        assert np.array_equal(rf.decode(rle.box_counts(x, y, w, h, H, W), H, W), ref), (x, y, w, h)
    for x, y, w, h in ((40, 0, 5, 5), (0, 25, 5, 5), (3, 3, 0, 5), (-9, 0, 4, 4)):      # nothing left inside the frame
        assert rle.box_counts(x, y, w, h, H, W) == [H * W]


def test_decode_refuses_bad_input():
    """Every ValueError of rle.decode, before any launch: the device named here does not have to exist."""
    H, W = 4, 3
    ok = [5, 3, 4]
    with pytest.raises(ValueError, match="mask 1 has a negative count"):
        rle.decode(ok + [13, -1], [0, 3, 5], H, W, "cuda:0")
    with pytest.raises(ValueError, match=r"mask 1: its runs sum to 11, not H \* W = 12"):
        rle.decode(ok + [5, 6], [0, 3, 5], H, W, "cuda:0")
    with pytest.raises(ValueError, match="mask 0: its runs sum to 13"):
        rle.decode([5, 3, 5], [0, 3], H, W, "cuda:0")
    with pytest.raises(ValueError, match="mask 1 has no run"):
        rle.decode(ok + ok, [0, 3, 3, 6], H, W, "cuda:0")
    with pytest.raises(ValueError, match="mask 1: offs is not increasing"):
        rle.decode(ok + ok, [0, 3, 2, 6], H, W, "cuda:0")
    with pytest.raises(ValueError, match="mask 1: its runs 3 .. 7 lie outside the 6 counts"):
        rle.decode(ok + ok, [0, 3, 7], H, W, "cuda:0")
    with pytest.raises(ValueError, match="mask 0: its runs -1"):
        rle.decode(ok, [-1, 3], H, W, "cuda:0")
    with pytest.raises(ValueError, match="positive"):
        rle.decode(ok, [0, 3], 0, 12, "cuda:0")
    with pytest.raises(ValueError, match="int32"):
        rle.decode(ok, [0, 3], 65536, 32768, "cuda:0")
    with pytest.raises(RuntimeError, match="HIP path only"):
        rle.decode(ok, [0, 3], H, W, "cpu")              # valid input, but no host fallback


def test_rle_host_side_errors():
    fn = _lib.lib().krrn_rle_decode_u8
    N = ctypes.c_void_p(0)
    names = ("counts", "offs", "ends", "mask", "info")

    def call(n=2, H=48, W=64, **over):
        p = {k: ctypes.c_void_p((i + 1) << 36) for i, k in enumerate(names)}   # never dereferenced
        p.update(over)
        return fn(p["counts"], p["offs"], n, H, W, p["ends"], p["mask"], p["info"], N)

    for k in names:
        assert call(**{k: N}) == -1, k
    assert call(n=-1) == -2 and call(H=0) == -2 and call(H=-3) == -2 and call(W=0) == -2 and call(W=-1) == -2
    assert call(H=65536, W=32768) == -2 and call(H=46341, W=46341) == -2      # H * W = 2^31 and just above it
    assert call(n=0) == 0                                 # nothing to do: returns before any HIP call
    assert call(n=0, H=32768, W=65535) == 0               # H * W = 2^31 - 32768 fits
    assert call(n=0, info=N) == -1 and call(n=0, H=0) == -2   # pointers, then shapes, are checked first


def test_abi_lists_the_entry_point():
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["krrn_rle_decode_u8"] == [P, P, I, I, I, P, P, P, P]
