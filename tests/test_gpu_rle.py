"""krrn_rle_decode_u8 on the GPU against its numpy restatement (tests/rle_ref.py): planes, info rows and the
prefix-sum workspace, all integers, compared exactly. Every output sits inside a sentinel buffer (tests/guarded.py),
so an unwritten byte (the call does no memset) or a stray write shows. Frames: 5 x 3 (smaller than a tile), 16 x 16,
21 x 37 and 41 x 50 (ragged tiles, rows not 16-byte aligned: byte stores), 48 x 64 (aligned rows: 16-byte stores),
480 x 640. Masks: rle_ref.cases."""
import numpy as np
import pytest
import torch

import rle_ref as rf
from guarded import GUARD, Guarded
from pose_estimation_amd import _lib, rle
from pose_estimation_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu


def _raw(dev, runs, H, W):
    """The entry point itself on a list of run lists, every output guarded: (mask, info, ends) as host arrays."""
    counts = np.concatenate([np.asarray(r, np.int32) for r in runs])
    offs = np.cumsum([0] + [len(r) for r in runs]).astype(np.int32)
    n = len(runs)
    cd, od = torch.from_numpy(counts).to(dev), torch.from_numpy(offs).to(dev)
    mask, info = Guarded(dev, (n, H, W), torch.uint8), Guarded(dev, (n, 5), torch.int32)
    ends = Guarded(dev, (len(counts),), torch.int32)
    _lib.call("krrn_rle_decode_u8", ptr(cd), ptr(od), n, H, W, ends.ptr, mask.ptr, info.ptr, stream_ptr(dev))
    torch.cuda.synchronize()
    return mask.get(), info.get(), ends.get()


def _check(tag, got, runs, H, W):
    mask, info, ends = got
    o = 0
    for i, r in enumerate(runs):
        ref = rf.decode(r, H, W)
        print(f"{tag}[{i}]: {len(r)} runs, info {info[i].tolist()}, mask diff {int((mask[i] != ref).sum())}")
        assert np.array_equal(mask[i], ref), (tag, i)
        assert np.array_equal(info[i], rf.info(ref)), (tag, i, info[i].tolist(), rf.info(ref).tolist())
        assert np.array_equal(ends[o:o + len(r)], np.cumsum(r)), (tag, i)
        o += len(r)


@pytest.mark.parametrize("H,W", rf.SIZES)
def test_decode_parity(dev, H, W):
    """Every mask of the size's case list, each decoded alone and all of them in one launch."""
    cases = rf.cases(H, W)
    for name, r in cases:
        _check(f"{H}x{W}/{name}", _raw(dev, [r], H, W), [r], H, W)
    runs = [r for _, r in cases]
    _check(f"{H}x{W}/all", _raw(dev, runs, H, W), runs, H, W)


def test_batch_does_not_change_a_mask(dev):
    """Masks of very different run counts in one launch: each plane and info row equals the mask decoded alone."""
    H, W = 21, 37
    by = dict(rf.cases(H, W))
    runs = [by["zeros"], by["checkerboard"], by["ones"], by[f"runs_{rf.CHUNK}"], by["random"], by["last_pixel"],
            by[f"runs_{2 * rf.CHUNK + 1}"]]
    assert sorted(len(r) for r in runs)[0] == 1 and max(len(r) for r in runs) == H * W + 1
    mask, info, _ = _raw(dev, runs, H, W)
    for i, r in enumerate(runs):
        m1, i1, _ = _raw(dev, [r], H, W)
        assert np.array_equal(mask[i], m1[0]) and np.array_equal(info[i], i1[0]), i
    rev = _raw(dev, runs[::-1], H, W)
    assert np.array_equal(rev[0], mask[::-1]) and np.array_equal(rev[1], info[::-1])


@pytest.mark.parametrize("H,W", [(21, 37), (48, 64)])
def test_binding_and_misaligned_out(dev, H, W):
    """rle.decode: its own allocation, a guarded `out`, and an `out` one byte into a larger buffer (no row starts on
    a 16-byte boundary any more at 48 x 64: byte stores) all hold the same planes; nothing around `out` changes."""
    runs = [r for _, r in rf.cases(H, W)]
    counts, offs = np.concatenate([np.asarray(r) for r in runs]), np.cumsum([0] + [len(r) for r in runs])
    n = len(runs)
    ref = np.stack([rf.decode(r, H, W) for r in runs])
    plain = rle.decode(counts, offs, H, W, dev)
    assert plain["mask"].dtype == torch.uint8 and plain["info"].dtype == torch.int32
    assert tuple(plain["mask"].shape) == (n, H, W) and tuple(plain["info"].shape) == (n, 5)
    g = Guarded(dev, (n, H, W), torch.uint8)
    assert g.view.data_ptr() % 16 == 0
    inside = rle.decode(counts, offs, H, W, dev, out=g.view)
    assert inside["mask"].data_ptr() == g.view.data_ptr()
    big = torch.full((n * H * W + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    off = big[1:1 + n * H * W].view(n, H, W)
    assert off.data_ptr() % 16 == 1 and off.is_contiguous()
    shifted = rle.decode(counts, offs, H, W, dev, out=off)
    torch.cuda.synchronize()
    assert np.array_equal(plain["mask"].cpu().numpy(), ref) and np.array_equal(g.get(), ref)
    assert np.array_equal(off.cpu().numpy(), ref)
    h = big.cpu().numpy()
    assert h[0] == 0xA5 and (h[1 + n * H * W:] == 0xA5).all()
    want = np.stack([rf.info(p) for p in ref])
    for res in (plain, inside, shifted):
        assert np.array_equal(res["info"].cpu().numpy(), want)
    with pytest.raises(ValueError, match="out must be"):
        rle.decode(counts, offs, H, W, dev, out=torch.empty((n, W, H), dtype=torch.uint8, device=dev))


def test_any_counts_stay_inside_the_plane(dev):
    """Runs that do not sum to H * W (the binding refuses them; the entry point must still stay inside its buffers):
    a pixel at or past the total takes the parity of the run count, sums past H * W saturate, a negative count is 0."""
    H, W = 21, 37
    HW = H * W
    short_odd, short_even = [10, 5, 20], [10, 5, 20, 7]              # totals 35 and 42
    long_ = [100, 2 ** 30, 2 ** 30, 2 ** 30, 5]                      # the int32 sum would wrap
    neg = [4, -3, 6, HW]
    runs = [short_odd, short_even, long_, neg]
    mask, info, ends = _raw(dev, runs, H, W)
    flat = lambda i: mask[i].T.reshape(-1)                           # noqa: E731  (column-major pixel order)
    exp = np.zeros(HW, np.uint8)
    exp[10:15] = 1
    exp[35:] = 1                                                     # three runs: odd
    assert np.array_equal(flat(0), exp)
    exp = np.zeros(HW, np.uint8)
    exp[10:15] = 1
    exp[35:42] = 1
    assert np.array_equal(flat(1), exp)
    exp = np.zeros(HW, np.uint8)
    exp[100:] = 1
    assert np.array_equal(flat(2), exp)
    exp = np.zeros(HW, np.uint8)
    exp[4:10] = 0                                                    # runs 4, 0, 6, HW: ones [4, 4) then [10, HW)
    exp[10:] = 1
    assert np.array_equal(flat(3), exp)
    for i in range(4):
        assert np.array_equal(info[i], rf.info(mask[i])), i
    assert ends.tolist() == [10, 15, 35, 10, 15, 35, 42, 100, HW, HW, HW, HW, 4, 4, 10, HW]
