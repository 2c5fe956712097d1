"""krrn_mask_paste_f32 on the GPU against tests/paste_ref.py, exactly (integer output from IEEE comparisons: no
tolerance applies). `mask` and `info` sit inside sentinel buffers (tests/guarded.py), so a byte the call leaves
unwritten or a write outside the extent shows. Frames 37 x 53 (no multiple of the 16 x 16 tile either way: cut rows,
byte stores) and 48 x 64 (whole tiles, 16-byte stores); windows of 1, 5, 16, 17 and 40 pixels (40 = the smallest
production crop, 2.5 tiles)."""
import numpy as np
import pytest
import torch

import paste_ref as pr
import rle_ref as rf
from guarded import Guarded
from pose_estimation_amd import _lib, rle
from pose_estimation_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu

FRAMES = ((37, 53), (48, 64))
SIZES = (1, 5, 16, 17, 40)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _i32(dev, v, shape):
    return torch.from_numpy(np.asarray(v, np.int64).astype(np.int32).reshape(shape)).to(dev)


def _raw(dev, logits, chan, rc, H, W, shift=0):
    """The entry point itself on a device tensor f32 [B, C1, S, S] (possibly a channel slice), every output guarded:
    (mask [B, H, W], info [B, 5]) as host arrays. shift: the plane starts that many bytes into its guarded buffer."""
    B, C1, S, _ = logits.shape
    assert logits.stride()[1:] == (S * S, S, 1) and logits.is_cuda and logits.dtype == torch.float32
    mask, info = Guarded(dev, (B * H * W + shift,), torch.uint8), Guarded(dev, (B, 5), torch.int32)
    cd, rd = _i32(dev, chan, (B,)), _i32(dev, rc, (B, 2))
    _lib.call("krrn_mask_paste_f32", ptr(logits), int(logits.stride(0)), C1, S, ptr(cd), ptr(rd), B, H, W,
              mask.ptr + shift, info.ptr, stream_ptr(dev))
    torch.cuda.synchronize()
    m = mask.get()
    assert (m[:shift] == mask.sentinel).all()
    return m[shift:].reshape(B, H, W), info.get()


def _check(tag, got, logits, chan, rc, H, W):
    want = pr.paste(logits, chan, rc, H, W)
    diff = int((got[0] != want[0]).sum())
    print(f"{tag}: {len(chan)} crops, {int(want[0].sum())} px set, {diff} bytes differ, "
          f"info rows differing {int((got[1] != want[1]).any(1).sum())}")
    assert diff == 0, tag
    assert np.array_equal(got[1], want[1]), (tag, got[1].tolist(), want[1].tolist())
    return want


def _logits(seed, B, C1, S):
    return np.random.default_rng(seed).standard_normal((B, C1, S, S)).astype(np.float32)


def _placements(S, H, W):
    """(rmin, cmin), then how many of the last ones lie wholly outside the frame."""
    out = [(0, 0), (H - S, W - S), (2, 7), (1, 17),                  # corner, flush bottom right, odd cmin twice
           (-((S + 1) // 2), 3), (H - S // 2 - 1, 5), (3, -((S + 1) // 2)), (4, W - S // 2 - 1),   # cut by each border
           (-((S + 1) // 2), W - S // 2 - 1),                        # and by two at once
           (H, 0), (0, -S), (-S, W), (I32_MIN, I32_MAX), (I32_MAX, I32_MIN), (I32_MAX, 0), (0, I32_MIN)]
    return out, 7


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("S", SIZES)
def test_window_placement(dev, H, W, S):
    rc, n_out = _placements(S, H, W)
    B = len(rc)
    l = _logits(100 * S + H, B, 2, S)
    l[:, 1] += 0.5                                       # a little more foreground than background
    chan = [1] * B
    got = _raw(dev, torch.from_numpy(l).to(dev), chan, rc, H, W)
    want = _check(f"{H}x{W} S={S}", got, l, chan, rc, H, W)
    assert not got[0][B - n_out:].any() and not got[1][B - n_out:].any()     # wholly outside: zeros, five zeros
    if S >= 5:                                           # a 1 x 1 window cannot be cut: it is inside or outside
        assert want[0][:B - n_out].any(1).any(1).all()


@pytest.mark.parametrize("H,W", FRAMES)
def test_out_at_an_odd_address(dev, H, W):
    """The plane one byte into a larger buffer, so no row starts on a 16-byte boundary: byte stores give what the
    aligned plane gets, through the entry point and through rle.paste_masks(out=...)."""
    S, B = 17, 4
    rc = [(0, 0), (H - S, W - S), (5, 16), (-3, 31)]
    l = _logits(7, B, 2, S)
    chan = [1, 0, 1, 1]
    dl = torch.from_numpy(l).to(dev)
    aligned, shifted = _raw(dev, dl, chan, rc, H, W), _raw(dev, dl, chan, rc, H, W, shift=1)
    _check("aligned", aligned, l, chan, rc, H, W)
    _check("shifted", shifted, l, chan, rc, H, W)
    big = torch.full((B * H * W + 2,), 0xA5, dtype=torch.uint8, device=dev)
    out = big[1:1 + B * H * W].view(B, H, W)
    assert out.data_ptr() % 16 == 1 and out.is_contiguous()
    res = rle.paste_masks(dl, chan, rc, H, W, out=out)
    assert res["mask"].data_ptr() == out.data_ptr() and res["info"].dtype == torch.int32
    host = big.cpu().numpy()
    assert host[0] == 0xA5 and host[-1] == 0xA5
    assert np.array_equal(host[1:-1].reshape(B, H, W), aligned[0]) and np.array_equal(res["info"].cpu().numpy(), aligned[1])
    plain = rle.paste_masks(dl, torch.tensor(chan, dtype=torch.int32, device=dev),
                            torch.tensor(rc, dtype=torch.int32, device=dev), H, W)   # device operands, own plane
    assert np.array_equal(plain["mask"].cpu().numpy(), aligned[0]) and tuple(plain["info"].shape) == (B, 5)


@pytest.mark.parametrize("shift", [0, 1])
def test_wide_frame(dev, shift):
    """37 x 272: two full spans of 8 tiles and a cut one a tile row, so whole spans the window misses take the span
    store (not with the plane one byte off alignment); windows inside one span, across two, in the cut one, and two
    that miss the frame or select nothing."""
    H, W, S = 37, 272, 17
    rc = [(3, 5), (10, 120), (20, 250), (-8, 111), (25, 128), (0, 0), (H, 0)]
    chan = [1, 1, 0, 1, 1, 2, 1]
    l = _logits(51, len(rc), 2, S)
    got = _raw(dev, torch.from_numpy(l).to(dev), chan, rc, H, W, shift=shift)
    want = _check(f"wide shift={shift}", got, l, chan, rc, H, W)
    assert want[0][:5].any(1).any(1).all() and not want[0][5:].any()


def test_batch_stride(dev):
    """Logits as the channel slice [:, 0:C1] of a wider tensor (what pred["mask"] is): ld_b > C1 S S, no copy."""
    H, W, S, B, C1 = 37, 53, 17, 3, 4
    wide = torch.from_numpy(_logits(11, B, 9, S)).to(dev)
    view = wide[:, 0:C1]
    assert not view.is_contiguous() and view.stride(0) == 9 * S * S and view.data_ptr() == wide.data_ptr()
    chan, rc = [2, 0, 3], [(3, 5), (-4, 40), (25, 0)]
    l = view.cpu().numpy()
    a = _raw(dev, view, chan, rc, H, W)
    b = _raw(dev, view.contiguous(), chan, rc, H, W)
    _check("slice", a, l, chan, rc, H, W)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    res = rle.paste_masks(view, chan, rc, H, W)
    assert np.array_equal(res["mask"].cpu().numpy(), a[0]) and np.array_equal(res["info"].cpu().numpy(), a[1])


@pytest.mark.parametrize("C1", [1, 2, 4])
def test_channels(dev, C1):
    """chan = every foreground channel, 0 (any foreground), C1 and -1 (nothing), on the same logits."""
    H, W, S = 37, 53, 16
    chans = list(range(-1, C1 + 1)) + [I32_MAX, I32_MIN]
    B = len(chans)
    l = np.repeat(_logits(20 + C1, 1, C1, S), B, 0)
    rc = [(9, 21)] * B
    got = _raw(dev, torch.from_numpy(l).to(dev), chans, rc, H, W)
    _check(f"C1={C1}", got, l, chans, rc, H, W)
    by = dict(zip(chans, got[0]))
    assert not by[-1].any() and not by[C1].any() and not by[I32_MAX].any() and not by[I32_MIN].any()
    if C1 > 1:
        assert all(by[c].any() for c in range(1, C1))
        assert np.array_equal(by[0], np.maximum.reduce([by[c] for c in range(1, C1)]))   # any foreground = their union
    else:
        assert not by[0].any()


def test_crafted_logits(dev):
    """Ties, signed zeros, infinities and NaNs: one pixel per vector [l0, l1, l2], then whole-window NaN cases."""
    nan, inf = float("nan"), float("inf")
    vec = [([0.0, 1.0, 1.0], 1), ([1.0, 1.0, 0.0], 0), ([2.0, 1.0, 2.0], 0), ([-0.0, 0.0, -1.0], 0), ([0.0, -0.0, 0.0], 0),
           ([-1.0, -0.0, 0.0], 1), ([-inf, -inf, -inf], 0), ([-inf, inf, inf], 1), ([inf, inf, 0.0], 0), ([-inf, 0.0, inf], 2),
           ([nan, 5.0, 6.0], 0), ([0.0, nan, -1.0], 0), ([0.0, nan, 1.0], 2), ([-1.0, -0.5, nan], 1), ([nan, nan, nan], 0),
           ([0.0, 1.0, 2.0], 2)]
    S, H, W = 4, 37, 53
    l = np.asarray([v for v, _ in vec], np.float32).T.reshape(1, 3, S, S).copy()
    assert pr.decide(l[0]).reshape(-1).tolist() == [b for _, b in vec]
    all_nan, nan0, nan_wanted = np.full_like(l, nan), l.copy(), l.copy()
    nan0[0, 0], nan_wanted[0, 1] = nan, nan
    cases = [(l, 0), (l, 1), (l, 2), (all_nan, 0), (all_nan, 1), (nan0, 0), (nan0, 2), (nan_wanted, 1), (nan_wanted, 2)]
    logits = np.concatenate([c for c, _ in cases])
    chan = [ch for _, ch in cases]
    rc = [(30, 47)] * len(cases)                         # rows 30 .. 33, columns 47 .. 50: across the cut tiles
    got = _raw(dev, torch.from_numpy(logits).to(dev), chan, rc, H, W)
    _check("crafted", got, logits, chan, rc, H, W)
    assert [int(g.sum()) for g in got[0][3:8]] == [0, 0, 0, 0, 0]
    assert got[0][1][30:34, 47:51].reshape(-1).tolist() == [int(b == 1) for _, b in vec]


def test_single_set_pixel(dev):
    H, W, S = 48, 64, 17
    l = np.zeros((2, 2, S, S), np.float32)
    l[0, 1, 16, 0] = 1.0                                 # lands on frame pixel (row 47, column 63): the last one
    l[1, 1, 3, 4] = np.float32(1e-45)                    # the smallest subnormal still beats 0
    rc = [(31, 63), (10, 20)]
    got = _raw(dev, torch.from_numpy(l).to(dev), [1, 0], rc, H, W)
    _check("single", got, l, [1, 0], rc, H, W)
    assert got[1].tolist() == [[1, 63, 47, 0, 0], [1, 24, 13, 0, 0]]


def test_checkerboard_window(dev):
    """An 80 x 80 checkerboard in a 96 x 100 frame: the planes, and encode_planes of them although the run count is
    far past encode_gpu's default slot min(H W + 1, 8 W + 1) = 801."""
    H, W, S = 96, 100, 80
    yy, xx = np.mgrid[0:S, 0:S]
    board = np.where((yy + xx) & 1, 1.0, -1.0).astype(np.float32)
    l = np.stack([np.stack([np.zeros_like(board), board]), np.stack([np.zeros_like(board), -board])])
    rc = [(9, 13), (16, 20)]
    dl = torch.from_numpy(l).to(dev)
    got = _raw(dev, dl, [1, 1], rc, H, W)
    want = _check("checkerboard", got, l, [1, 1], rc, H, W)
    assert got[1].tolist() == [[3200, 13, 9, 79, 79], [3200, 20, 16, 79, 79]]
    res = rle.paste_masks(dl, [1, 1], rc, H, W)
    runs = rle.encode_planes(res["mask"])
    refs = [rle.encode(p) for p in want[0]]
    print("runs per mask:", [len(r) for r in refs], "default slot", min(H * W + 1, 8 * W + 1))
    assert min(len(r) for r in refs) > 6000 > min(H * W + 1, 8 * W + 1) == 801
    assert runs == refs


def test_batch_does_not_change_a_crop(dev):
    """A crop pasted alone and as one of 5 mixed crops: identical bytes and info."""
    H, W, S, C1 = 37, 53, 17, 3
    l = _logits(31, 5, C1, S)
    l[3, :, 2, :] = float("nan")
    chan = [1, 2, 0, 1, 3]
    rc = [(0, 0), (25, 40), (-5, 17), (10, 3), (1, 1)]
    dl = torch.from_numpy(l).to(dev)
    together = _raw(dev, dl, chan, rc, H, W)
    _check("together", together, l, chan, rc, H, W)
    rev = _raw(dev, torch.from_numpy(l[::-1].copy()).to(dev), chan[::-1], rc[::-1], H, W)
    assert np.array_equal(rev[0][::-1], together[0]) and np.array_equal(rev[1][::-1], together[1])
    for i in range(5):
        alone = _raw(dev, dl[i:i + 1], chan[i:i + 1], rc[i:i + 1], H, W)
        assert np.array_equal(alone[0][0], together[0][i]) and np.array_equal(alone[1][0], together[1][i]), i


def test_round_trip(dev):
    """rle.decode(encode_planes(paste)) is the paste, and the decoder's info rows are the paste's."""
    H, W, S = 37, 53, 40
    l = _logits(41, 3, 2, S)
    rc = [(0, 0), (-3, 13), (20, 30)]
    res = rle.paste_masks(torch.from_numpy(l).to(dev), [1, 1, 0], rc, H, W)
    want = pr.paste(l, [1, 1, 0], rc, H, W)
    assert np.array_equal(res["mask"].cpu().numpy(), want[0])
    runs = rle.encode_planes(res["mask"])
    assert runs == [rle.encode(p) for p in want[0]] == [rf.encode(p) for p in want[0]]
    back = rle.decode(np.concatenate([np.asarray(r) for r in runs]), np.cumsum([0] + [len(r) for r in runs]), H, W, dev)
    assert torch.equal(back["mask"], res["mask"]) and torch.equal(back["info"], res["info"])
    empty = rle.paste_masks(torch.zeros((0, 2, S, S), device=dev), [], [], H, W)
    assert tuple(empty["mask"].shape) == (0, H, W) and tuple(empty["info"].shape) == (0, 5)
