"""The fused upsample + F(4x4) Winograd launch (winograd4.hip, UP form) rests on two counts, restated here
with krrn_src_index's f32 arithmetic (krrn_common.h, align_corners, scale (float)(n - 1) / (float)(2 n - 1)):

  * a tile's 6-pixel patch side (destination pixels 4 t - 1 .. 4 t + 4, those inside the map) touches at most
    4 consecutive source pixels, starting at the source index of its first pixel inside the map;
  * the windows of the 32 tiles of a block start at most 62 source pixels apart, so a block's source window
    is at most 66 pixels wide (kUC).

Checked for every source size n = 1 .. 1024 (conv sizes 2 .. 2048). The plan produces n = S / 2 for crop
size S, and only n >= 16 reaches the F(4x4) kernel (ops.wino4_eligible: a map of at least 32 x 32); the
entry point itself accepts any even size, hence the range from 1."""
import numpy as np

f32 = np.float32


def _src_index(dst, n_in, scale):
    """krrn_src_index(dst, n_in, scale, align = 1) on an int array: (i0, i1)."""
    s = (f32(scale) * dst.astype(f32)).astype(f32)
    i = np.minimum(s.astype(np.int64), n_in - 1)
    return i, i + (i < n_in - 1)


def test_patch_side_touches_at_most_4_source_pixels_and_a_block_66():
    worst_taps, worst_span = 0, 0
    for n in range(1, 1025):
        n_out = 2 * n
        scale = f32(n - 1) / f32(n_out - 1)
        assert scale.dtype == f32
        tiles = np.arange((n_out + 3) // 4)
        x0 = 4 * tiles - 1
        base, _ = _src_index(np.maximum(x0, 0), n, scale)
        assert np.all(np.diff(base) >= 0)
        for p in range(6):
            x = x0 + p
            ok = (x >= 0) & (x < n_out)
            i0, i1 = _src_index(np.clip(x, 0, n_out - 1), n, scale)
            assert np.all((i0 - base >= 0)[ok]) and np.all((i1 - base <= 3)[ok]), (n, p)
            worst_taps = max(worst_taps, int((i1 - base)[ok].max(initial=0)) + 1)
        # blocks start at tiles 0, 32, 64, ...: the last tile's window start against the block's
        for t0 in range(0, len(tiles), 32):
            worst_span = max(worst_span, int(base[t0:t0 + 32].max() - base[t0]) + 4)
    assert worst_taps <= 4 and worst_span <= 66, (worst_taps, worst_span)
