"""krrn_mask_paste_f32 restated in numpy (not a test; include/krrn_hip.h gives the definition): the class decision per
crop pixel as the walk `best = 0; for c = 1 .. C1 - 1: if l[c] > l[best]: best = c` with IEEE comparisons (not
np.argmax, which takes a NaN for the maximum), the rule that turns `best` and chan into a set pixel, and the placement
of the S x S window at (rmin, cmin) in an H x W frame with Python integers, so that any rc is handled without a
wrap. `info` is rle_ref.info of the plane."""
import numpy as np

import rle_ref as rf


def decide(logits):
    """best int64 [S, S] of logits f32 [C1, S, S]."""
    l = np.asarray(logits, np.float32)
    best = np.zeros(l.shape[1:], np.int64)
    top = l[0].copy()
    for c in range(1, l.shape[0]):
        with np.errstate(invalid="ignore"):
            win = l[c] > top                             # False where either side is NaN
        best[win] = c
        top[win] = l[c][win]
    return best


def window(logits, chan):
    """The crop's own S x S mask, u8 of 0 / 1."""
    l = np.asarray(logits, np.float32)
    C1, chan = l.shape[0], int(chan)
    best = decide(l)
    if 1 <= chan < C1:
        return (best == chan).astype(np.uint8)
    if chan == 0:
        return (best != 0).astype(np.uint8)
    return np.zeros(l.shape[1:], np.uint8)


def paste(logits, chan, rc, H, W):
    """(mask u8 [B, H, W], info int32 [B, 5]) of logits [B, C1, S, S], chan [B], rc [B][2] = (rmin, cmin)."""
    l = np.asarray(logits, np.float32)
    B, _, S, _ = l.shape
    mask = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        rmin, cmin = int(rc[b][0]), int(rc[b][1])
        r0, r1 = max(rmin, 0), min(rmin + S, H)          # frame rows r0 .. r1 - 1 = window rows r0 - rmin ..
        c0, c1 = max(cmin, 0), min(cmin + S, W)
        if r1 > r0 and c1 > c0:
            mask[b, r0:r1, c0:c1] = window(l[b], chan[b])[r0 - rmin:r1 - rmin, c0 - cmin:c1 - cmin]
    info = np.stack([rf.info(m) for m in mask]) if B else np.zeros((0, 5), np.int32)
    return mask, info
