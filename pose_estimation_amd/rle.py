"""COCO run-length encoded masks, the `segmentation` of BOP's detection files: the string codec, an encoder and a
box's runs on the host, and the decoder on the GPU (krrn_rle_decode_u8; include/krrn_hip.h states the definition).

    runs = counts_from_string("61X13mN000`0")           # [6, 1, 40, 4, 5, 4, 5, 4, 21]; counts_to_string inverts it
    runs = encode(mask)                                 # host u8 / bool [H, W] -> run list
    runs = box_counts(x, y, w, h, H, W)                 # a filled box, for a detection without `segmentation`
    out = decode(counts, offs, H, W, device)            # {"mask": u8 [n, H, W] of 0 / 1, "info": int32 [n, 5]}

Run semantics are COCO's: pixels are numbered column-major (p = x * H + y), the first run is zeros, the runs
alternate, and a run may have length 0 (the first one when pixel (0, 0) is set). `info` = (pixel count, x, y, w, h):
the tight box of the set pixels in BOP's convention w = x_max - x_min, h = y_max - y_min; five zeros for an empty
mask. The compressed string form is the published one (pycocotools' rleToString / rleFrString): 5 payload bits per
character above '0', bit 0x20 = another character follows, the last character's bit 0x10 is the sign, and from the
fourth value on the value two places back is added."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .runtime import h2d, ptr, stream_ptr


def counts_from_string(s: str) -> List[int]:
    out: List[int] = []
    i, n = 0, len(s)
    while i < n:
        x, k, more = 0, 0, True
        while more:
            if i >= n:
                raise ValueError("RLE string ends inside a value")
            c = ord(s[i]) - 48
            if not 0 <= c < 64:
                raise ValueError(f"RLE string holds the character {s[i]!r}, outside '0' .. 'o'")
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            i, k = i + 1, k + 1
            if not more and (c & 0x10):
                x -= 1 << (5 * k)                        # sign-extend
        if len(out) > 2:
            x += out[-2]
        out.append(x)
    return out


def counts_to_string(counts: Sequence[int]) -> str:
    counts = [int(c) for c in counts]
    chars = []
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5                                      # arithmetic: a negative value ends at -1
            more = (x != -1) if (c & 0x10) else (x != 0)
            chars.append(chr((c | 0x20 if more else c) + 48))
    return "".join(chars)


def encode(mask) -> List[int]:
    """The runs of a host mask [H, W] (any non-zero element is set): column-major transitions, with a leading 0
    when pixel (0, 0) is set."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError(f"mask must be [H, W], got {m.shape}")
    flat = (m != 0).T.reshape(-1)
    if flat.size == 0:
        return [0]
    edges = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    runs = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
    return [0] + runs if flat[0] else runs


def box_counts(x, y, w, h, H: int, W: int) -> List[int]:
    """The runs of the filled box of pixels x <= col < x + w, y <= row < y + h, clipped to the H x W frame (bounds
    rounded to the nearest pixel); [H * W] when nothing is left."""
    x0, x1 = max(0, int(round(float(x)))), min(int(W), int(round(float(x) + float(w))))
    y0, y1 = max(0, int(round(float(y)))), min(int(H), int(round(float(y) + float(h))))
    if x1 <= x0 or y1 <= y0:
        return [int(H) * int(W)]
    m = np.zeros((int(H), int(W)), np.uint8)
    m[y0:y1, x0:x1] = 1
    return encode(m)


def _validate(counts: np.ndarray, offs: np.ndarray, H: int, W: int) -> None:
    if H <= 0 or W <= 0 or H * W > 0x7fffffff:
        raise ValueError(f"frame {H} x {W}: H and W must be positive and H * W fit an int32")
    if len(offs) < 1:
        raise ValueError("offs must be [n + 1]")
    for i in range(len(offs) - 1):
        a, b = int(offs[i]), int(offs[i + 1])
        if a < 0 or b > len(counts):
            raise ValueError(f"mask {i}: its runs {a} .. {b} lie outside the {len(counts)} counts")
        if b < a:
            raise ValueError(f"mask {i}: offs is not increasing ({a} then {b})")
        if b == a:
            raise ValueError(f"mask {i} has no run")
        c = counts[a:b]
        if (c < 0).any():
            raise ValueError(f"mask {i} has a negative count")
        if int(c.sum()) != H * W:
            raise ValueError(f"mask {i}: its runs sum to {int(c.sum())}, not H * W = {H * W}")


def decode(counts, offs, H: int, W: int, device, out: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """krrn_rle_decode_u8 for n masks. `counts` = the masks' run lists concatenated and `offs` [n + 1] their
    bounds in it (mask i owns counts[offs[i]:offs[i + 1]]), host integer arrays. Refused before anything is
    launched, with a ValueError naming the mask: a negative count, runs that do not sum to H * W, a mask with no
    run, non-increasing offs. `out`: an optional u8 [n, H, W] GPU tensor to decode into (contiguous, at any byte
    address). Queued on the current stream; nothing is read back."""
    c64 = np.asarray(counts, dtype=np.int64).reshape(-1)
    o64 = np.asarray(offs, dtype=np.int64).reshape(-1)
    H, W = int(H), int(W)
    _validate(c64, o64, H, W)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("rle.decode runs on the HIP path only (a GPU device)")
    n = len(o64) - 1
    if out is None:
        out = torch.empty((n, H, W), dtype=torch.uint8, device=device)
    elif (out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W) or not out.is_cuda or not out.is_contiguous()
          or out.device != device):
        raise ValueError(f"out must be a contiguous u8 [{n}, {H}, {W}] tensor on {device}")
    info = torch.empty((n, 5), dtype=torch.int32, device=device)
    if n == 0:
        return {"mask": out, "info": info}
    cd = h2d(torch.from_numpy(c64.astype(np.int32)), device)
    od = h2d(torch.from_numpy(o64.astype(np.int32)), device)
    ends = torch.empty((len(c64),), dtype=torch.int32, device=device)
    _lib.call("krrn_rle_decode_u8", ptr(cd), ptr(od), n, H, W, ptr(ends), ptr(out), ptr(info), stream_ptr(device))
    return {"mask": out, "info": info}
