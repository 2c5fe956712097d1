"""COCO run-length encoded masks, the `segmentation` of BOP's detection files: the string codec, an encoder and a
box's runs on the host, and the decoder, the encoder and the paste of the mask head's crop windows into full-frame
planes on the GPU (krrn_rle_decode_u8 / krrn_rle_encode_u8 / krrn_mask_paste_f32; include/krrn_hip.h states the
definitions), and the IoU of pairs of run lists or boxes on the GPU (krrn_rle_iou_f64 / krrn_box_iou_f64).

    runs = counts_from_string("61X13mN000`0")           # [6, 1, 40, 4, 5, 4, 5, 4, 21]; counts_to_string inverts it
    runs = encode(mask)                                 # host u8 / bool [H, W] -> run list
    runs = box_counts(x, y, w, h, H, W)                 # a filled box, for a detection without `segmentation`
    out = decode(counts, offs, H, W, device)            # {"mask": u8 [n, H, W] of 0 / 1, "info": int32 [n, 5]}
    enc = encode_gpu(planes)                            # GPU u8 / bool [n, H, W] -> {"counts", "n_runs", "info"}
    runs = encode_planes(planes)                        # the same as n run lists: [encode(m) for m in planes.cpu()]
    res = paste_masks(pred["mask"], chan, rc, H, W)     # crop-window logits -> {"mask": u8 [B, H, W], "info"}
    res = iou(counts, offs, pair, crowd, device)        # run-list pairs -> {"inter", "iou" f64 [P], "area" [n]}
    res = box_iou(box, pair, crowd, device)             # [x, y, w, h] pairs -> {"iou" f64 [P], "area" f64 [n]}

Run semantics are COCO's: pixels are numbered column-major (p = x * H + y), the first run is zeros, the runs
alternate, and a run may have length 0 (the first one when pixel (0, 0) is set). `info` = (pixel count, x, y, w, h):
the tight box of the set pixels in BOP's convention w = x_max - x_min, h = y_max - y_min; five zeros for an empty
mask. The compressed string form is the published one (pycocotools' rleToString / rleFrString): 5 payload bits per
character above '0', bit 0x20 = another character follows, the last character's bit 0x10 is the sign, and from the
fourth value on the value two places back is added."""
from __future__ import annotations

import ctypes
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


def _pairs(pair, crowd):
    """pair as int64 [P, 2] and crowd as u8 [P] or None (host arrays); ValueError for another shape."""
    pr = np.asarray(pair, dtype=np.int64).reshape(-1, 2)
    if pr.size and (pr.min() < -0x80000000 or pr.max() > 0x7fffffff):
        raise ValueError("pair must fit an int32")
    cr = None
    if crowd is not None:
        cr = (np.asarray(crowd).reshape(-1) != 0).astype(np.uint8)
        if len(cr) != len(pr):
            raise ValueError(f"crowd must hold one flag per pair: {len(cr)} flags for {len(pr)} pairs")
    return pr, cr


def iou(counts, offs, pair, crowd=None, device=None) -> Dict[str, torch.Tensor]:
    """krrn_rle_iou_f64 for P pairs of n masks: the intersection, the areas and the IoU from the run lists alone (no
    plane is decoded, and no H or W is needed). `counts` / `offs` as decode takes them, `pair` [P, 2] = (detection
    mask, ground-truth mask), `crowd` [P] (optional): where set, the pair's IoU is inter / area(detection), COCO's
    crowd form. Host integer arrays. Refused before anything is launched, with a ValueError naming the mask or the
    pair: a mask with no run, a negative count, runs whose sum does not fit an int32, non-increasing offs, and a
    pair whose two masks do not have the same total (masks of different frames). A pair that names a mask outside
    [0, n) is passed on and gives 0, as the header states. Returns {"inter": int32 [P], "iou": f64 [P], "area": int32
    [n]} on the device. Queued on the current stream; nothing is read back. The definition is written from COCO's
    published one and not checked against pycocotools' own output (it is not a dependency)."""
    c64 = np.asarray(counts, dtype=np.int64).reshape(-1)
    o64 = np.asarray(offs, dtype=np.int64).reshape(-1)
    if len(o64) < 1:
        raise ValueError("offs must be [n + 1]")
    n = len(o64) - 1
    total = np.zeros(n, np.int64)
    for i in range(n):
        a, b = int(o64[i]), int(o64[i + 1])
        if a < 0 or b > len(c64):
            raise ValueError(f"mask {i}: its runs {a} .. {b} lie outside the {len(c64)} counts")
        if b < a:
            raise ValueError(f"mask {i}: offs is not increasing ({a} then {b})")
        if b == a:
            raise ValueError(f"mask {i} has no run")
        c = c64[a:b]
        if (c < 0).any():
            raise ValueError(f"mask {i} has a negative count")
        total[i] = int(c.sum())
        if total[i] > 0x7fffffff:
            raise ValueError(f"mask {i}: its runs sum to {int(total[i])}, which does not fit an int32")
    pr, cr = _pairs(pair, crowd)
    inside = ((pr >= 0) & (pr < n)).all(1)
    odd = np.flatnonzero(inside & (total[np.where(inside, pr[:, 0], 0)] != total[np.where(inside, pr[:, 1], 0)])) if n else []
    if len(odd):
        p, (a, b) = int(odd[0]), pr[odd[0]].tolist()
        raise ValueError(f"pair {p}: mask {a} has {int(total[a])} pixels and mask {b} {int(total[b])}")
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("rle.iou runs on the HIP path only (a GPU device)")
    device = torch.device(device)
    P = len(pr)
    out = {"inter": torch.empty((P,), dtype=torch.int32, device=device),
           "iou": torch.empty((P,), dtype=torch.float64, device=device),
           "area": torch.empty((n,), dtype=torch.int32, device=device)}
    if P == 0 and n == 0:
        return out
    dummy = torch.empty((1,), dtype=torch.float64, device=device)  # a non-null address for an empty operand
    at = lambda t: ptr(t) if t.numel() else ptr(dummy)  # noqa: E731
    cd = h2d(torch.from_numpy(c64.astype(np.int32)), device) if len(c64) else dummy
    od = h2d(torch.from_numpy(o64.astype(np.int32)), device)
    pd = h2d(torch.from_numpy(pr.astype(np.int32)), device) if P else dummy
    kd = h2d(torch.from_numpy(cr), device) if cr is not None and P else None
    n_ints = ctypes.c_longlong(0)
    _lib.call("krrn_rle_iou_ws", len(c64), ctypes.byref(n_ints))
    ws = torch.empty((max(1, n_ints.value),), dtype=torch.int32, device=device)
    _lib.call("krrn_rle_iou_f64", ptr(cd), len(c64), ptr(od), n, ptr(pd), ptr(kd), P, ptr(ws), at(out["inter"]),
              at(out["iou"]), at(out["area"]), stream_ptr(device))
    return out


def box_iou(box, pair, crowd=None, device=None) -> Dict[str, torch.Tensor]:
    """krrn_box_iou_f64 for P pairs of n boxes: `box` [n, 4] = [x, y, w, h] (host numbers), `pair` / `crowd` as iou
    takes them. bop_scene._box_iou's arithmetic in f64, bit for bit; the crowd form divides by the detection's area.
    Returns {"iou": f64 [P], "area": f64 [n] = max(w, 0) max(h, 0)} on the device. Queued on the current stream;
    nothing is read back. ValueError for a box array that is not [n, 4]."""
    b64 = np.asarray(box, dtype=np.float64)
    if b64.size == 0:
        b64 = b64.reshape(0, 4)
    if b64.ndim != 2 or b64.shape[1] != 4:
        raise ValueError(f"box must be [n, 4] = [x, y, w, h], got {b64.shape}")
    n = len(b64)
    pr, cr = _pairs(pair, crowd)
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("rle.box_iou runs on the HIP path only (a GPU device)")
    device = torch.device(device)
    P = len(pr)
    out = {"iou": torch.empty((P,), dtype=torch.float64, device=device),
           "area": torch.empty((n,), dtype=torch.float64, device=device)}
    if P == 0 and n == 0:
        return out
    dummy = torch.empty((1,), dtype=torch.float64, device=device)  # a non-null address for an empty operand
    at = lambda t: ptr(t) if t.numel() else ptr(dummy)  # noqa: E731
    bd = h2d(torch.from_numpy(np.ascontiguousarray(b64)), device) if n else dummy
    pd = h2d(torch.from_numpy(pr.astype(np.int32)), device) if P else dummy
    kd = h2d(torch.from_numpy(cr), device) if cr is not None and P else None
    _lib.call("krrn_box_iou_f64", ptr(bd), n, ptr(pd), ptr(kd), P, at(out["iou"]), at(out["area"]), stream_ptr(device))
    return out


def encode_gpu(mask: torch.Tensor, max_runs: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """krrn_rle_encode_u8 for the n planes of `mask`, a u8 or bool GPU tensor [n, H, W] or [H, W] (any non-zero
    element is set; contiguous, at any byte address). Returns {"counts": int32 [n, max_runs], "n_runs": int32 [n],
    "info": int32 [n, 5]}: mask i's runs are counts[i, :n_runs[i]] (what `encode` returns for the plane) and the rest
    of its slot is 0; n_runs is the true count even where it exceeds max_runs, and the slot then holds the first
    max_runs runs. max_runs defaults to min(H W + 1, 8 W + 1): room for any mask whose columns change value 8 times
    on average. A mask of another dtype or rank, a non-contiguous one or max_runs < 1 raises ValueError, a CPU tensor
    RuntimeError, before anything is launched. Queued on the current stream; nothing is read back."""
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool) or mask.dim() not in (2, 3):
        what = f"{mask.dtype} {tuple(mask.shape)}" if isinstance(mask, torch.Tensor) else type(mask).__name__
        raise ValueError(f"mask must be a u8 or bool [n, H, W] or [H, W] tensor, got {what}")
    if not mask.is_contiguous():
        raise ValueError("mask must be contiguous")
    m = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    m = m[None] if m.dim() == 2 else m
    n, H, W = (int(v) for v in m.shape)
    if H <= 0 or W <= 0 or H * W > 0x7fffffff:
        raise ValueError(f"frame {H} x {W}: H and W must be positive and H * W fit an int32")
    max_runs = min(H * W + 1, 8 * W + 1) if max_runs is None else int(max_runs)
    if max_runs < 1:
        raise ValueError(f"max_runs must be >= 1, got {max_runs}")
    if not mask.is_cuda:
        raise RuntimeError("rle.encode_gpu runs on the HIP path only (a GPU tensor)")
    dev = m.device
    counts = torch.empty((n, max_runs), dtype=torch.int32, device=dev)
    n_runs = torch.empty((n,), dtype=torch.int32, device=dev)
    info = torch.empty((n, 5), dtype=torch.int32, device=dev)
    if n == 0:
        return {"counts": counts, "n_runs": n_runs, "info": info}
    n_ints = ctypes.c_longlong(0)
    _lib.call("krrn_rle_encode_ws", n, W, ctypes.byref(n_ints))
    ws = torch.empty((n_ints.value,), dtype=torch.int32, device=dev)
    _lib.call("krrn_rle_encode_u8", ptr(m), n, H, W, max_runs, ptr(ws), ptr(counts), ptr(n_runs), ptr(info),
              stream_ptr(dev))
    return {"counts": counts, "n_runs": n_runs, "info": info}


def encode_planes(mask: torch.Tensor, max_runs: Optional[int] = None) -> List[List[int]]:
    """The run lists of the n planes of a GPU mask (as encode_gpu takes it), python ints: equal to [encode(m) for m
    in mask.cpu()], but only the runs cross the bus. One read-back of n_runs and counts; if a mask has more than
    max_runs runs, one more call with max_runs = n_runs.max()."""
    return runs_of(mask, encode_gpu(mask, max_runs))


def runs_of(mask: torch.Tensor, res: Dict[str, torch.Tensor]) -> List[List[int]]:
    """encode_planes' read-back for a `res` = encode_gpu(mask, ...) queued earlier: the planes' run lists, with one more
    encode_gpu call if a mask has more runs than res's slot holds (so `mask` must still hold the planes)."""
    nr = res["n_runs"].cpu().numpy()
    cap = int(res["counts"].shape[1])
    if len(nr) and int(nr.max()) > cap:
        res = encode_gpu(mask, int(nr.max()))
    top = int(nr.max()) if len(nr) else 0
    counts = res["counts"][:, :top].cpu().numpy()        # the slots' zero tails past the longest list stay behind
    return [counts[i, :int(k)].tolist() for i, k in enumerate(nr)]


def _int32_operand(v, shape, name: str, device) -> torch.Tensor:
    """`v` as an int32 device tensor of `shape`: a host integer sequence is staged with h2d, a tensor must already
    be int32, contiguous and on `device`."""
    if isinstance(v, torch.Tensor):
        if v.dtype != torch.int32 or tuple(v.shape) != shape or v.device != device or not v.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int32 {list(shape)} tensor on {device} (or a host sequence)")
        return v
    a = np.asarray(v, dtype=np.int64).reshape(shape)     # raises ValueError for another size
    if a.size and (a.min() < -0x80000000 or a.max() > 0x7fffffff):
        raise ValueError(f"{name} must fit an int32")
    if a.size == 0:
        return torch.empty(shape, dtype=torch.int32, device=device)
    return h2d(torch.from_numpy(a.astype(np.int32)), device)


def paste_masks(logits: torch.Tensor, chan, rc, H: int, W: int, out: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """krrn_mask_paste_f32: the mask head's logits of B crops, a GPU f32 [B, C1, S, S] tensor, to full-frame planes
    that encode_gpu takes. Crop b is the S x S window of its H x W frame with top left pixel rc[b] = (rmin, cmin);
    chan[b] is the channel that sets a pixel where it wins the walk `best = 0; for c: if l[c] > l[best]: best = c`
    (cls_id + 1 under the label convention multi_cls_mask = mask (cls + 1); 0 = any foreground channel; any other
    value sets nothing). `logits` may be a view such as pred["mask"], a channel slice of a wider tensor: strides (>=
    C1 S S, S S, S, 1) are passed through, no copy is made (the view is read when the call runs on the stream:
    enqueue it before the next forward rewrites the plan's buffer). Another stride pattern, dtype or rank raises
    ValueError, a CPU tensor RuntimeError, before anything is launched. chan [B] and rc [B, 2]: host integer sequences
    (staged with h2d) or int32 device tensors. `out`: an optional contiguous u8 [B, H, W] GPU tensor at any byte
    address (another dtype, shape or layout raises ValueError). Returns {"mask": u8 [B, H, W] of 0 / 1, "info": int32
    [B, 5]} (info as decode's). Queued on the current stream; nothing is read back."""
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() != 4 or \
            logits.shape[2] != logits.shape[3]:
        what = f"{logits.dtype} {tuple(logits.shape)}" if isinstance(logits, torch.Tensor) else type(logits).__name__
        raise ValueError(f"logits must be an f32 [B, C1, S, S] tensor, got {what}")
    B, C1, S = (int(v) for v in logits.shape[:3])
    H, W = int(H), int(W)
    if C1 < 1 or S < 1 or C1 * S * S > 0x7fffffff:
        raise ValueError(f"logits [B, {C1}, {S}, {S}]: C1 and S must be positive and C1 * S * S fit an int32")
    if H <= 0 or W <= 0 or H * W > 0x7fffffff:
        raise ValueError(f"frame {H} x {W}: H and W must be positive and H * W fit an int32")
    sb, sc, si, sj = (int(v) for v in logits.stride())   # the stride of an axis of one element is never used
    if not ((S == 1 or (si, sj) == (S, 1)) and (C1 == 1 or sc == S * S) and (B <= 1 or sb >= C1 * S * S)):
        raise ValueError(f"logits must have strides (>= C1 S S, S S, S, 1), got {tuple(logits.stride())}")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8
                            or tuple(out.shape) != (B, H, W) or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous u8 [{B}, {H}, {W}] tensor")
    if not logits.is_cuda:
        raise RuntimeError("rle.paste_masks runs on the HIP path only (a GPU tensor)")
    dev = logits.device
    if out is None:
        out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    elif out.device != dev:
        raise ValueError(f"out must be on the logits' device {dev}, got {out.device}")
    cd, rd = _int32_operand(chan, (B,), "chan", dev), _int32_operand(rc, (B, 2), "rc", dev)
    info = torch.empty((B, 5), dtype=torch.int32, device=dev)
    if B == 0:
        return {"mask": out, "info": info}
    _lib.call("krrn_mask_paste_f32", ptr(logits), sb if B > 1 else C1 * S * S, C1, S, ptr(cd), ptr(rd), B, H, W,
              ptr(out), ptr(info), stream_ptr(dev))
    return {"mask": out, "info": info}
