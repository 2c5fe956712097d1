"""Whole scenes in one z-buffer on the GPU, and the pictures made from them (krrn_scene_render_f64,
krrn_scene_overlay_u8, krrn_scene_depth_diff_u8; include/krrn_hip.h states the definitions, tests/scene_ref.py restates
them in numpy). Every other render here draws one instance per launch slot; this one draws all instances of a frame,
each under its own pose, with one object hiding another.

    res = render(verts, faces, face_range, R, t, K4, inst_range, H, W)
    # N instances over F frames -> {"inst": int32 [F, H, W] (the winner's index in the list, -1 for none),
    #   "depth": f32 [F, H, W] metres (0 for none), "shade": u8 [F, H, W] (a flat Lambert term in 64 .. 255, 0 for none)}
    img = overlay(rgb, res["inst"], res["shade"], palette(obj_ids), gt=gt_res["inst"])   # u8 [F, H, W, 3]
    img = depth_diff(res["depth"], observed)                                             # u8 [F, H, W, 3]

bop_scene.vis_results(dataset, rows, out_dir, device) writes such pictures for a result file, and
evaluate.test_epoch(..., vis_dir=...) for an epoch's own estimates."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .runtime import h2d, ptr, stream_ptr

# twelve colours told apart at a glance, cycled by object id
PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180),
           (70, 240, 240), (240, 50, 230), (210, 245, 60), (250, 190, 190), (0, 128, 128), (170, 110, 40))


def palette(obj_ids: Sequence[int]) -> np.ndarray:
    """The tint of each object id, u8 [n, 3]: PALETTE[obj_id % 12]."""
    ids = np.asarray(list(obj_ids), dtype=np.int64).reshape(-1)
    return np.asarray(PALETTE, np.uint8)[ids % len(PALETTE)].reshape(-1, 3)


def _gpu(x, dtype, shape, name: str) -> torch.Tensor:
    """A large operand as it stands: a contiguous tensor of `dtype` whose shape matches `shape` (None = any size);
    ValueError otherwise. _on_device then asks for the GPU."""
    want = f"a contiguous {str(dtype).replace('torch.', '')} [{', '.join('n' if s is None else str(s) for s in shape)}] tensor"
    if not isinstance(x, torch.Tensor) or x.dtype != dtype or x.dim() != len(shape) or \
            any(s is not None and int(d) != s for d, s in zip(x.shape, shape)) or not x.is_contiguous():
        got = f"{x.dtype} {tuple(x.shape)}" if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"{name} must be {want}, got {got}")
    return x


def _on_device(fn: str, **tensors):
    """The one GPU device of the given tensors (None entries skipped): RuntimeError for a CPU tensor, ValueError for
    two devices."""
    given = {k: v for k, v in tensors.items() if v is not None}
    if not all(v.is_cuda for v in given.values()):
        raise RuntimeError(f"scene.{fn} runs on the HIP path only ({' / '.join(given)} must be GPU tensors)")
    dev = next(iter(given.values())).device
    if any(v.device != dev for v in given.values()):
        raise ValueError(f"scene.{fn}: {' / '.join(given)} must be on one device")
    return dev


def _staged(x, dtype, shape, name: str, device) -> torch.Tensor:
    """A small operand on `device`: a host sequence, array or tensor is converted and staged with h2d; a GPU tensor
    must already have the dtype and sit on `device`. ValueError for another size."""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        if x.dtype != dtype or x.device != device:
            raise ValueError(f"{name}: a GPU tensor must be {dtype} on {device}, got {x.dtype} on {x.device}")
        tn = x
    else:
        tn = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
        if tn.numel() and tn.is_floating_point() != dtype.is_floating_point:
            raise ValueError(f"{name} must hold {'floats' if dtype.is_floating_point else 'integers'}, got {tn.dtype}")
    n = 1
    for s in shape:
        n *= s
    if tn.numel() != n:
        raise ValueError(f"{name} must be {list(shape)}, got {tuple(tn.shape)}")
    if n == 0:
        return torch.empty(shape, dtype=dtype, device=device)
    return h2d(tn.reshape(shape), device, dtype)


def _frame(H, W):
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or H * W > 0x7fffffff:
        raise ValueError(f"frame {H} x {W}: H and W must be positive and H * W fit an int32")
    return H, W


def render(verts: torch.Tensor, faces: torch.Tensor, face_range, R, t, K4, inst_range, H: int,
           W: int) -> Dict[str, torch.Tensor]:
    """krrn_scene_render_f64 for N instances over F frames (module doc). verts f32 [Vtot, 3] and faces int32 [Ftot, 3]
    (global vertex indices) are GPU tensors; face_range [N, 2], R [N, 3, 3] (or [N, 9]), t [N, 3] metres, K4 [N, 4] and
    inst_range [F, 2] = (first instance, count) per frame may be host sequences, arrays or tensors (staged with h2d)
    or GPU tensors of the kernel's types (int32 / f64 / f64 / f32 / int32). Frame f's instances are drawn in index
    order into one depth buffer; equal depths go to the lowest index. Another dtype, shape or device raises ValueError,
    a CPU mesh RuntimeError, before anything is launched. Queued on the current stream; nothing is read back."""
    v = _gpu(verts, torch.float32, (None, 3), "verts")
    f = _gpu(faces, torch.int32, (None, 3), "faces")
    if v.shape[0] < 1:
        raise ValueError("verts holds no vertex")
    H, W = _frame(H, W)
    dev = _on_device("render", verts=v, faces=f)
    N = int(np.prod(np.shape(t))) // 3 if not isinstance(t, torch.Tensor) else t.numel() // 3
    F = (int(np.prod(np.shape(inst_range))) if not isinstance(inst_range, torch.Tensor) else inst_range.numel()) // 2
    if F < 1:
        raise ValueError("inst_range must be [F, 2] with F >= 1")
    fr = _staged(face_range, torch.int32, (N, 2), "face_range", dev)
    Rd = _staged(R, torch.float64, (N, 9), "R", dev)
    td = _staged(t, torch.float64, (N, 3), "t", dev)
    Kd = _staged(K4, torch.float32, (N, 4), "K4", dev)
    ir = _staged(inst_range, torch.int32, (F, 2), "inst_range", dev)
    n_ints = ctypes.c_longlong(0)
    _lib.call("krrn_scene_render_ws", N, ctypes.byref(n_ints))
    ws = torch.empty((max(1, n_ints.value),), dtype=torch.int32, device=dev)
    out = {"inst": torch.empty((F, H, W), dtype=torch.int32, device=dev),
           "depth": torch.empty((F, H, W), dtype=torch.float32, device=dev),
           "shade": torch.empty((F, H, W), dtype=torch.uint8, device=dev)}
    dummy = torch.empty((9,), dtype=torch.float64, device=dev)     # a non-null address for an empty operand
    at = lambda x: ptr(x) if x.numel() else ptr(dummy)  # noqa: E731
    _lib.call("krrn_scene_render_f64", ptr(v), v.shape[0], at(f), f.shape[0], at(fr), at(Rd), at(td), at(Kd), ptr(ir), N,
              F, H, W, ptr(ws), ptr(out["inst"]), ptr(out["depth"]), ptr(out["shade"]), stream_ptr(dev))
    return out


def overlay(rgb: torch.Tensor, est: torch.Tensor, shade: torch.Tensor, tint, alpha: int = 128, radius: int = 1,
            gt: Optional[torch.Tensor] = None, gt_colour: Sequence[int] = (0, 255, 0)) -> torch.Tensor:
    """krrn_scene_overlay_u8: rgb u8 [F, H, W, 3] with the instances of est int32 [F, H, W] blended over it, each in
    its tint [N, 3] (u8; a host sequence is staged) lit by shade u8 [F, H, W], weight alpha / 256, and outlined in its
    plain tint `radius` pixels wide; gt (optional, int32 [F, H, W]) adds the outlines of a second id plane in gt_colour.
    GPU tensors, contiguous. Returns u8 [F, H, W, 3]. alpha outside 0 .. 256, radius outside 1 .. 4, a colour outside
    0 .. 255, another dtype, shape or device raise ValueError, a CPU tensor RuntimeError, before anything is launched.
    Queued on the current stream; nothing is read back."""
    c = _gpu(rgb, torch.uint8, (None, None, None, 3), "rgb")
    F, H, W = (int(x) for x in c.shape[:3])
    e = _gpu(est, torch.int32, (F, H, W), "est")
    s = _gpu(shade, torch.uint8, (F, H, W), "shade")
    g = _gpu(gt, torch.int32, (F, H, W), "gt") if gt is not None else None
    if F < 1:
        raise ValueError("rgb holds no frame")
    H, W = _frame(H, W)
    alpha, radius, col = int(alpha), int(radius), [int(x) for x in gt_colour]
    if not 0 <= alpha <= 256:
        raise ValueError(f"alpha must be 0 .. 256, got {alpha}")
    if not 1 <= radius <= 4:
        raise ValueError(f"radius must be 1 .. 4, got {radius}")
    if len(col) != 3 or not all(0 <= x <= 255 for x in col):
        raise ValueError(f"gt_colour must be three values in 0 .. 255, got {col}")
    dev = _on_device("overlay", rgb=c, est=e, shade=s, gt=g)
    if isinstance(tint, torch.Tensor) and tint.is_cuda:
        N = tint.numel() // 3
    else:
        ta = np.asarray(tint.numpy() if isinstance(tint, torch.Tensor) else tint)
        if ta.size and (ta.dtype.kind not in "iu" or ta.min() < 0 or ta.max() > 255):
            raise ValueError("tint must hold integers in 0 .. 255")
        N, tint = ta.size // 3, ta.astype(np.uint8)
    td = _staged(tint, torch.uint8, (N, 3), "tint", dev)
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    dummy = torch.empty((4,), dtype=torch.uint8, device=dev)       # a non-null address for an empty tint
    _lib.call("krrn_scene_overlay_u8", ptr(c), ptr(e), ptr(s), ptr(td) if N else ptr(dummy), N, alpha, radius, ptr(g),
              col[0], col[1], col[2], F, H, W, ptr(out), stream_ptr(dev))
    return out


def depth_diff(ren: torch.Tensor, obs: torch.Tensor, depth_scale: float = 1.0, tol: float = 0.02) -> torch.Tensor:
    """krrn_scene_depth_diff_u8: ren (a rendered depth plane, such as render's "depth") against obs / depth_scale, f32
    [F, H, W] GPU tensors, as u8 [F, H, W, 3]: white where they agree, towards red where the model lies behind the
    observed surface (hidden, or too far) and towards blue where it lies in front, saturated at `tol` metres; grey where
    the model is rendered and nothing is observed, black where nothing is rendered. tol not finite or not > 0,
    depth_scale == 0, another dtype or shape raise ValueError, a CPU tensor RuntimeError, before anything is launched.
    Queued on the current stream; nothing is read back."""
    r = _gpu(ren, torch.float32, (None, None, None), "ren")
    F, H, W = (int(x) for x in r.shape)
    o = _gpu(obs, torch.float32, (F, H, W), "obs")
    if F < 1:
        raise ValueError("ren holds no frame")
    H, W = _frame(H, W)
    depth_scale, tol = float(depth_scale), float(tol)
    if not (tol > 0.0 and tol != float("inf")):
        raise ValueError(f"tol must be finite and > 0, got {tol}")
    if depth_scale == 0.0:
        raise ValueError("depth_scale must not be 0")
    _on_device("depth_diff", ren=r, obs=o)
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=r.device)
    _lib.call("krrn_scene_depth_diff_u8", ptr(r), ptr(o), depth_scale, tol, F, H, W, ptr(out), stream_ptr(r.device))
    return out
