"""Pose refinement by render-and-compare on the depth frame, batched and on the GPU (krrn_pose_refine_depth_f32;
include/krrn_hip.h states the definition, tests/depth_refine_ref.py restates it in numpy). The reference project has
no such step; the definition is this project's own.

    R, t = refine(verts, faces, face_range, R, t, K4, depth, frame, max_dist, radius)
    # R [B, 3, 3], t [B, 3]: the starting pose, model to camera; verts / faces / face_range: the resident meshes;
    # depth [F, H, W] the observed frames, frame [B] each crop's frame; max_dist, radius metres (a float or [B])

Per crop and pass: the mesh is rendered under the current pose (VSD's depth walk), every rendered pixel is paired
with the observed depth at that same pixel and kept if the two differ by less than max_dist (and the optional mask
is set there); one damped Gauss-Newton step on the point-to-plane error of the kept pixels, in a twist about the
object's own centre with the rotation scaled by `radius`, gives the next pose. Unlike icp.refine only the visible
surface takes part, and the cost per pass is one render. The loop stops when fewer than min_pairs pixels are left
(STARVED), when the mean squared residual changes by at most tol of itself (CONVERGED), after max_iter updates
(MAX_ITER), or on normal equations without a positive-definite, finite solution (DEGENERATE: the pose from before
the update is returned). `info` describes the returned pose: passes (the updates applied), pairs, rmse, status.

The defaults below are this project's choices, from a numpy prototype on the test scenes.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Union

import torch

from . import _lib
from .bop import per_crop, stage_scene
from .icp import STATUS  # noqa: F401  (the same four codes, in the same order)
from .runtime import h2d, ptr, stream_ptr

MAX_ITER = 10        # updates at most (max_iter + 1 renders); the kernel allows 0 .. 32. The generic scenes converge
                     # in 4 .. 10 passes from 2-3 degrees / 3-5 mm
TOL = 1e-4           # relative change of the mean squared residual that counts as converged (icp.TOL)
MIN_PAIRS = 6        # fewer kept pixels: STARVED (six unknowns; the kernel refuses less)
DIST_FRAC = 0.2      # max_dist as a share of the object's diameter: at 0.1 a start 3 degrees off still lost
                     # pixels on its first step, at 0.2 the pixel count never dropped
DAMP = 1e-4          # A += DAMP trace(A) / 6 I: keeps an unobservable direction (a plane's in-plane slide, a
                     # sphere's rotation) from blowing the step up without slowing the observable ones
RADIUS_FRAC = 0.5    # rho = diameter / 2: a unit of the scaled rotation moves the surface about as far as a unit of
                     # translation, so one damping value serves both


def refine(verts: torch.Tensor, faces: torch.Tensor, face_range: torch.Tensor, R: torch.Tensor, t: torch.Tensor,
           K4: torch.Tensor, depth: torch.Tensor, frame: torch.Tensor, max_dist: Union[float, torch.Tensor],
           radius: Union[float, torch.Tensor], mask: Optional[torch.Tensor] = None, depth_scale: float = 1.0,
           max_iter: int = MAX_ITER, tol: float = TOL, min_pairs: int = MIN_PAIRS, damp: float = DAMP,
           return_info: bool = False):
    """krrn_pose_refine_depth_f32 for B crops (module doc) -> (R f32 [B, 3, 3], t f32 [B, 3]), with return_info also
    {"passes", "pairs" int32 [B], "rmse" f32 [B], "status" int32 [B] (icp.STATUS)}. verts [Vtot, 3] / faces [Ftot, 3]
    / depth [F, H, W] / mask u8 [F, H, W] are GPU tensors; face_range [B, 2], R [B, 3, 3], t [B, 3], K4 [B, 4], frame
    [B] and tensor max_dist / radius [B] may be host tensors (staged here). Nothing is read back and the host makes
    no decision between the launches: the start poses may come straight from a solver's launch. The inputs are not
    modified."""
    # every converted operand stays bound until the launches are enqueued (metric.add_metric's rule)
    s = stage_scene("depth_refine.refine", verts, faces, face_range, K4, depth, frame, mask)
    dev, B = verts.device, s.B
    if R.numel() != 9 * B or t.numel() != 3 * B:
        raise ValueError(f"R must be [B, 3, 3] and t [B, 3] with B = {B}, got {tuple(R.shape)}, {tuple(t.shape)}")
    R0 = h2d(R.reshape(B, 9), dev, torch.float32)
    t0 = h2d(t.reshape(B, 3), dev, torch.float32)
    md = per_crop(max_dist, B, dev, "max_dist")
    rho = per_crop(radius, B, dev, "radius")
    n_bytes = ctypes.c_longlong(0)
    _lib.call("krrn_pose_refine_depth_ws", B, s.H, s.W, ctypes.byref(n_bytes))
    ws = torch.empty(((n_bytes.value + 7) // 8,), dtype=torch.float64, device=dev)
    Rn = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    tn = torch.empty((B, 3), dtype=torch.float32, device=dev)
    info = {"passes": torch.empty((B,), dtype=torch.int32, device=dev),
            "pairs": torch.empty((B,), dtype=torch.int32, device=dev),
            "rmse": torch.empty((B,), dtype=torch.float32, device=dev),
            "status": torch.empty((B,), dtype=torch.int32, device=dev)}
    _lib.call("krrn_pose_refine_depth_f32", ptr(s.v), s.v.shape[0], ptr(s.f), s.f.shape[0], ptr(s.fr), ptr(R0), ptr(t0),
              ptr(s.K), ptr(s.d), ptr(s.m), s.F, s.H, s.W, ptr(s.fi), float(depth_scale), ptr(md), ptr(rho),
              int(max_iter), float(tol), int(min_pairs), float(damp), B, ptr(ws), ptr(Rn), ptr(tn), ptr(info["passes"]),
              ptr(info["pairs"]), ptr(info["rmse"]), ptr(info["status"]), stream_ptr(dev))
    if return_info:
        return Rn, tn, info
    return Rn, tn
