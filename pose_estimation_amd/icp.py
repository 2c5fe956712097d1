"""Pose refinement by point-to-point ICP against the depth cloud, batched and on the GPU
(krrn_icp_refine_f32). The reference project has no ICP; the definition is this project's own
(include/krrn_hip.h; tests/icp_ref.py restates it in numpy).

    R, t = refine(R, t, cloud, model_points, max_dist)
    # R [B, 3, 3], t [B, 3]: the starting pose, model to camera (p = R m + t); cloud [B, N, 3] camera
    # frame, model_points [B, M, 3] object frame ([3, 3] / [N, 3] / [M, 3] = one crop); max_dist in metres

Per crop and pass: every cloud point goes to the object frame, pairs with its nearest model point (f64,
brute force, the lowest index among equal distances) and is kept if closer than max_dist; Kabsch on
the kept pairs gives the next pose. The loop stops when fewer than min_pairs pairs are left (STARVED),
when the mean squared pair distance changes by at most tol of itself (CONVERGED), after max_iter
updates (MAX_ITER), or on a pair set without a finite rotation (DEGENERATE: the pose from before the
update is returned). `info` describes the returned pose: passes, pairs, rmse, status, nn_idx.

The defaults are this project's design choices (nothing in the reference fixes them): max_iter 20,
tol 1e-4, min_pairs 6, and in the eval loop max_dist = DIST_FRAC (0.1) x the object's diameter.
"""
from __future__ import annotations

from typing import Union

import torch

from .runtime import Immediate, ptr

MAX_ITER = 20        # updates at most (max_iter + 1 passes); the kernel allows 0 .. 64
TOL = 1e-4           # relative change of the mean squared pair distance that counts as converged
MIN_PAIRS = 6        # fewer kept pairs: STARVED (the kernel needs >= 3)
DIST_FRAC = 0.1      # max_dist as a fraction of the object's diameter (pose.refine_pose_icp, the eval loop)
MAX_POINTS = 4096    # kIcpMaxN / kIcpMaxM of csrc/icp.hip
STATUS = ("CONVERGED", "MAX_ITER", "STARVED", "DEGENERATE")  # info["status"] codes 0 .. 3


def dist_tensor(max_dist: Union[float, torch.Tensor], B: int, device) -> torch.Tensor:
    """max_dist as the f32 [B] device tensor the kernel reads."""
    if isinstance(max_dist, torch.Tensor):
        md = max_dist.to(device=device, dtype=torch.float32).reshape(-1).contiguous()
        if md.numel() != B:
            raise ValueError(f"max_dist must be a float or a [B] tensor with B = {B}, got {tuple(max_dist.shape)}")
        return md
    return torch.full((B,), float(max_dist), dtype=torch.float32, device=device)


def refine_step(ctx, R0: torch.Tensor, t0: torch.Tensor, cloud: torch.Tensor, model: torch.Tensor,
                max_dist: torch.Tensor, B: int, N: int, M: int, max_iter: int = MAX_ITER, tol: float = TOL,
                min_pairs: int = MIN_PAIRS, with_nn: bool = True):
    """The krrn_icp_refine_f32 launch, stated once, on `ctx` (a runtime.Plan or runtime.Immediate). R0 [B, 3, 3],
    t0 [B, 3], cloud [B, N, 3], model [B, M, 3], max_dist [B]: f32 contiguous device tensors. Returns (R, t, info)
    buffers; without `with_nn` the kernel gets a null nn_idx and info["nn_idx"] is None."""
    R = ctx.buf((B, 3, 3))
    t = ctx.buf((B, 3))
    passes = ctx.buf((B,), torch.int32)
    pairs = ctx.buf((B,), torch.int32)
    rmse = ctx.buf((B,))
    status = ctx.buf((B,), torch.int32)
    nn_idx = ctx.buf((B, N), torch.int32) if with_nn else None
    ctx.add("krrn_icp_refine_f32", ptr(R0), ptr(t0), ptr(cloud), N, ptr(model), M, ptr(max_dist), int(max_iter),
            float(tol), int(min_pairs), ptr(R), ptr(t), ptr(passes), ptr(pairs), ptr(rmse), ptr(status), ptr(nn_idx), B)
    return R, t, {"passes": passes, "pairs": pairs, "rmse": rmse, "status": status, "nn_idx": nn_idx}


def solve(R0: torch.Tensor, t0: torch.Tensor, cloud: torch.Tensor, model: torch.Tensor, max_dist: torch.Tensor,
          max_iter: int = MAX_ITER, tol: float = TOL, min_pairs: int = MIN_PAIRS, with_nn: bool = True):
    """f32 contiguous GPU tensors R0 [B, 3, 3], t0 [B, 3], cloud [B, N, 3], model [B, M, 3], max_dist [B]
    -> (R, t, info) device buffers; info["nn_idx"] is None without `with_nn`."""
    B, N, _ = cloud.shape
    return refine_step(Immediate(cloud.device), R0, t0, cloud, model, max_dist, B, N, model.shape[1], max_iter, tol,
                       min_pairs, with_nn)


def refine(R: torch.Tensor, t: torch.Tensor, cloud: torch.Tensor, model_points: torch.Tensor,
           max_dist: Union[float, torch.Tensor], max_iter: int = MAX_ITER, tol: float = TOL,
           min_pairs: int = MIN_PAIRS, return_info: bool = False):
    """(R [B, 3, 3], t [B, 3]) refined against `cloud`; with return_info also the dict of passes / pairs /
    rmse / status [B] and nn_idx [B, N] (the model point paired with every cloud point under the returned
    pose, -1 = rejected). max_dist: a float or a [B] tensor. The inputs are not modified."""
    ts = (R, t, cloud, model_points)
    if not all(isinstance(x, torch.Tensor) and x.is_cuda for x in ts):
        raise RuntimeError("icp.refine runs on the HIP path only (R / t / cloud / model_points must be GPU tensors)")
    if cloud.dim() == 2:
        R, t, cloud, model_points = R[None], t.reshape(1, -1), cloud[None], model_points[None]
    if cloud.dim() != 3 or cloud.shape[-1] != 3 or model_points.dim() != 3 or model_points.shape[-1] != 3:
        raise ValueError("cloud must be [B, N, 3] and model_points [B, M, 3] (or [N, 3] / [M, 3]).")
    B = cloud.shape[0]
    if model_points.shape[0] != B or tuple(R.shape) != (B, 3, 3) or t.numel() != 3 * B:
        raise ValueError(f"R must be [B, 3, 3], t [B, 3] and model_points [B, M, 3] with the cloud's B = {B}; got "
                         f"{tuple(R.shape)}, {tuple(t.shape)}, {tuple(model_points.shape)}")
    dev = cloud.device
    f = lambda x: x.to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    R0, t0, c, m = f(R), f(t).reshape(B, 3), f(cloud), f(model_points)
    md = dist_tensor(max_dist, B, dev)
    Rn, tn, info = solve(R0, t0, c, m, md, max_iter, tol, min_pairs, with_nn=return_info)
    if return_info:
        return Rn, tn, info
    return Rn, tn
