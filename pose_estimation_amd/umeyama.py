"""Similarity transform from 3D-3D correspondences by Umeyama-RANSAC:
lib/transform/umeyama.py's estimateSimilarityTransform (:8-98), batched and on the GPU
(krrn_umeyama_ransac_f32).

    Scale, Rotation, Translation, OutTransform = estimateSimilarityTransform(source, target)
    # source / target [B, N, 3] (or [N, 3] = one crop): target ~ Scale * Rotation @ source + Translation
    # Scale [B], Rotation [B, 3, 3], Translation [B, 3], OutTransform [B, 4, 4] = [[s R, t], [0, 1]]

Reference semantics kept: inlier threshold Scale_h * 0.1 * 2 * max |source - mean(source)|,
128 hypotheses of 5 correspondences each, the loop's early stop at confidence 0.99, failure
below an inlier ratio of 0.1, refit on the best hypothesis's inliers; f64 arithmetic. The
hypotheses are scored in parallel and selected by the reference's own loop over them in order.
Where the reference returns None the batched form reports `inliers == 0` with Scale = 1,
Rotation = I, Translation = 0.

Samples: the reference draws np.random.randint(N, size=5) (with replacement) per iteration; pass the
same `subsets` [B, H, 5] for exact parity. Without them they are drawn on the device
(krrn_ransac_subsets: 5 distinct indices per hypothesis).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .runtime import Immediate, RngStream, device_seed, h2d, ptr

N_HYP = 128          # maxIter (:21)
INLIER_FRAC = 0.1    # InlierT = SourceDiameter / 10 (:20)
CONFIDENCE = 0.99    # (:22)
MIN_RATIO = 0.1      # (:50)
MAX_POINTS = 4096    # kUmeMaxN of csrc/umeyama.hip

_seeds: Dict[int, torch.Tensor] = {}  # this module's own counters (pose.py keeps another table)


def ransac_step(ctx, src: torch.Tensor, dst: torch.Tensor, B: int, N: int, n_hyp: int = N_HYP,
                subsets=None, seed=None, stream_id=None):
    """The krrn_umeyama_ransac_f32 launch, stated once, on `ctx` (a runtime.Plan or runtime.Immediate). src / dst
    f32 [B, N, 3] and `subsets` int32 [B, n_hyp, 5] are contiguous device tensors; without `subsets` they are drawn
    through `ctx` from `seed` on counter stream `stream_id` (the caller advances the seed). Returns buffers."""
    if subsets is None:
        subsets = ctx.buf((B, n_hyp, 5), torch.int32)
        ctx.add("krrn_ransac_subsets", ptr(seed), int(stream_id), B, n_hyp, N, ptr(subsets))
    scale = ctx.buf((B,))
    R = ctx.buf((B, 3, 3))
    t = ctx.buf((B, 3))
    inl = ctx.buf((B,), torch.int32)
    best = ctx.buf((B,), torch.int32)
    counts = ctx.buf((B, n_hyp), torch.int32)
    mask = ctx.buf((B, N), torch.uint8)
    ctx.add("krrn_umeyama_ransac_f32", ptr(src), ptr(dst), N, ptr(subsets), n_hyp, INLIER_FRAC, CONFIDENCE, MIN_RATIO,
            ptr(counts), ptr(scale), ptr(R), ptr(t), ptr(inl), ptr(best), ptr(mask), B)
    return scale, R, t, {"inliers": inl, "best_hyp": best, "hyp_counts": counts, "mask": mask, "subsets": subsets}


def solve(src: torch.Tensor, dst: torch.Tensor, subsets: Optional[torch.Tensor] = None, n_hyp: int = N_HYP,
          seed: Optional[torch.Tensor] = None, stream_id: int = RngStream.UMEYAMA_OWN):
    """src / dst f32 [B, N, 3] contiguous GPU tensors -> (scale, R, t, info) device buffers. Without
    `subsets` they are drawn from `seed` (default: this module's own counter), which is then advanced."""
    dev = src.device
    B, N, _ = src.shape
    ctx = Immediate(dev)
    if subsets is not None:
        subsets = h2d(subsets.reshape(B, -1, 5), dev, torch.int32)
        return ransac_step(ctx, src, dst, B, N, subsets.shape[1], subsets)
    seed = device_seed(_seeds, dev) if seed is None else seed
    out = ransac_step(ctx, src, dst, B, N, n_hyp, None, seed, stream_id)
    ctx.add("krrn_rng_advance", ptr(seed))
    return out


def estimateSimilarityTransform(source: torch.Tensor, target: torch.Tensor, subsets: Optional[torch.Tensor] = None,
                                n_hyp: int = N_HYP, return_info: bool = False):
    if not (isinstance(source, torch.Tensor) and isinstance(target, torch.Tensor) and source.is_cuda and target.is_cuda):
        raise RuntimeError("estimateSimilarityTransform runs on the HIP path only (source / target must be GPU tensors)")
    if source.dim() == 2:
        source, target = source[None], target[None]
    if source.dim() != 3 or source.shape[-1] != 3 or source.shape != target.shape:
        raise ValueError("Source and Target must be [B, N, 3] (or [N, 3]) with the same number of points.")
    src = source.to(torch.float32).contiguous()
    dst = target.to(device=src.device, dtype=torch.float32).contiguous()
    scale, R, t, info = solve(src, dst, subsets, n_hyp)
    B = src.shape[0]
    T = torch.zeros((B, 4, 4), dtype=torch.float32, device=src.device)
    T[:, :3, :3] = scale[:, None, None] * R
    T[:, :3, 3] = t
    T[:, 3, 3] = 1.0
    if return_info:
        return scale, R, t, T, info
    return scale, R, t, T
