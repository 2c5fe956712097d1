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

from .runtime import P, h2d, ptr
from . import _lib

N_HYP = 128          # maxIter (:21)
INLIER_FRAC = 0.1    # InlierT = SourceDiameter / 10 (:20)
CONFIDENCE = 0.99    # (:22)
MIN_RATIO = 0.1      # (:50)
MAX_POINTS = 4096    # kUmeMaxN of csrc/umeyama.hip
SUBSET_STREAM = 8    # counter-RNG stream of this module's draws (krrn.py: 0-4, pose.py: 5-7, 9, 10)

_seeds: Dict[int, torch.Tensor] = {}


def _seed(device) -> torch.Tensor:
    idx = device.index or 0
    if idx not in _seeds:
        _seeds[idx] = torch.zeros(1, dtype=torch.int64, device=device)
    return _seeds[idx]


def solve(src: torch.Tensor, dst: torch.Tensor, subsets: Optional[torch.Tensor] = None, n_hyp: int = N_HYP,
          seed: Optional[torch.Tensor] = None, stream_id: int = SUBSET_STREAM):
    """src / dst f32 [B, N, 3] contiguous GPU tensors -> (scale, R, t, info) device buffers."""
    dev = src.device
    B, N, _ = src.shape
    stream = P(torch.cuda.current_stream(dev).cuda_stream)
    lib = _lib.lib()
    if subsets is None:
        subsets = torch.empty((B, n_hyp, 5), dtype=torch.int32, device=dev)
        seed = _seed(dev) if seed is None else seed
        _lib.check(lib.krrn_ransac_subsets(ptr(seed), stream_id, B, n_hyp, N, ptr(subsets), stream),
                   "krrn_ransac_subsets")
        _lib.check(lib.krrn_rng_advance(ptr(seed), stream), "krrn_rng_advance")
    else:
        subsets = h2d(subsets.reshape(B, -1, 5), dev, torch.int32)
        n_hyp = subsets.shape[1]
    scale = torch.empty((B,), dtype=torch.float32, device=dev)
    R = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    t = torch.empty((B, 3), dtype=torch.float32, device=dev)
    inl = torch.empty((B,), dtype=torch.int32, device=dev)
    best = torch.empty((B,), dtype=torch.int32, device=dev)
    counts = torch.empty((B, n_hyp), dtype=torch.int32, device=dev)
    mask = torch.empty((B, N), dtype=torch.uint8, device=dev)
    _lib.check(lib.krrn_umeyama_ransac_f32(ptr(src), ptr(dst), N, ptr(subsets), n_hyp, INLIER_FRAC, CONFIDENCE,
                                           MIN_RATIO, ptr(counts), ptr(scale), ptr(R), ptr(t), ptr(inl), ptr(best),
                                           ptr(mask), B, stream), "krrn_umeyama_ransac_f32")
    return scale, R, t, {"inliers": inl, "best_hyp": best, "hyp_counts": counts, "mask": mask, "subsets": subsets}


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
