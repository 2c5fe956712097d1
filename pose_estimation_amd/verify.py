"""Pose verification by render-and-compare on the GPU (krrn_pose_score_f32; include/krrn_hip.h states the
definition, tests/verify_ref.py restates it in numpy): C candidate poses per crop are rendered with VSD's depth
walk, compared with the observed depth frame and the detector's mask, and the best is kept. No ground-truth pose
is involved: the score is a depth-aware IoU between what a pose claims is visible and where the mask has depth.

    out = score_poses(verts, faces, face_range, R, t, K4, depth, frame, mask=mask, box=box)
    # R [B, C, 3, 3], t [B, C, 3] -> {"counts": int32 [B, C, 6] in the order of COUNTS, "score": f64 [B, C],
    #   "best": int32 [B], "R": f32 [B, 3, 3], "t": f32 [B, 3] (candidate best[b]'s pose)}

pose.select_pose(cands, data, dataset) is the same over a batch made with dataset.batch(..., verify=True);
evaluate.test_epoch(..., select="depth") uses it per crop.
"""
from __future__ import annotations

from typing import Dict, Optional, Union

import torch

from . import _lib
from .bop import DELTA, per_crop, stage_scene
from .runtime import h2d, ptr, stream_ptr

TAU = DELTA                                             # metres: the tolerance BOP uses for the same question
MAX_C = 8                                               # kVerMaxC of csrc/verify.hip
COUNTS = ("render", "claim", "evid", "both", "inter", "union")


def score_poses(verts: torch.Tensor, faces: torch.Tensor, face_range: torch.Tensor, R: torch.Tensor, t: torch.Tensor,
                K4: torch.Tensor, depth: torch.Tensor, frame: torch.Tensor,
                tau: Union[float, torch.Tensor] = TAU, mask: Optional[torch.Tensor] = None,
                box: Optional[torch.Tensor] = None, depth_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """krrn_pose_score_f32 for B crops with C candidates each (module doc). verts [Vtot, 3] / faces [Ftot, 3] /
    depth [F, H, W] / mask u8 [F, H, W] are GPU tensors; face_range [B, 2], R [B, C, 3, 3], t [B, C, 3], K4 [B, 4],
    frame [B], box [B, 4] = (rmin, rmax, cmin, cmax) and tau (a float or [B], metres) may be host tensors (staged
    here). Nothing is read back: the candidates may come straight from a solver's launch."""
    # every converted operand stays bound until the launch is enqueued (metric.add_metric's rule)
    s = stage_scene("score_poses", verts, faces, face_range, K4, depth, frame, mask)
    dev, B = verts.device, s.B
    if t.dim() != 3 or t.shape[0] != B or t.shape[2] != 3:
        raise ValueError(f"t must be [B, C, 3] with B = {B}, got {tuple(t.shape)}")
    C = int(t.shape[1])
    if not 1 <= C <= MAX_C:
        raise ValueError(f"1 .. {MAX_C} candidates, got {C}")
    Rd = h2d(R, dev, torch.float64).reshape(B, C, 9).contiguous()
    td = h2d(t, dev, torch.float64).reshape(B, C, 3).contiguous()
    bx = h2d(box.reshape(B, 4), dev, torch.int32) if box is not None else None
    ta = per_crop(tau, B, dev, "tau")
    ws = torch.empty((B, C, 4), dtype=torch.int32, device=dev)        # krrn_pose_score_ws(B, C)
    out = {"counts": torch.empty((B, C, len(COUNTS)), dtype=torch.int32, device=dev),
           "score": torch.empty((B, C), dtype=torch.float64, device=dev),
           "best": torch.empty((B,), dtype=torch.int32, device=dev),
           "R": torch.empty((B, 3, 3), dtype=torch.float32, device=dev),
           "t": torch.empty((B, 3), dtype=torch.float32, device=dev)}
    _lib.call("krrn_pose_score_f32", ptr(s.v), s.v.shape[0], ptr(s.f), s.f.shape[0], ptr(s.fr), ptr(Rd), ptr(td), C,
              ptr(s.K), ptr(s.d), ptr(s.m), s.F, s.H, s.W, ptr(s.fi), ptr(bx), float(depth_scale), ptr(ta), B, ptr(ws),
              ptr(out["counts"]), ptr(out["score"]), ptr(out["best"]), ptr(out["R"]), ptr(out["t"]), stream_ptr(dev))
    return out
