"""The zoom-in pass's windows: re-crop each object about its estimated pose, on the GPU.

A detector's box is loose, tight or off-centre by amounts the network never saw in its ground-truth-centred crops.
The usual test-time remedy is a second look: project the object under the first pose estimate, cut a fresh square
window centred on that projection and run the network again. `pose_windows` computes those windows on the device
(include/krrn_hip.h: krrn_pose_windows_f64) in the form the resized input kernels read from device memory, so a pose
computed on the GPU re-crops without a read-back: PoseDataset.zoom_batch, evaluate.test_epoch(..., zoom=n).

ZOOM_PAD and ZOOM_MIN_SIDE are design choices, not measurements: the repository holds no trained weights, so whether
the second pass improves any accuracy figure is unmeasured."""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from . import _lib
from .runtime import h2d, ptr, stream_ptr

# the window's side is the projected points' larger extent times ZOOM_PAD, at least ZOOM_MIN_SIDE pixels
ZOOM_PAD = 1.2
ZOOM_MIN_SIDE = 40
# pose_windows' status values
STATUS_RECROPPED, STATUS_BAD_POSE, STATUS_OUTSIDE = 0, 1, 2


def pose_windows(model_points: torch.Tensor, R: torch.Tensor, t: torch.Tensor, K4: torch.Tensor,
                 frame_hw: Tuple[int, int], rc_prev: torch.Tensor, side_prev: torch.Tensor, T: int,
                 pad: float = ZOOM_PAD, min_side: int = ZOOM_MIN_SIDE) -> Dict[str, torch.Tensor]:
    """krrn_pose_windows_f64 for B crops: model_points f32 [B, P, 3] (metres), the pose R [B, 3, 3] and t [B, 3]
    (staged as f64 on the device, as bop._poses stages the BOP kernels' poses), K4 f32 [B, 4], the frame's (H, W), the
    windows in use rc_prev int32 [B, 2] = (r0, c0) and side_prev int32 [B], and the network's side T. Returns device
    tensors: rc int32 [B, 2] and side int32 [B] (what krrn_crop_inputs_resize_u8 / krrn_choose_points_resize read),
    bbox f32 [B, 4] = (r0, r0 + S, c0, c0 + S), resize_scale f32 [B], resize_intrinsic f32 [B, 4]
    (dataset.resize_intrinsic's values) and status int32 [B]: 0 a new window; 1 a pose that puts a point at or behind
    the camera or projects it to a non-finite pixel; 2 a projection that misses the frame. Rows with status != 0 keep
    the previous window. Queued on the current stream; nothing is read back."""
    if not (model_points.is_cuda and rc_prev.is_cuda and side_prev.is_cuda):
        raise RuntimeError("pose_windows runs on the HIP path only (model_points / rc_prev / side_prev must be GPU "
                           "tensors)")
    if model_points.dim() != 3 or model_points.shape[2] != 3:
        raise ValueError(f"model_points is [B, P, 3], got {tuple(model_points.shape)}")
    dev = model_points.device
    B, P = int(model_points.shape[0]), int(model_points.shape[1])
    H, W = int(frame_hw[0]), int(frame_hw[1])
    if tuple(rc_prev.shape) != (B, 2) or tuple(side_prev.shape) != (B,) or K4.numel() != 4 * B:
        raise ValueError(f"one previous window and one K4 row per crop: {B} crops, rc {tuple(rc_prev.shape)}, side "
                         f"{tuple(side_prev.shape)}, K4 {tuple(K4.shape)}")
    pts = h2d(model_points, dev, torch.float32)
    Rd = h2d(R, dev, torch.float64).reshape(B, 9).contiguous()
    td = h2d(t, dev, torch.float64).reshape(B, 3).contiguous()
    Kd = h2d(K4, dev, torch.float32).reshape(B, 4).contiguous()
    rc_in = h2d(rc_prev, dev, torch.int32)
    side_in = h2d(side_prev, dev, torch.int32)
    out = {"rc": torch.empty((B, 2), dtype=torch.int32, device=dev),
           "side": torch.empty((B,), dtype=torch.int32, device=dev),
           "bbox": torch.empty((B, 4), dtype=torch.float32, device=dev),
           "resize_scale": torch.empty((B,), dtype=torch.float32, device=dev),
           "resize_intrinsic": torch.empty((B, 4), dtype=torch.float32, device=dev),
           "status": torch.empty((B,), dtype=torch.int32, device=dev)}
    _lib.call("krrn_pose_windows_f64", ptr(pts), P, ptr(Rd), ptr(td), ptr(Kd), H, W, int(T), float(pad), int(min_side),
              ptr(rc_in), ptr(side_in), B, ptr(out["rc"]), ptr(out["side"]), ptr(out["bbox"]), ptr(out["resize_scale"]),
              ptr(out["resize_intrinsic"]), ptr(out["status"]), stream_ptr(dev))
    return out
