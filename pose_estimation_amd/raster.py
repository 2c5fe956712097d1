"""Ground-truth map rendering on the GPU: the per-pixel model coordinate, normal, region label and
coverage of an object mesh under its GT pose (krrn_raster_maps_f32), and the loader's pointwise masking
of them (krrn_gt_maps_finish_f32). The reference unpickles these maps from an offline renderer that is
not in its tree (dataset/linemod/batchdataset.py:200-210); the definition is this project's own
(include/krrn_hip.h; tests/raster_ref.py restates it in numpy).

    maps = render_maps(verts, faces, face_range, R, t, K4, boxes, region_pts)
    # verts [Vtot, 3] metres, faces [Ftot, 3] indices into verts, face_range [B, 2] = first face, count;
    # R [B, 3, 3], t [B, 3] model to camera; K4 [B, 4] = fx fy cx cy; boxes = B x (rmin, rmax, cmin, cmax)
    # of one size S; region_pts [B, NR, 3] metres -> face, depth, region [B, S, S]; coord, normal [B, 3, S, S]
    pts = region_points(verts, 64)          # FPS from index 0 (sample_model.py:33-46): the region centres

Two stated departures from the reference's offline maps: normals are the faces' flat unit normals in the
camera frame, turned towards the camera; and finish_maps masks by coverage, not by `coordinate != 0`.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from .fps import farthest_point_sampling
from .runtime import h2d, ptr, stream_ptr

MAX_S = 480          # kRastMaxS of csrc/raster.hip
MAX_REGIONS = 256    # kRastMaxNR
N_REGIONS = 64       # the region head's classes (batchdataset.py:105's fps_64)


def region_points(verts: torch.Tensor, n: int = N_REGIONS) -> torch.Tensor:
    """The n farthest-point samples of verts [V, 3] (GPU), starting at index 0, f32 [n, 3]."""
    v = verts.to(torch.float32).contiguous()
    if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] < n:
        raise ValueError(f"verts must be [V, 3] with V >= {n}, got {tuple(verts.shape)}")
    return v.index_select(0, farthest_point_sampling(v, n))


def render_maps(verts: torch.Tensor, faces: torch.Tensor, face_range: torch.Tensor, R: torch.Tensor, t: torch.Tensor,
                K4: torch.Tensor, boxes: Sequence[Tuple[int, int, int, int]], region_pts: torch.Tensor,
                frame_hw: Optional[Tuple[int, int]] = None) -> Dict[str, torch.Tensor]:
    """The raw maps of B crops (module doc). verts / faces / region_pts are GPU tensors; face_range, R, t,
    K4 may be host tensors (staged here). frame_hw = (H, W) also returns `cover_frame` u8 [B, H, W]: coverage
    written at each crop's window of its own zeroed frame (build_inputs' obj_mask with frame_idx = range(B))."""
    if not (verts.is_cuda and faces.is_cuda and region_pts.is_cuda):
        raise RuntimeError("render_maps runs on the HIP path only (verts / faces / region_pts must be GPU tensors)")
    dev = verts.device
    B = len(boxes)
    sizes = {rmax - rmin for rmin, rmax, _, _ in boxes} | {cmax - cmin for _, _, cmin, cmax in boxes}
    if len(sizes) != 1:
        raise ValueError(f"one crop size per batch, got {sorted(sizes)}")
    S = sizes.pop()
    fr_host = face_range.detach().cpu().reshape(-1, 2) if not face_range.is_cuda else None
    if fr_host is not None and (fr_host.shape[0] != B or bool((fr_host < 0).any())
                                or bool((fr_host.sum(1) > faces.shape[0]).any())):
        raise ValueError(f"face_range must be [B = {B}, 2] = (first, count) inside the {faces.shape[0]} faces")
    if frame_hw is not None:
        Hf, Wf = frame_hw
        if any(b[0] < 0 or b[2] < 0 or b[0] + S > Hf or b[2] + S > Wf for b in boxes):
            raise ValueError(f"a crop window leaves the {Hf} x {Wf} frame")
    if region_pts.dim() != 3 or region_pts.shape[0] != B or region_pts.shape[2] != 3:
        raise ValueError(f"region_pts must be [B = {B}, NR, 3], got {tuple(region_pts.shape)}")
    NR = region_pts.shape[1]
    # every converted operand stays bound until the launch is enqueued (metric.add_metric's rule)
    v = verts.to(torch.float32).contiguous()
    f = faces.to(torch.int32).contiguous()
    fr = h2d(face_range.reshape(B, 2), dev, torch.int32)
    R64 = h2d(R.reshape(B, 9), dev, torch.float64)
    t64 = h2d(t.reshape(B, 3), dev, torch.float64)
    K = h2d(K4.reshape(B, 4), dev, torch.float32)
    rc = h2d(torch.tensor([[b[0], b[2]] for b in boxes], dtype=torch.int32), dev)
    rp = region_pts.to(torch.float32).contiguous()
    out = {"face": torch.empty((B, S, S), dtype=torch.int32, device=dev),
           "depth": torch.empty((B, S, S), dtype=torch.float32, device=dev),
           "coord": torch.empty((B, 3, S, S), dtype=torch.float32, device=dev),
           "normal": torch.empty((B, 3, S, S), dtype=torch.float32, device=dev),
           "region": torch.empty((B, S, S), dtype=torch.int32, device=dev)}
    cover, Hf, Wf = None, 0, 0
    if frame_hw is not None:
        Hf, Wf = frame_hw
        cover = torch.zeros((B, Hf, Wf), dtype=torch.uint8, device=dev)
        out["cover_frame"] = cover
    _lib.call("krrn_raster_maps_f32", ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(fr), ptr(R64), ptr(t64), ptr(K),
              ptr(rc), S, ptr(rp), NR, B, ptr(out["face"]), ptr(out["depth"]), ptr(out["coord"]), ptr(out["normal"]),
              ptr(out["region"]), ptr(cover), Hf, Wf, stream_ptr(dev))
    return out


def finish_maps(maps: Dict[str, torch.Tensor], point_mask: torch.Tensor, cls: torch.Tensor, extent: torch.Tensor,
                lfborder: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The loader's GT keys from render_maps' output and the crop's point mask [B, 1, S, S] u8 (label * depth
    * cover): xyz, normal [B, 3, S, S], region, multi_cls_mask [B, S, S] int64, mask, mask_obj [B, 1, S, S].
    maps["normal"] is masked in place and returned."""
    coord, normal = maps["coord"], maps["normal"]
    dev = coord.device
    B, _, S, _ = coord.shape
    pm = point_mask.to(device=dev, dtype=torch.uint8).contiguous()
    c = h2d(cls.reshape(B), dev, torch.int64)
    ext = h2d(extent.reshape(B, 3), dev, torch.float64)
    lfb = h2d(lfborder.reshape(B, 3), dev, torch.float64)
    out = {"xyz": torch.empty((B, 3, S, S), dtype=torch.float32, device=dev), "normal": normal,
           "region": torch.empty((B, S, S), dtype=torch.int64, device=dev),
           "mask": torch.empty((B, 1, S, S), dtype=torch.float32, device=dev),
           "multi_cls_mask": torch.empty((B, S, S), dtype=torch.int64, device=dev),
           "mask_obj": torch.empty((B, 1, S, S), dtype=torch.float32, device=dev)}
    _lib.call("krrn_gt_maps_finish_f32", ptr(coord), ptr(maps["region"]), ptr(maps["face"]), ptr(pm), ptr(c), ptr(ext),
              ptr(lfb), B, S * S, ptr(out["xyz"]), ptr(normal), ptr(out["region"]), ptr(out["mask"]),
              ptr(out["multi_cls_mask"]), ptr(out["mask_obj"]), stream_ptr(dev))
    return out
