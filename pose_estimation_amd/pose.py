"""Rotation by PnP-RANSAC on the reconstructed correspondences: Trainer.get_pose
(tools/trainer.py:383-438), batched and on the GPU (krrn_pnp_ransac_f32).

    R, t = get_pose(pred, data)          # R [B, 3, 3], t [B, 3] (PnP translation)

Reference semantics kept: 256 of the N chosen pixels per crop (torch.randperm on the CPU
generator, :406-408), object points = xyz * extent + lfborder (f64, :415-421), image points
= full-frame (x, y) of the same pixels, EPnP hypotheses, 1 px reprojection threshold,
EPnP refinement on the inliers, R as a matrix (the rvec -> kornia Rodrigues step is an
identity on R). The reference asserts B == 1 (:402); any B works here, one workgroup per crop.
RANSAC: H = 100 hypotheses per crop (cv2's default iterationsCount), drawn on the device
(krrn_ransac_subsets) unless given explicitly, scored in parallel and selected by cv2's own loop
(in order, stopping at its adaptive iteration count for confidence 0.9999, :426).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .runtime import P, Plan, h2d, ptr
from . import _lib, icp, umeyama

NUM_POINTS = 256
N_HYP = 100
THRESHOLD = 1.0
CONFIDENCE = 0.9999
# counter-RNG stream ids (krrn.py's pool draws use 0-4, the PnP step 5-7, umeyama.py's own draws 8)
UMEYAMA_STREAM = 9
UMEYAMA_PLAN_STREAM = 10

_seeds: Dict[int, torch.Tensor] = {}


def _seed(device) -> torch.Tensor:
    idx = device.index or 0
    if idx not in _seeds:
        _seeds[idx] = torch.zeros(1, dtype=torch.int64, device=device)
    return _seeds[idx]


def _dev(t: torch.Tensor, device, dtype=None) -> torch.Tensor:
    return h2d(t, device, dtype)


def draw_sel(B: int, N: int, num_points: int = NUM_POINTS) -> torch.Tensor:
    """torch.randperm(N)[:num_points] per crop on the CPU generator (trainer.py:406-408)."""
    return torch.stack([torch.randperm(N)[:num_points] for _ in range(B)]).to(torch.int32)


def get_pose(pred, data, num_points: int = NUM_POINTS, n_hyp: int = N_HYP, thr: float = THRESHOLD,
             sel: Optional[torch.Tensor] = None, subsets: Optional[torch.Tensor] = None, return_info: bool = False):
    xyz = pred["xyz"]
    if not xyz.is_cuda:
        raise RuntimeError("get_pose runs on the HIP path only (pred['xyz'] must be a GPU tensor)")
    dev = xyz.device
    xyz = xyz.contiguous()
    B, _, H, W = xyz.shape
    choose = _dev(data["choose"].reshape(B, -1), dev, torch.int64)
    N = choose.shape[1]
    P_ = min(num_points, N)
    if sel is None:
        sel = draw_sel(B, N, P_)
    sel = _dev(sel.reshape(B, P_), dev, torch.int32)
    xm = _dev(data["x_map_choosed"].reshape(B, N), dev, torch.float32)
    ym = _dev(data["y_map_choosed"].reshape(B, N), dev, torch.float32)
    K4 = _dev(data["intrinsic"].reshape(B, 4), dev, torch.float32)
    ext = _dev(data["extent"].reshape(B, 3), dev, torch.float64)
    lfb = _dev(data["lfborder"].reshape(B, 3), dev, torch.float64)
    stream = P(torch.cuda.current_stream(dev).cuda_stream)
    lib = _lib.lib()
    if subsets is None:
        subsets = torch.empty((B, n_hyp, 5), dtype=torch.int32, device=dev)
        seed = _seed(dev)
        _lib.check(lib.krrn_ransac_subsets(ptr(seed), 7, B, n_hyp, P_, ptr(subsets), stream), "krrn_ransac_subsets")
        _lib.check(lib.krrn_rng_advance(ptr(seed), stream), "krrn_rng_advance")
    else:
        subsets = _dev(subsets.reshape(B, -1, 5), dev, torch.int32)
        n_hyp = subsets.shape[1]
    R = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    t = torch.empty((B, 3), dtype=torch.float32, device=dev)
    inl = torch.empty((B,), dtype=torch.int32, device=dev)
    mask = torch.empty((B, P_), dtype=torch.uint8, device=dev)
    ws = torch.empty((B * n_hyp * 13,), dtype=torch.float32, device=dev)
    _lib.check(lib.krrn_pnp_ransac_f32(ptr(xyz), H * W, ptr(choose), N, ptr(sel), P_, ptr(xm), ptr(ym), ptr(K4),
                                       ptr(ext), ptr(lfb), ptr(subsets), n_hyp, float(thr), CONFIDENCE, ptr(ws), ptr(R), ptr(t),
                                       ptr(inl), ptr(mask), B, stream), "krrn_pnp_ransac_f32")
    if return_info:
        return R, t, {"inliers": inl, "mask": mask, "sel": sel, "subsets": subsets, "workspace": ws}
    return R, t


def get_pose_umeyama(pred, data, n_hyp: int = umeyama.N_HYP, subsets: Optional[torch.Tensor] = None,
                     return_info: bool = False):
    """(R [B, 3, 3], t [B, 3]) from the depth: Umeyama-RANSAC (umeyama.estimateSimilarityTransform,
    lib/transform/umeyama.py:8-98) on the 3D-3D pairs tools/script/eval.py:128,151 feeds it:
    source = model coordinates of all N chosen pixels (xyz * extent + lfborder, f64 then f32,
    krrn_model_points_f32), target = data['cloud']. `info` carries the similarity's `scale`, `src`, and the
    solver's inliers / best_hyp / hyp_counts / mask / subsets; a failed crop has inliers == 0, R = I, t = 0.
    Without `subsets` [B, H, 5] the samples are drawn on the device (krrn_ransac_subsets: 5 DISTINCT
    indices per hypothesis, where the reference's np.random.randint draws with replacement);
    explicit subsets cover exact parity with the reference."""
    xyz = pred["xyz"]
    if not xyz.is_cuda:
        raise RuntimeError("get_pose_umeyama runs on the HIP path only (pred['xyz'] must be a GPU tensor)")
    dev = xyz.device
    xyz = xyz.to(torch.float32).contiguous()
    B, _, H, W = xyz.shape
    choose = _dev(data["choose"].reshape(B, -1), dev, torch.int64)
    N = choose.shape[1]
    cloud = _dev(data["cloud"].reshape(B, N, 3), dev, torch.float32)
    ext = _dev(data["extent"].reshape(B, 3), dev, torch.float64)
    lfb = _dev(data["lfborder"].reshape(B, 3), dev, torch.float64)
    stream = P(torch.cuda.current_stream(dev).cuda_stream)
    src = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().krrn_model_points_f32(ptr(xyz), H * W, ptr(choose), N, ptr(ext), ptr(lfb), ptr(src), B,
                                                stream), "krrn_model_points_f32")
    scale, R, t, info = umeyama.solve(src, cloud, subsets, n_hyp, seed=_seed(dev), stream_id=UMEYAMA_STREAM)
    if return_info:
        info.update(scale=scale, src=src)
        return R, t, info
    return R, t


def add_umeyama_ops(plan: Plan, xyz: torch.Tensor, choose: torch.Tensor, cloud: torch.Tensor, B: int, N: int,
                    ext: torch.Tensor, lfb: torch.Tensor, seed: torch.Tensor, n_hyp: int = umeyama.N_HYP):
    """Append the Umeyama-RANSAC pose step to a plan (graph-capturable: subsets drawn on the device from
    `seed`; the caller's plan advances the seed). Returns (R, t, inliers, info) buffers; info holds
    scale, src, subsets, hyp_counts, best_hyp, mask."""
    H, W = xyz.shape[2], xyz.shape[3]
    src = plan.buf((B, N, 3))
    subsets = plan.buf((B, n_hyp, 5), torch.int32)
    counts = plan.buf((B, n_hyp), torch.int32)
    scale = plan.buf((B,))
    R = plan.buf((B, 3, 3))
    t = plan.buf((B, 3))
    inl = plan.buf((B,), torch.int32)
    best = plan.buf((B,), torch.int32)
    mask = plan.buf((B, N), torch.uint8)
    plan.add("krrn_model_points_f32", ptr(xyz), H * W, ptr(choose), N, ptr(ext), ptr(lfb), ptr(src), B)
    plan.add("krrn_ransac_subsets", ptr(seed), UMEYAMA_PLAN_STREAM, B, n_hyp, N, ptr(subsets))
    plan.add("krrn_umeyama_ransac_f32", ptr(src), ptr(cloud), N, ptr(subsets), n_hyp, umeyama.INLIER_FRAC,
             umeyama.CONFIDENCE, umeyama.MIN_RATIO, ptr(counts), ptr(scale), ptr(R), ptr(t), ptr(inl), ptr(best),
             ptr(mask), B)
    return R, t, inl, dict(scale=scale, src=src, subsets=subsets, hyp_counts=counts, best_hyp=best, mask=mask)


def refine_pose_icp(R: torch.Tensor, t: torch.Tensor, data, diameter=None, max_dist=None,
                    max_iter: int = icp.MAX_ITER, tol: float = icp.TOL, min_pairs: int = icp.MIN_PAIRS,
                    return_info: bool = False):
    """(R [B, 3, 3], t [B, 3]) polished by ICP (icp.refine) of data['model_points'] against data['cloud'].
    Pairs farther apart than max_dist are rejected: icp.DIST_FRAC x `diameter` per crop (a float or a [B]
    tensor, metres), or an explicit `max_dist`; one of the two is required. The reference has no such step:
    the defaults are this project's choices (icp.py)."""
    if not (isinstance(R, torch.Tensor) and isinstance(t, torch.Tensor) and R.is_cuda and t.is_cuda):
        raise RuntimeError("refine_pose_icp runs on the HIP path only (R / t must be GPU tensors)")
    if max_dist is None:
        if diameter is None:
            raise ValueError("refine_pose_icp needs `diameter` (max_dist = icp.DIST_FRAC x diameter) or `max_dist`")
        max_dist = icp.DIST_FRAC * (diameter.to(torch.float32) if isinstance(diameter, torch.Tensor)
                                    else float(diameter))
    dev = R.device
    B = R.shape[0]
    cloud = _dev(data["cloud"].reshape(B, -1, 3), dev, torch.float32)
    mp = _dev(data["model_points"].reshape(B, -1, 3), dev, torch.float32)
    return icp.refine(R, t.reshape(B, 3), cloud, mp, max_dist, max_iter, tol, min_pairs, return_info)


def add_icp_ops(plan: Plan, R: torch.Tensor, t: torch.Tensor, cloud: torch.Tensor, model: torch.Tensor,
                max_dist: torch.Tensor, B: int, N: int, M: int, max_iter: int = icp.MAX_ITER, tol: float = icp.TOL,
                min_pairs: int = icp.MIN_PAIRS):
    """Append the ICP refinement to a plan (graph-capturable: one launch, no host decision). R [B, 3, 3],
    t [B, 3], cloud [B, N, 3], model [B, M, 3], max_dist [B]: f32 contiguous device buffers read at run
    time. Returns (R, t, info) buffers; info holds passes, pairs, rmse, status, nn_idx."""
    Ro = plan.buf((B, 3, 3))
    to = plan.buf((B, 3))
    passes = plan.buf((B,), torch.int32)
    pairs = plan.buf((B,), torch.int32)
    rmse = plan.buf((B,))
    status = plan.buf((B,), torch.int32)
    nn_idx = plan.buf((B, N), torch.int32)
    plan.add("krrn_icp_refine_f32", ptr(R), ptr(t), ptr(cloud), N, ptr(model), M, ptr(max_dist), int(max_iter),
             float(tol), int(min_pairs), ptr(Ro), ptr(to), ptr(passes), ptr(pairs), ptr(rmse), ptr(status),
             ptr(nn_idx), B)
    return Ro, to, dict(passes=passes, pairs=pairs, rmse=rmse, status=status, nn_idx=nn_idx)


def add_pose_ops(plan: Plan, xyz: torch.Tensor, choose: torch.Tensor, B: int, N: int, xm: torch.Tensor,
                 ym: torch.Tensor, K4: torch.Tensor, ext: torch.Tensor, lfb: torch.Tensor, seed: torch.Tensor,
                 num_points: int = NUM_POINTS, n_hyp: int = N_HYP, thr: float = THRESHOLD):
    """Append the pose step to a plan (graph-capturable: choose subset and RANSAC subsets drawn
    on the device). Returns (R, t, inliers) buffers."""
    H, W = xyz.shape[2], xyz.shape[3]
    P_ = min(num_points, N)
    sel = plan.buf((B, P_), torch.int32)
    subsets = plan.buf((B, n_hyp, 5), torch.int32)
    R = plan.buf((B, 3, 3))
    t = plan.buf((B, 3))
    inl = plan.buf((B,), torch.int32)
    mask = plan.buf((B, P_), torch.uint8)
    ws = plan.buf((B * n_hyp * 13,))
    plan.add("krrn_randperm_i32", ptr(seed), 5, N, P_, B, ptr(sel))
    plan.add("krrn_ransac_subsets", ptr(seed), 6, B, n_hyp, P_, ptr(subsets))
    plan.add("krrn_pnp_ransac_f32", ptr(xyz), H * W, ptr(choose), N, ptr(sel), P_, ptr(xm), ptr(ym), ptr(K4), ptr(ext),
             ptr(lfb), ptr(subsets), n_hyp, float(thr), CONFIDENCE, ptr(ws), ptr(R), ptr(t), ptr(inl), ptr(mask), B)
    return R, t, inl, dict(sel=sel, subsets=subsets, mask=mask)
