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

from .runtime import Immediate, Plan, RngStream, device_seed, h2d, ptr
from . import depth_refine, icp, umeyama, verify

NUM_POINTS = 256
N_HYP = 100
THRESHOLD = 1.0
CONFIDENCE = 0.9999

_seeds: Dict[int, torch.Tensor] = {}  # this module's counters (umeyama.py's own draws keep another table)


def draw_sel(B: int, N: int, num_points: int = NUM_POINTS) -> torch.Tensor:
    """torch.randperm(N)[:num_points] per crop on the CPU generator (trainer.py:406-408)."""
    return torch.stack([torch.randperm(N)[:num_points] for _ in range(B)]).to(torch.int32)


def pnp_step(ctx, xyz: torch.Tensor, choose: torch.Tensor, B: int, N: int, xm: torch.Tensor, ym: torch.Tensor,
             K4: torch.Tensor, ext: torch.Tensor, lfb: torch.Tensor, P_: int, n_hyp: int = N_HYP,
             thr: float = THRESHOLD, sel=None, subsets=None, seed=None, sel_stream=None, subsets_stream=None):
    """The krrn_pnp_ransac_f32 launch, stated once, on `ctx` (a runtime.Plan or runtime.Immediate). Contiguous
    device tensors: xyz f32 [B, 3, H, W], choose i64 [B, N], xm / ym f32 [B, N], K4 f32 [B, 4], ext / lfb f64 [B, 3],
    sel int32 [B, P_], subsets int32 [B, n_hyp, 5]; without `sel` / `subsets` they are drawn through `ctx` from
    `seed` on counter streams `sel_stream` / `subsets_stream` (the caller advances the seed). Returns buffers."""
    H, W = xyz.shape[2], xyz.shape[3]
    if sel is None:
        sel = ctx.buf((B, P_), torch.int32)
        ctx.add("krrn_randperm_i32", ptr(seed), int(sel_stream), N, P_, B, ptr(sel))
    if subsets is None:
        subsets = ctx.buf((B, n_hyp, 5), torch.int32)
        ctx.add("krrn_ransac_subsets", ptr(seed), int(subsets_stream), B, n_hyp, P_, ptr(subsets))
    R = ctx.buf((B, 3, 3))
    t = ctx.buf((B, 3))
    inl = ctx.buf((B,), torch.int32)
    mask = ctx.buf((B, P_), torch.uint8)
    ws = ctx.buf((B * n_hyp * 13,))
    ctx.add("krrn_pnp_ransac_f32", ptr(xyz), H * W, ptr(choose), N, ptr(sel), P_, ptr(xm), ptr(ym), ptr(K4), ptr(ext),
            ptr(lfb), ptr(subsets), n_hyp, float(thr), CONFIDENCE, ptr(ws), ptr(R), ptr(t), ptr(inl), ptr(mask), B)
    return R, t, inl, dict(sel=sel, subsets=subsets, mask=mask, workspace=ws)


def model_points_step(ctx, xyz: torch.Tensor, choose: torch.Tensor, B: int, N: int, ext: torch.Tensor,
                      lfb: torch.Tensor) -> torch.Tensor:
    """The krrn_model_points_f32 launch: src f32 [B, N, 3] = xyz * extent + lfborder at the chosen pixels."""
    src = ctx.buf((B, N, 3))
    ctx.add("krrn_model_points_f32", ptr(xyz), xyz.shape[2] * xyz.shape[3], ptr(choose), N, ptr(ext), ptr(lfb),
            ptr(src), B)
    return src


def get_pose(pred, data, num_points: int = NUM_POINTS, n_hyp: int = N_HYP, thr: float = THRESHOLD,
             sel: Optional[torch.Tensor] = None, subsets: Optional[torch.Tensor] = None, return_info: bool = False):
    xyz = pred["xyz"]
    if not xyz.is_cuda:
        raise RuntimeError("get_pose runs on the HIP path only (pred['xyz'] must be a GPU tensor)")
    dev = xyz.device
    xyz = xyz.contiguous()
    B = xyz.shape[0]
    choose = h2d(data["choose"].reshape(B, -1), dev, torch.int64)
    N = choose.shape[1]
    P_ = min(num_points, N)
    if sel is None:
        sel = draw_sel(B, N, P_)
    sel = h2d(sel.reshape(B, P_), dev, torch.int32)
    xm, ym = (h2d(data[k].reshape(B, N), dev, torch.float32) for k in ("x_map_choosed", "y_map_choosed"))
    K4 = h2d(data["intrinsic"].reshape(B, 4), dev, torch.float32)
    ext, lfb = (h2d(data[k].reshape(B, 3), dev, torch.float64) for k in ("extent", "lfborder"))
    ctx = Immediate(dev)
    seed = device_seed(_seeds, dev) if subsets is None else None
    if subsets is not None:
        subsets = h2d(subsets.reshape(B, -1, 5), dev, torch.int32)
        n_hyp = subsets.shape[1]
    R, t, inl, info = pnp_step(ctx, xyz, choose, B, N, xm, ym, K4, ext, lfb, P_, n_hyp, thr, sel, subsets, seed,
                               subsets_stream=RngStream.PNP_SUBSETS)
    if seed is not None:
        ctx.add("krrn_rng_advance", ptr(seed))
    if return_info:
        return R, t, dict(info, inliers=inl)
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
    B = xyz.shape[0]
    choose = h2d(data["choose"].reshape(B, -1), dev, torch.int64)
    N = choose.shape[1]
    cloud = h2d(data["cloud"].reshape(B, N, 3), dev, torch.float32)
    ext, lfb = (h2d(data[k].reshape(B, 3), dev, torch.float64) for k in ("extent", "lfborder"))
    src = model_points_step(Immediate(dev), xyz, choose, B, N, ext, lfb)
    scale, R, t, info = umeyama.solve(src, cloud, subsets, n_hyp, seed=device_seed(_seeds, dev),
                                      stream_id=RngStream.UMEYAMA_POSE)
    if return_info:
        info.update(scale=scale, src=src)
        return R, t, info
    return R, t


def add_umeyama_ops(plan: Plan, xyz: torch.Tensor, choose: torch.Tensor, cloud: torch.Tensor, B: int, N: int,
                    ext: torch.Tensor, lfb: torch.Tensor, seed: torch.Tensor, n_hyp: int = umeyama.N_HYP):
    """Append the Umeyama-RANSAC pose step to a plan (graph-capturable: subsets drawn on the device from
    `seed`; the caller's plan advances the seed). Returns (R, t, inliers, info) buffers; info holds
    scale, src, subsets, hyp_counts, best_hyp, mask."""
    src = model_points_step(plan, xyz, choose, B, N, ext, lfb)
    scale, R, t, info = umeyama.ransac_step(plan, src, cloud, B, N, n_hyp, seed=seed,
                                            stream_id=RngStream.UMEYAMA_PLAN)
    inl = info.pop("inliers")
    return R, t, inl, dict(info, scale=scale, src=src)


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
    cloud = h2d(data["cloud"].reshape(B, -1, 3), dev, torch.float32)
    mp = h2d(data["model_points"].reshape(B, -1, 3), dev, torch.float32)
    return icp.refine(R, t.reshape(B, 3), cloud, mp, max_dist, max_iter, tol, min_pairs, return_info)


def select_pose(cands, data, dataset, tau=None):
    """The best of several pose candidates per crop, by render-and-compare against the observed depth and the
    detector's mask (verify.score_poses; include/krrn_hip.h: krrn_pose_score_f32). `cands` is a list of 1 .. 8
    (R [B, 3, 3], t [B, 3]) GPU tensor pairs in priority order (ties keep the earlier one); `data` is
    dataset.batch(indices, device, verify=True); tau metres (a float or [B]; default verify.TAU). Returns {"R" f32
    [B, 3, 3], "t" f32 [B, 3]: the winner's pose, "best" int32 [B], "score" f64 [B, C], "counts" int32 [B, C, 6]}.
    Queued on the current stream, nothing is read back: the candidates may come straight from their solvers."""
    if "verify_mask" not in data:
        raise ValueError("select_pose needs a batch made with dataset.batch(indices, device, verify=True)")
    if not cands:
        raise ValueError("select_pose needs at least one candidate")
    dev = cands[0][1].device
    if dev.type != "cuda":
        raise RuntimeError("select_pose runs on the HIP path only (GPU tensors)")
    B = cands[0][1].reshape(-1, 3).shape[0]
    R = torch.stack([r.reshape(B, 3, 3).to(torch.float64) for r, _ in cands], 1)
    t = torch.stack([x.reshape(B, 3).to(torch.float64) for _, x in cands], 1)
    mesh = dataset._mesh_for(dev)
    out = verify.score_poses(mesh["verts"], mesh["faces"], data["bop_face_range"], R, t, data["intrinsic"],
                             data["bop_depth"], data["bop_frame"], verify.TAU if tau is None else tau,
                             mask=data["verify_mask"], box=data["bbox"].to(torch.int32))
    return {"R": out["R"], "t": out["t"], "best": out["best"], "score": out["score"], "counts": out["counts"]}


def refine_pose_depth(R: torch.Tensor, t: torch.Tensor, data, dataset, diameter, use_mask: bool = False,
                      max_dist=None, radius=None, max_iter: int = depth_refine.MAX_ITER,
                      tol: float = depth_refine.TOL, min_pairs: int = depth_refine.MIN_PAIRS,
                      damp: float = depth_refine.DAMP, return_info: bool = False):
    """(R [B, 3, 3], t [B, 3]) polished by render-based point-to-plane refinement on the observed depth frame
    (depth_refine.refine; include/krrn_hip.h: krrn_pose_refine_depth_f32). `data` is dataset.batch(indices, device,
    verify=True); `diameter` per crop (a float or a [B] tensor, metres) gives max_dist = depth_refine.DIST_FRAC x
    diameter and the twist's radius = diameter / 2 unless they are given. use_mask keeps only pixels of the crop's
    mask_label frame. Queued on the current stream, nothing is read back. The reference has no such step: the
    defaults are this project's choices (depth_refine.py)."""
    if "verify_mask" not in data or "bop_depth" not in data:
        raise ValueError("refine_pose_depth needs a batch made with dataset.batch(indices, device, verify=True)")
    if not (isinstance(R, torch.Tensor) and isinstance(t, torch.Tensor) and R.is_cuda and t.is_cuda):
        raise RuntimeError("refine_pose_depth runs on the HIP path only (R / t must be GPU tensors)")
    dia = diameter.to(torch.float64) if isinstance(diameter, torch.Tensor) else float(diameter)
    if max_dist is None:
        max_dist = depth_refine.DIST_FRAC * dia
    if radius is None:
        radius = depth_refine.RADIUS_FRAC * dia
    dev = R.device
    B = R.shape[0]
    mesh = dataset._mesh_for(dev)
    return depth_refine.refine(mesh["verts"], mesh["faces"], data["bop_face_range"], R, t.reshape(B, 3),
                               data["intrinsic"], data["bop_depth"], data["bop_frame"], max_dist, radius,
                               mask=data["verify_mask"] if use_mask else None, max_iter=max_iter, tol=tol,
                               min_pairs=min_pairs, damp=damp, return_info=return_info)


def add_icp_ops(plan: Plan, R: torch.Tensor, t: torch.Tensor, cloud: torch.Tensor, model: torch.Tensor,
                max_dist: torch.Tensor, B: int, N: int, M: int, max_iter: int = icp.MAX_ITER, tol: float = icp.TOL,
                min_pairs: int = icp.MIN_PAIRS):
    """Append the ICP refinement to a plan (graph-capturable: one launch, no host decision). R [B, 3, 3],
    t [B, 3], cloud [B, N, 3], model [B, M, 3], max_dist [B]: f32 contiguous device buffers read at run
    time. Returns (R, t, info) buffers; info holds passes, pairs, rmse, status, nn_idx."""
    return icp.refine_step(plan, R, t, cloud, model, max_dist, B, N, M, max_iter, tol, min_pairs)


def add_pose_ops(plan: Plan, xyz: torch.Tensor, choose: torch.Tensor, B: int, N: int, xm: torch.Tensor,
                 ym: torch.Tensor, K4: torch.Tensor, ext: torch.Tensor, lfb: torch.Tensor, seed: torch.Tensor,
                 num_points: int = NUM_POINTS, n_hyp: int = N_HYP, thr: float = THRESHOLD):
    """Append the pose step to a plan (graph-capturable: choose subset and RANSAC subsets drawn
    on the device; the caller's plan advances the seed). Returns (R, t, inliers) buffers."""
    R, t, inl, info = pnp_step(plan, xyz, choose, B, N, xm, ym, K4, ext, lfb, min(num_points, N), n_hyp, thr,
                               seed=seed, sel_stream=RngStream.PNP_PLAN_SEL,
                               subsets_stream=RngStream.PNP_PLAN_SUBSETS)
    return R, t, inl, dict(sel=info["sel"], subsets=info["subsets"], mask=info["mask"])
