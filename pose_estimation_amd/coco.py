"""COCO's average precision, the metric of BOP's 2D detection and 2D segmentation tasks: the per-image matching on
the GPU (krrn_coco_match_f64; include/krrn_hip.h states it) and the accumulation over images on the host.

    res = match(score, det_range, gt_range, pair_off, iou, det_area, gt_area, gt_flags, device=dev)
    acc = accumulate(cat, det_range, gt_range, score, res["rank"], res["dt_match"], res["dt_ig"], res["gt_ig"], K)
    out = summarize(acc)                                 # AP, AP50, AP75, AP_small / medium / large, AR1 / 10 / 100

A group is one (scene, image, category): its detections and ground truths are two ranges, its IoUs a detection-major
block of `iou` (rle.iou or rle.box_iou over the group's pairs). bop_scene.eval_coco builds the groups from a
scene_gt_coco.json and a detection / segmentation result file.

Written from the published definitions (pycocotools' COCOeval.evaluateImg, accumulate and summarize) and not checked
against pycocotools' own output: it is not a dependency. tests/coco_ref.py restates all three loop by loop."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .bop import MATCH_MAX                               # kMatchMax of csrc/krrn_match.h: rows per side of a group
from .runtime import h2d, ptr, stream_ptr

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
AREA_RNG = np.array([[0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]])   # all, small, medium, large
AREA_NAMES = ("all", "small", "medium", "large")
MAX_DETS = (1, 10, 100)


def match(score, det_range, gt_range, pair_off, iou, det_area, gt_area, gt_flags, area_rng=AREA_RNG, iou_thr=IOU_THRS,
          max_det: int = MAX_DETS[-1], device=None, lim_det: int = MATCH_MAX, lim_gt: int = MATCH_MAX
          ) -> Dict[str, torch.Tensor]:
    """krrn_coco_match_f64 for G groups: score / det_area [Dtot], det_range / gt_range [G, 2] = (first, count),
    pair_off [G] into iou [Ptot] (detection-major per group), gt_area / gt_flags [GTtot] (bit 0 = iscrowd, bit 1 =
    ignore), area_rng [A, 2], iou_thr [T]. Operands may be host arrays / tensors (staged here) or GPU tensors;
    `device` is needed only when none of them is on a GPU. max_det is COCO's maxDets (the detections ranked at or
    past it get rank -1 and take no part); lim_det / lim_gt are the limits the caller states for the ranges, and a
    group that breaks them is matched as an empty one. Returns {"dt_match": int32 [Dtot, A, T] (the global ground
    truth index or -1), "dt_ig": u8 [Dtot, A, T], "gt_ig": u8 [GTtot, A], "rank": int32 [Dtot]} on the device.
    Nothing is read back. ValueError: shapes that do not fit together, A outside 1..8, T outside 1..16."""
    as_t = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))  # noqa: E731
    score, det_range, gt_range, pair_off, iou, det_area, gt_area, gt_flags, area_rng, iou_thr = (
        as_t(x) for x in (score, det_range, gt_range, pair_off, iou, det_area, gt_area, gt_flags, area_rng, iou_thr))
    if device is None:
        device = next((x.device for x in (iou, score, det_area) if x.is_cuda), None)
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("coco.match runs on the HIP path only (a GPU tensor or device= is needed)")
    dev = torch.device(device)
    D, GT, G, P = score.numel(), gt_area.numel(), pair_off.numel(), iou.numel()
    if det_area.numel() != D or gt_flags.numel() != GT or det_range.numel() != 2 * G or gt_range.numel() != 2 * G:
        raise ValueError(f"score / det_area must be [{D}], gt_area / gt_flags [{GT}], det_range / gt_range [{G}, 2]")
    if area_rng.dim() != 2 or area_rng.shape[1] != 2 or not 1 <= area_rng.shape[0] <= 8:
        raise ValueError(f"area_rng must be [A, 2] with 1 <= A <= 8, got {tuple(area_rng.shape)}")
    if not 1 <= iou_thr.numel() <= 16:
        raise ValueError(f"iou_thr must hold 1 .. 16 thresholds, got {iou_thr.numel()}")
    if P > 2 ** 31 - 1:
        raise ValueError(f"{P} pairs do not fit int32: match fewer groups per call")
    A, T = int(area_rng.shape[0]), int(iou_thr.numel())
    f64 = lambda x: h2d(x.reshape(-1), dev, torch.float64)  # noqa: E731
    i32 = lambda x: h2d(x.reshape(-1), dev, torch.int32)    # noqa: E731
    sc, io, da, ga, ar, th = f64(score), f64(iou), f64(det_area), f64(gt_area), f64(area_rng), f64(iou_thr)
    dr, gr, po, gf = i32(det_range), i32(gt_range), i32(pair_off), i32(gt_flags)
    out = {"dt_match": torch.empty((D, A, T), dtype=torch.int32, device=dev),
           "dt_ig": torch.empty((D, A, T), dtype=torch.uint8, device=dev),
           "gt_ig": torch.empty((GT, A), dtype=torch.uint8, device=dev),
           "rank": torch.empty((D,), dtype=torch.int32, device=dev)}
    if G == 0:
        return out
    _lib.call("krrn_coco_match_f64", ptr(sc), D, ptr(dr), ptr(gr), ptr(po), ptr(io), P, ptr(da), ptr(ga), ptr(gf), GT,
              ptr(ar), A, ptr(th), T, int(max_det), int(lim_det), int(lim_gt), G, ptr(out["dt_match"]),
              ptr(out["dt_ig"]), ptr(out["gt_ig"]), ptr(out["rank"]), stream_ptr(dev))
    return out


def accumulate(cat, det_range, gt_range, score, rank, dt_match, dt_ig, gt_ig, n_cat: int,
               max_dets: Sequence[int] = MAX_DETS) -> Dict[str, np.ndarray]:
    """pycocotools' accumulate over G groups, host numpy f64. cat [G] = each group's category index in [0, n_cat);
    det_range / gt_range [G, 2]; score / rank [Dtot]; dt_match / dt_ig [Dtot, A, T]; gt_ig [GTtot, A], as match
    returns them (read back). The groups' order is the images' order: it decides between equal scores.

    Per category k, area range a and maxDet m: the groups of k in order, each group's detections with 0 <= rank < m
    in rank order, concatenated; a stable sort by score descending; tp = matched and not dt_ig, fp = not matched and
    not dt_ig, cumulative sums; npig = the ground truths of k with gt_ig == 0 (the cell stays -1 when npig == 0); rc
    = tp / npig, pr = tp / (tp + fp + spacing(1)), pr made non-increasing from the right and sampled at
    searchsorted(rc, REC_THRS, side="left") (0 past the end); recall = rc[-1] (0 without a detection).
    Returns {"precision": f64 [T, 101, n_cat, A, M], "recall": f64 [T, n_cat, A, M]}, -1 where not defined."""
    cat, det_range, gt_range = np.asarray(cat, np.int64), np.asarray(det_range, np.int64), np.asarray(gt_range, np.int64)
    score, rank = np.asarray(score, np.float64), np.asarray(rank, np.int64)
    dt_match, dt_ig, gt_ig = np.asarray(dt_match), np.asarray(dt_ig) != 0, np.asarray(gt_ig) != 0
    A, T = int(dt_match.shape[1]), int(dt_match.shape[2])
    M, R = len(max_dets), len(REC_THRS)
    precision = -np.ones((T, R, n_cat, A, M))
    recall = -np.ones((T, n_cat, A, M))
    for k in range(n_cat):
        gs = np.flatnonzero(cat == k)
        if len(gs) == 0:
            continue
        gts = np.concatenate([np.arange(gt_range[g, 0], gt_range[g, 0] + gt_range[g, 1]) for g in gs])
        for mi, max_det in enumerate(max_dets):
            ds = []
            for g in gs:
                d = np.arange(det_range[g, 0], det_range[g, 0] + det_range[g, 1])
                d = d[(rank[d] >= 0) & (rank[d] < max_det)]
                ds.append(d[np.argsort(rank[d], kind="stable")])
            ds = np.concatenate(ds)
            ds = ds[np.argsort(-score[ds], kind="mergesort")]
            for a in range(A):
                npig = int((~gt_ig[gts, a]).sum())
                if npig == 0:
                    continue
                matched, ig = dt_match[ds, a, :].T >= 0, dt_ig[ds, a, :].T                  # [T, nd]
                tps = np.cumsum(matched & ~ig, axis=1).astype(np.float64)
                fps = np.cumsum(~matched & ~ig, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tps[t], fps[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, mi] = rc[-1] if nd else 0.0
                    q = np.zeros(R)
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side="left")):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, k, a, mi] = q
    return {"precision": precision, "recall": recall}


def _mean(x: np.ndarray) -> float:
    x = x[x > -1]
    return float(np.mean(x)) if x.size else -1.0


def summarize(acc: Dict[str, np.ndarray], iou_thr=IOU_THRS, max_dets: Sequence[int] = MAX_DETS,
              cats: Optional[Sequence[int]] = None) -> Dict[str, object]:
    """pycocotools' summarize of accumulate's arrays, which must come from AREA_RNG's four ranges: AP (IoU 0.5 : 0.95,
    area all, the last maxDet), AP50, AP75 (the thresholds nearest 0.5 / 0.75), AP_small / AP_medium / AP_large, AR1 /
    AR10 / AR100 (the three maxDets, area all). Every mean is over the entries > -1, and -1 if there are none.
    `cats` (the category ids, accumulate's n_cat of them) adds "per_obj": {id: {"AP", "AR100"}}."""
    pr, rc = acc["precision"], acc["recall"]
    thr = np.asarray(iou_thr, np.float64)
    t50, t75 = int(np.argmin(np.abs(thr - 0.5))), int(np.argmin(np.abs(thr - 0.75)))
    last = len(max_dets) - 1
    out: Dict[str, object] = {
        "AP": _mean(pr[:, :, :, 0, last]), "AP50": _mean(pr[t50, :, :, 0, last]), "AP75": _mean(pr[t75, :, :, 0, last]),
        "AP_small": _mean(pr[:, :, :, 1, last]), "AP_medium": _mean(pr[:, :, :, 2, last]),
        "AP_large": _mean(pr[:, :, :, 3, last])}
    for mi, m in enumerate(max_dets):
        out[f"AR{m}"] = _mean(rc[:, :, 0, mi])
    if cats is not None:
        out["per_obj"] = {int(c): {"AP": _mean(pr[:, :, k, 0, last]), f"AR{max_dets[last]}": _mean(rc[:, k, 0, last])}
                          for k, c in enumerate(cats)}
    return out
