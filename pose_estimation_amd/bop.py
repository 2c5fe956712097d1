"""The BOP-19 pose errors on the GPU: VSD, MSSD and MSPD (Hodan et al., "BOP Challenge 2020 on 6D Object
Localization", ECCV-W 2020) and the average recalls AR_VSD / AR_MSSD / AR_MSPD / AR that LineMOD and LM-O
results are published with. Written from the published definition (include/krrn_hip.h states it,
tests/bop_ref.py restates it in numpy); it has not been compared against the BOP toolkit's output. One known
departure: pixels are sampled at their integer coordinates, this project's rasteriser convention.

    e = vsd(verts, faces, face_range, R_est, t_est, R_gt, t_gt, K4, depth, frame, diameter)
    # -> {"counts": int32 [B, 2 + T] = (union, inter, step_k), "e_vsd": f64 [B, T]}
    d = mssd_mspd(verts, vert_range, R_est, t_est, R_gt, t_gt, K4, syms, sym_range)
    # -> {"mssd": f64 [B] metres, "mspd": f64 [B] pixels, "sym_idx": int32 [B, 2]}
    syms = symmetry_set(discrete=[...], continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}])   # [NS, 12]
    errs = bop_errors(pred_r, pred_t, data, dataset)      # data = dataset.batch(idx, device, bop=True)
    res = fold_bop(records, objlist, diameter, width)     # evaluate.test_epoch(..., bop=True)["bop"]
    gt = visibility(verts, faces, face_range, R, t, K4, depth, frame)   # ground-truth visibility of B instances
    # -> {"mask", "mask_visib": u8 [B, H, W], "info": int32 [B, 11] (INFO), "visib_fract": f64 [B]}

`visibility` is what BOP's calc_gt_masks / calc_gt_info scripts compute, with VSD's render and VSD's visibility
rule. Its two stated departures from those scripts: bbox_obj is clipped to the frame (BOP renders the silhouette
into a 3 x larger window), and pixels are sampled at their integer coordinates, as everywhere in this project.

fold_bop scores one estimate per target against the GT pose it was cropped from (LineMOD's eval: recall is
correct / targets). match_poses is the BOP toolkit's greedy match_poses for many targets at once: it matches a
target's estimates to its GT instances per error function and threshold (krrn_bop_match_f64), and
bop_scene.eval_results builds the protocol's recalls for a result file on it.

    m = match_poses(score, err, est_range, gt_range, pair_off, thr, n_top, n_inst)
    # -> {"match": int32 [n_inst, C, NT] (estimate index or -1), "tp": int32 [G, C, NT]}
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .runtime import h2d, ptr, stream_ptr

DELTA = 0.015                                           # metres: BOP-19's visibility tolerance
TAUS = tuple(0.05 * k for k in range(1, 11))            # VSD misalignment tolerances, fractions of the diameter
THETAS = tuple(0.05 * k for k in range(1, 11))          # correctness thresholds of VSD and (x diameter) MSSD
THETAS_PX = tuple(5.0 * k for k in range(1, 11))        # MSPD's, pixels at a 640-px-wide image
MAX_T = 16                                              # kBopMaxT of csrc/bop.hip
SYM_SPLIT = 16                                          # kBopSymSplit
FRAME_W = 640                                           # LineMOD's frames (dataset.get_square_bbox)
# per-crop record of the eval epoch's BOP table (f64), beside evaluate.REC
BOP_REC = ("crop", "cls") + tuple(f"vsd_{k}" for k in range(len(TAUS))) + ("mssd", "mspd", "valid")
_B = {k: i for i, k in enumerate(BOP_REC)}


def _poses(dev, B, R_est, t_est, R_gt, t_gt):
    """The four pose operands as f64 [B, 9] / [B, 3] on `dev` (converted there: no host round trip)."""
    return [h2d(x, dev, torch.float64).reshape(B, w).contiguous()
            for x, w in ((R_est, 9), (t_est, 3), (R_gt, 9), (t_gt, 3))]


class Scene(NamedTuple):
    """stage_scene's result: the operands every render-versus-depth entry point takes, as the kernels read them."""
    v: torch.Tensor                 # verts f32 [Vtot, 3]
    f: torch.Tensor                 # faces int32 [Ftot, 3]
    d: torch.Tensor                 # depth f32 [F, H, W]
    m: Optional[torch.Tensor]       # mask u8 [F, H, W], or None
    fr: torch.Tensor                # face_range int32 [B, 2]
    K: torch.Tensor                 # K4 f32 [B, 4]
    fi: torch.Tensor                # frame int32 [B]
    B: int
    F: int
    H: int
    W: int


def stage_scene(name: str, verts, faces, face_range, K4, depth, frame, *mask) -> Scene:
    """What vsd, visibility, verify.score_poses and depth_refine.refine share: verts / faces / depth (and the optional
    u8 mask of depth's shape, for the callers that pass one) must be GPU tensors (RuntimeError naming `name`), depth
    [F, H, W] (ValueError); they are converted to the kernels' types, and face_range [B, 2], K4 [B, 4] and frame [B]
    are staged on verts' device. The caller keeps the returned Scene bound until its launch is enqueued
    (metric.add_metric's rule): a converted operand that nothing holds would be freed under the kernel."""
    m = mask[0] if mask else None
    if not (verts.is_cuda and faces.is_cuda and depth.is_cuda and (m is None or m.is_cuda)):
        raise RuntimeError(f"{name} runs on the HIP path only (verts / faces / depth{' / mask' if mask else ''} must be "
                           "GPU tensors)")
    dev = verts.device
    B = int(face_range.reshape(-1, 2).shape[0])
    if depth.dim() != 3:
        raise ValueError(f"depth must be [F, H, W], got {tuple(depth.shape)}")
    if m is not None and (m.dtype != torch.uint8 or tuple(m.shape) != tuple(depth.shape)):
        raise ValueError(f"mask must be uint8 {tuple(depth.shape)}, got {m.dtype} {tuple(m.shape)}")
    return Scene(verts.to(torch.float32).contiguous(), faces.to(torch.int32).contiguous(),
                 depth.to(torch.float32).contiguous(), m.contiguous() if m is not None else None,
                 h2d(face_range.reshape(B, 2), dev, torch.int32), h2d(K4.reshape(B, 4), dev, torch.float32),
                 h2d(frame.reshape(B), dev, torch.int32), B, *(int(x) for x in depth.shape))


def per_crop(x: Union[float, torch.Tensor], B: int, device, name: str) -> torch.Tensor:
    """A float or a [B] tensor (host or GPU) as f64 [B] on `device`."""
    if isinstance(x, torch.Tensor):
        if x.numel() != B:
            raise ValueError(f"{name} must be a float or a [B] tensor with B = {B}, got {tuple(x.shape)}")
        return h2d(x.reshape(B), device, torch.float64)
    return h2d(torch.full((B,), float(x), dtype=torch.float64), device)


def vsd(verts: torch.Tensor, faces: torch.Tensor, face_range: torch.Tensor, R_est: torch.Tensor, t_est: torch.Tensor,
        R_gt: torch.Tensor, t_gt: torch.Tensor, K4: torch.Tensor, depth: torch.Tensor, frame: torch.Tensor,
        diameter: torch.Tensor, depth_scale: float = 1.0, delta: float = DELTA,
        taus: Sequence[float] = TAUS) -> Dict[str, torch.Tensor]:
    """krrn_bop_vsd_f32 for B crops (module doc). verts [Vtot, 3] / faces [Ftot, 3] / depth [F, H, W] are GPU
    tensors; face_range [B, 2], the poses, K4 [B, 4], frame [B] and diameter [B] (metres) may be host tensors
    (staged here). Nothing is read back: the poses may come straight from a solver's launch."""
    s = stage_scene("vsd", verts, faces, face_range, K4, depth, frame)
    dev, B, T = verts.device, s.B, len(taus)
    if not 1 <= T <= MAX_T:
        raise ValueError(f"1 .. {MAX_T} taus, got {T}")
    Re, te, Rg, tg = _poses(dev, B, R_est, t_est, R_gt, t_gt)
    dia = h2d(diameter.reshape(B), dev, torch.float64)
    tau = h2d(torch.tensor(list(taus), dtype=torch.float64), dev)
    ws = torch.empty((B, 8), dtype=torch.int32, device=dev)       # krrn_bop_vsd_ws(B)
    counts = torch.empty((B, 2 + T), dtype=torch.int32, device=dev)
    e = torch.empty((B, T), dtype=torch.float64, device=dev)
    _lib.call("krrn_bop_vsd_f32", ptr(s.v), s.v.shape[0], ptr(s.f), s.f.shape[0], ptr(s.fr), ptr(Re), ptr(te), ptr(Rg),
              ptr(tg), ptr(s.K), ptr(s.d), s.F, s.H, s.W, ptr(s.fi), float(depth_scale), ptr(dia), float(delta), ptr(tau),
              T, B, ptr(ws), ptr(counts), ptr(e), stream_ptr(dev))
    return {"counts": counts, "e_vsd": e}


VISIB_WS = 16                                           # kVisWs of csrc/bop.hip: ints per instance
INFO = ("px_count_all", "px_count_valid", "px_count_visib", "bbox_obj_x", "bbox_obj_y", "bbox_obj_w", "bbox_obj_h",
        "bbox_visib_x", "bbox_visib_y", "bbox_visib_w", "bbox_visib_h")


def visibility(verts: torch.Tensor, faces: torch.Tensor, face_range: torch.Tensor, R: torch.Tensor, t: torch.Tensor,
               K4: torch.Tensor, depth: torch.Tensor, frame: torch.Tensor, depth_scale: float = 1.0,
               delta: float = DELTA, masks: bool = True) -> Dict[str, torch.Tensor]:
    """krrn_bop_visib_u8 for B instances (include/krrn_hip.h): the ground truth that BOP's calc_gt_masks /
    calc_gt_info scripts compute, from VSD's render and VSD's visibility rule. Operands and staging as `vsd`, one
    pose (R [B, 3, 3], t [B, 3]) per instance. Returns {"mask", "mask_visib": u8 [B, H, W] of 0 / 1 (absent with
    masks=False), "info": int32 [B, 11] in the order of INFO, "visib_fract": f64 [B]}; a box is (x, y, w, h) with
    BOP's w = x_max - x_min, h = y_max - y_min, or four -1 without a pixel. Two stated departures from BOP's
    scripts: bbox_obj is clipped to the frame (BOP renders the silhouette into a 3 x larger window), and pixels
    are sampled at their integer coordinates. Nothing is read back."""
    s = stage_scene("visibility", verts, faces, face_range, K4, depth, frame)
    dev, B, H, W = verts.device, s.B, s.H, s.W
    Rd = h2d(R, dev, torch.float64).reshape(B, 9).contiguous()
    td = h2d(t, dev, torch.float64).reshape(B, 3).contiguous()
    ws = torch.empty((B, VISIB_WS), dtype=torch.int32, device=dev)    # krrn_bop_visib_ws(B)
    out = {}
    if masks:
        out["mask"] = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        out["mask_visib"] = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    out["info"] = torch.empty((B, 11), dtype=torch.int32, device=dev)
    out["visib_fract"] = torch.empty((B,), dtype=torch.float64, device=dev)
    _lib.call("krrn_bop_visib_u8", ptr(s.v), s.v.shape[0], ptr(s.f), s.f.shape[0], ptr(s.fr), ptr(Rd), ptr(td), ptr(s.K),
              ptr(s.d), s.F, H, W, ptr(s.fi), float(depth_scale), float(delta), B, ptr(ws), ptr(out.get("mask")),
              ptr(out.get("mask_visib")), ptr(out["info"]), ptr(out["visib_fract"]), stream_ptr(dev))
    return out


def mssd_mspd(verts: torch.Tensor, vert_range: torch.Tensor, R_est: torch.Tensor, t_est: torch.Tensor,
              R_gt: torch.Tensor, t_gt: torch.Tensor, K4: torch.Tensor, syms: torch.Tensor,
              sym_range: torch.Tensor) -> Dict[str, torch.Tensor]:
    """krrn_bop_mssd_mspd_f32 for B crops (module doc). verts [Vtot, 3] is a GPU tensor; syms [NStot, 12]
    (symmetry_set rows, concatenated over objects), the ranges [B, 2], the poses and K4 may be host tensors."""
    if not verts.is_cuda:
        raise RuntimeError("mssd_mspd runs on the HIP path only (verts must be a GPU tensor)")
    dev = verts.device
    B = int(vert_range.reshape(-1, 2).shape[0])
    v = verts.to(torch.float32).contiguous()
    vr = h2d(vert_range.reshape(B, 2), dev, torch.int32)
    sr = h2d(sym_range.reshape(B, 2), dev, torch.int32)
    sy = h2d(syms.reshape(-1, 12), dev, torch.float64)
    Re, te, Rg, tg = _poses(dev, B, R_est, t_est, R_gt, t_gt)
    K = h2d(K4.reshape(B, 4), dev, torch.float32)
    out = {"mssd": torch.empty((B,), dtype=torch.float64, device=dev),
           "mspd": torch.empty((B,), dtype=torch.float64, device=dev),
           "sym_idx": torch.empty((B, 2), dtype=torch.int32, device=dev)}
    ws = torch.empty((3 * B * SYM_SPLIT,), dtype=torch.float64, device=dev)   # krrn_bop_mssd_mspd_ws(B)
    _lib.call("krrn_bop_mssd_mspd_f32", ptr(v), v.shape[0], ptr(vr), ptr(Re), ptr(te), ptr(Rg), ptr(tg), ptr(K), ptr(sy),
              sy.shape[0], ptr(sr), B, ptr(ws), ptr(out["mssd"]), ptr(out["mspd"]), ptr(out["sym_idx"]),
              stream_ptr(dev))
    return out


MATCH_MAX = 128                                         # kMatchMax of csrc/krrn_match.h: rows per side of a group (coco's too)
MAX_NT = 16                                             # kMatchMaxNT: thresholds of correctness per error function


def match_poses(score: torch.Tensor, err: torch.Tensor, est_range: torch.Tensor, gt_range: torch.Tensor,
                pair_off: torch.Tensor, thr: torch.Tensor, n_top: torch.Tensor, n_inst: int, device=None,
                max_est: int = MATCH_MAX, max_gt: int = MATCH_MAX) -> Dict[str, torch.Tensor]:
    """krrn_bop_match_f64 for G groups (include/krrn_hip.h states the matching): score [Etot], err [Ptot, C],
    est_range / gt_range [G, 2], pair_off [G], thr [G, C, NT] and n_top [G] may be host or GPU tensors (staged
    here); n_inst = the length of the instance axis. `device` is needed only when every operand is a host tensor.
    max_est / max_gt are the limits that the caller states for the ranges (they are device memory to the entry
    point); a group that breaks them is matched as one without estimates. Returns {"match": int32 [n_inst, C, NT]
    (the matched estimate's index into score, or -1), "tp": int32 [G, C, NT]} on the device. Nothing is read back.
    ValueError: more than 2^31 - 1 pair rows, or shapes that do not fit together."""
    if device is None:
        device = next((x.device for x in (err, score, thr) if x.is_cuda), None)
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("match_poses runs on the HIP path only (a GPU tensor or device= is needed)")
    dev = torch.device(device)
    if err.dim() != 2 or thr.dim() != 3 or thr.shape[1] != err.shape[1]:
        raise ValueError(f"err must be [Ptot, C] and thr [G, C, NT], got {tuple(err.shape)} and {tuple(thr.shape)}")
    P, C = int(err.shape[0]), int(err.shape[1])
    G, NT = int(thr.shape[0]), int(thr.shape[2])
    if P > 2 ** 31 - 1:
        raise ValueError(f"{P} pair rows do not fit int32: match fewer groups per call")
    if not (est_range.numel() == 2 * G and gt_range.numel() == 2 * G and pair_off.numel() == G and n_top.numel() == G):
        raise ValueError(f"est_range / gt_range must be [{G}, 2] and pair_off / n_top [{G}]")
    sc = h2d(score.reshape(-1), dev, torch.float64)
    er = h2d(err, dev, torch.float64)
    e_r = h2d(est_range.reshape(G, 2), dev, torch.int32)
    g_r = h2d(gt_range.reshape(G, 2), dev, torch.int32)
    po = h2d(pair_off.reshape(G), dev, torch.int32)
    th = h2d(thr, dev, torch.float64)
    nt = h2d(n_top.reshape(G), dev, torch.int32)
    out = {"match": torch.empty((int(n_inst), C, NT), dtype=torch.int32, device=dev),
           "tp": torch.empty((G, C, NT), dtype=torch.int32, device=dev)}
    _lib.call("krrn_bop_match_f64", ptr(sc), sc.shape[0], ptr(er), P, C, ptr(e_r), ptr(g_r), ptr(po), ptr(th), NT,
              ptr(nt), G, int(n_inst), int(max_est), int(max_gt), ptr(out["match"]), ptr(out["tp"]), stream_ptr(dev))
    return out


def _axis_rotation(axis, angle: float) -> np.ndarray:
    a = np.asarray(axis, np.float64).reshape(3)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * (Kx @ Kx)   # Rodrigues


def symmetry_set(discrete=None, continuous=None, diameter_m: Optional[float] = None,
                 max_step: float = 0.01) -> np.ndarray:
    """The symmetry transformations of one object, f64 [NS, 12] = row-major R then t in metres, identity
    first, without duplicates. Inputs in BOP's models_info convention: `discrete` a list of 4 x 4 row-major
    matrices (16 numbers each, or [4, 4]) with translations in mm; `continuous` a list of {"axis": [3],
    "offset": [3] in mm}. Each continuous axis contributes ceil(pi / max_step) equal rotation steps about
    `axis` through `offset` (the first is the identity), combined with every discrete symmetry. max_step is
    the fraction of the object's diameter that the point farthest from the axis (at most diameter / 2 away)
    may travel per step, so the count does not depend on the diameter itself: diameter_m is accepted for the
    models_info call shape and not used."""
    eye = np.eye(4)
    disc = [eye]
    for m in (discrete or []):
        T = np.asarray(m, np.float64).reshape(4, 4).copy()
        T[:3, 3] /= 1000.0
        disc.append(T)
    cont = [eye]
    for c in (continuous or []):
        off = np.asarray(c.get("offset", (0.0, 0.0, 0.0)), np.float64).reshape(3) / 1000.0
        n = int(math.ceil(math.pi / max_step))
        steps = []
        for base in cont:                                   # several axes: every combination
            for i in range(n):
                T = np.eye(4)
                T[:3, :3] = _axis_rotation(c["axis"], 2.0 * math.pi * i / n)
                T[:3, 3] = off - T[:3, :3] @ off
                steps.append(T @ base)
        cont = steps
    out = []
    for d in disc:
        for c in cont:
            T = c @ d
            if not any(np.abs(T - o).max() < 1e-9 for o in out):
                out.append(T)
    return np.stack([np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]) for T in out])


def bop_errors(pred_r: torch.Tensor, pred_t: torch.Tensor, data: Dict[str, torch.Tensor], dataset,
               delta: float = DELTA, taus: Sequence[float] = TAUS) -> Dict[str, torch.Tensor]:
    """The three errors of one batch's estimates (pred_r [B, 3, 3], pred_t [B, 3], GPU) against its GT poses,
    as device tensors: {"vsd": f64 [B, T], "mssd": f64 [B] metres, "mspd": f64 [B] pixels}. `data` is
    dataset.batch(indices, device, bop=True): it carries the observed depth frames, each crop's frame index
    and its object's face / vertex / symmetry ranges; the meshes and symmetry sets are the dataset's, resident
    on the device. Queued on the current stream, nothing is read back."""
    if "bop_depth" not in data:
        raise ValueError("bop_errors needs a batch made with dataset.batch(indices, device, bop=True)")
    dev = pred_t.device
    if dev.type != "cuda":
        raise RuntimeError("bop_errors runs on the HIP path only (GPU tensors)")
    mesh = dataset._mesh_for(dev)
    B = pred_t.shape[0]
    dia = h2d(torch.tensor(dataset.diameter, dtype=torch.float64), dev)[h2d(data["cls_id"].reshape(B), dev)]
    Rg, tg = data["target_r"], data["target_t"]
    v = vsd(mesh["verts"], mesh["faces"], data["bop_face_range"], pred_r, pred_t, Rg, tg, data["intrinsic"],
            data["bop_depth"], data["bop_frame"], dia, 1.0, delta, taus)
    m = mssd_mspd(mesh["verts"], data["bop_vert_range"], pred_r, pred_t, Rg, tg, data["intrinsic"], mesh["syms"],
                  data["bop_sym_range"])
    return {"vsd": v["e_vsd"], "mssd": m["mssd"], "mspd": m["mspd"]}


def _recalls(rec: np.ndarray, dia: np.ndarray, width: float, missed: Optional[int] = None) -> Dict[str, float]:
    """missed: None (recall over the estimates), or the number of targets without an estimate, added to every
    recall's denominator and reported as "targets" = count + missed."""
    count = len(rec)
    n = count + (missed or 0)
    extra = {} if missed is None else {"targets": int(n)}
    if n == 0 or count == 0:
        return {"AR_VSD": 0.0, "AR_MSSD": 0.0, "AR_MSPD": 0.0, "AR": 0.0, "count": int(count), **extra}
    T = len(TAUS)
    e = rec[:, _B["vsd_0"]:_B["vsd_0"] + T]
    th = np.asarray(THETAS)
    ar_vsd = float(np.mean([(e < t).sum() / (n * T) for t in th]))             # 10 taus x 10 thresholds
    ar_mssd = float(np.mean([(rec[:, _B["mssd"]] < t * dia).sum() / n for t in th]))
    ar_mspd = float(np.mean([(rec[:, _B["mspd"]] < t * (width / 640.0)).sum() / n for t in THETAS_PX]))
    return {"AR_VSD": ar_vsd, "AR_MSSD": ar_mssd, "AR_MSPD": ar_mspd, "AR": (ar_vsd + ar_mssd + ar_mspd) / 3.0,
            "count": int(count), **extra}


def recalls_from_tp(tp: np.ndarray, targets: int, count: int) -> Dict[str, float]:
    """_recalls' six keys (with "targets") from matched-instance counts instead of records: tp integer [T + 2, NT] =
    the instances matched per error function (T VSD taus, MSSD, MSPD) and threshold of correctness, summed over the
    targets (bop_scene.eval_results). The averages are taken in _recalls' order, so that one estimate per target
    gives the same floats."""
    n, T = int(targets), tp.shape[0] - 2
    if n == 0 or count == 0:
        return {"AR_VSD": 0.0, "AR_MSSD": 0.0, "AR_MSPD": 0.0, "AR": 0.0, "count": int(count), "targets": n}
    ar_vsd = float(np.mean([tp[:T, k].sum() / (n * T) for k in range(tp.shape[1])]))
    ar_mssd = float(np.mean([tp[T, k] / n for k in range(tp.shape[1])]))
    ar_mspd = float(np.mean([tp[T + 1, k] / n for k in range(tp.shape[1])]))
    return {"AR_VSD": ar_vsd, "AR_MSSD": ar_mssd, "AR_MSPD": ar_mspd, "AR": (ar_vsd + ar_mssd + ar_mspd) / 3.0,
            "count": int(count), "targets": n}


def valid_by_crop(table) -> np.ndarray:
    """A (gathered) epoch table's rows without the pad rows, which evaluate.gather_epoch_records marks by a last column
    `valid` = 0, stably sorted by their first column `crop`: global crop order, however the crops were batched or
    sharded."""
    tab = table.numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    tab = tab[tab[:, -1] > 0]
    return tab[np.argsort(tab[:, 0], kind="stable")]


def fold_bop(records, objlist: Sequence[int], diameter: Sequence[float], width: float = FRAME_W,
             missed: Optional[Dict[int, int]] = None) -> Dict[str, object]:
    """The BOP-19 average recalls over per-crop BOP_REC records (any order, pad rows valid = 0), folded in
    global crop order like evaluate.fold_records. An estimate is correct w.r.t. an error when the error is
    strictly below the threshold; recall = correct / targets (one estimate per target).
      AR_VSD   mean over the 10 taus x 10 thresholds 0.05 .. 0.5 of the share of crops with e_vsd < threshold
      AR_MSSD  mean over thresholds 0.05 .. 0.5 x the object's diameter
      AR_MSPD  mean over thresholds 5 .. 50 px x (width / 640)
      AR       the mean of the three
    Returns {"AR_VSD", "AR_MSSD", "AR_MSPD", "AR", "count"} over all crops pooled, plus "per_obj": {obj id:
    the same five keys} for the objects that occur.
    missed: None, or {obj id: count} of targets that have no estimate (a detector missed them). They are added to
    every recall's denominator, per object and pooled: "count" stays the number of estimates and a sixth key
    "targets" = count + missed appears beside it; an object with missed targets only occurs in per_obj with recall
    0. With missed=None nothing changes."""
    rec = records.numpy() if isinstance(records, torch.Tensor) else np.asarray(records, np.float64)
    rec = valid_by_crop(rec.reshape(-1, len(BOP_REC)))
    cls = rec[:, _B["cls"]].astype(np.int64)
    dia = np.asarray(diameter, np.float64)[cls] if len(rec) else np.zeros((0,))
    if missed is None:
        out = _recalls(rec, dia, float(width))
        out["per_obj"] = {objlist[int(c)]: _recalls(rec[cls == c], dia[cls == c], float(width))
                          for c in dict.fromkeys(cls.tolist())}
        return out
    miss = {int(o): int(m) for o, m in missed.items() if int(m) > 0}
    out = _recalls(rec, dia, float(width), sum(miss.values()))
    objs = [objlist[int(c)] for c in dict.fromkeys(cls.tolist())]
    objs += [o for o in sorted(miss) if o not in objs]
    out["per_obj"] = {}
    for o in objs:
        sel = cls == (list(objlist).index(o) if o in objlist else -1)
        out["per_obj"][o] = _recalls(rec[sel], dia[sel], float(width), miss.get(o, 0))
    return out
