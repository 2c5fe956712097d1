"""Batched, sharded eval epoch: Trainer.test_epoch
(tools/trainer.py:145-250) over size-bucketed batches instead of one crop per step, split across
ranks.

Per batch of equal-size crops (BucketBatcher): the GPU-built inputs (PoseDataset.batch), one
KRRN forward, the eval-time KRRNLoss map terms per crop when the batch carries GT maps (a
PoseDataset(root, gt_maps=True) renders them from the tree's meshes on the input stream;
krrn_map_losses_crop_f32: the reference's batch-size-1 loop adds each crop's own losses,
trainer.py:180-182), get_pose (PnP-RANSAC, the "base" R / t), the TBase translation (the "reg" /
"final" t) and ADD(-S) / rotation / translation errors for the whole batch in one launch
(metric.cal_dis_batch). Each crop leaves one f64 record (REC fields below).

Multi-GPU (one process per GPU): every rank evaluates its own contiguous slice of every S bucket
(distributed.bucket_shard), the per-crop records are all-gathered (RCCL all_gather_into_tensor;
every rank knows every shard's size from the crop sizes, so records are padded to the largest
shard, no size exchange), and every rank folds them in global crop order — so the result dict,
sums included, is bit-identical for any world size. One all_reduce of the success counts checks
the gathered table against the ranks' own tallies.

The per-object bookkeeping keeps the reference's result keys and thresholds (ADD(-S) < 0.1 d,
5 deg, 5 cm); test_dis sums final ADD(-S) with opt_pose and base ADD(-S) without (:232-247);
the ADD(-S) AUC of Metric.cal_auc (metric.py:38-65) is reported per object and overall.
"""
from __future__ import annotations

import copy
from collections import namedtuple
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import distributed as kd
from .bop import BOP_REC, FRAME_W, TAUS, bop_errors, fold_bop, valid_by_crop
from . import rle
from .bop_scene import (_require, eval_coco, eval_results, net_mask_rows, vis_results, write_detections,
                        write_result_masks, write_results)
from .dataset import ZOOM_KEYS, PoseDataset
from .krrn import KRRN
from .loss import map_losses
from .metric import Metric, add_metric, rt_errors
from .pose import get_pose, get_pose_umeyama, refine_pose_depth, refine_pose_icp, select_pose

ROT_THR_DEG = 5.0     # trainer.py:156
TRANS_THR_M = 0.05    # trainer.py:157
_KEYS = ("all_num", "obj_num", "succ_base_rt", "dis_base_rt", "succ_base_r", "dis_base_r", "succ_base_t",
         "dis_base_t", "succ_reg_rt", "dis_reg_rt", "succ_reg_r", "dis_reg_r", "succ_reg_t", "dis_reg_t",
         "succ_final_rt", "dis_final_rt", "succ_final_r", "dis_final_r", "succ_final_t", "dis_final_t",
         "dis_mask", "dis_normal", "dis_xyz")
# per-crop record (f64)
REC = ("crop", "cls", "add_b", "r_b", "t_b", "add_f", "r_f", "t_f", "l_xyz", "l_mask", "l_normal", "valid")
_R = {k: i for i, k in enumerate(REC)}
# per-crop record of eval_records(poses=True) (f64): the scored pose, R row-major, t in metres
POSE_REC = ("crop",) + tuple(f"r{k}" for k in range(9)) + ("tx", "ty", "tz")
# per-crop record of eval_records(select="depth") (f64): the candidate that pose.select_pose kept, its score and the
# two counts the score is made of
SEL_REC = ("crop", "cand", "score", "inter", "union", "valid")
# what one evaluated batch leaves on the device until the epoch's single read-back (idx: its crop indices, on
# the host; score_r / score_t: the pose test_dis scores, i.e. the final pose (fin_r, pred_t) with opt_pose and the base
# pose without; add_f is None without opt_pose, lc without GT maps)
_Batch = namedtuple("_Batch", "idx cls_id target_r target_t base_r base_t score_r score_t add_b add_f lc")


class EpochTables(NamedTuple):
    """The per-crop tables of one eval epoch, f64 with one row per crop in the order evaluated, or None for a table
    that was not asked for: rec [n, len(REC)], bop [n, len(BOP_REC)], poses [n, len(POSE_REC)], sel [n, len(SEL_REC)]."""
    rec: Optional[torch.Tensor] = None
    bop: Optional[torch.Tensor] = None
    poses: Optional[torch.Tensor] = None
    sel: Optional[torch.Tensor] = None

    def legacy(self):
        """eval_records' documented return: the tables that are set, in the order rec, bop, poses, sel, as a tuple;
        rec alone as the lone tensor."""
        tabs = tuple(t for t in self if t is not None)
        return tabs if len(tabs) > 1 else tabs[0]

    @classmethod
    def of(cls, ret, bop: bool, poses: bool, select: bool) -> "EpochTables":
        """The bundle back from legacy()'s value, given which tables were asked for."""
        tabs = iter(ret if isinstance(ret, tuple) else (ret,))
        return cls(*(next(tabs) if on else None for on in (True, bop, poses, select)))


def _check_zoom(zoom, dataset) -> None:
    """eval_records' / test_epoch's `zoom`: a number of passes, on a dataset whose input path takes any window."""
    if isinstance(zoom, bool) or not isinstance(zoom, (int, np.integer)) or zoom < 0:
        raise ValueError(f"zoom is the number of extra passes, an integer >= 0, got {zoom!r}")
    if zoom > 0 and getattr(dataset, "resize", None) is None:
        raise ValueError("zoom needs a dataset built with resize")


def _batches(buckets: Dict[int, List[int]], bs: int):
    for S in sorted(buckets):
        idx = buckets[S]
        for lo in range(0, len(idx), bs):
            yield S, idx[lo:lo + bs]


def eval_records(model: KRRN, dataset: PoseDataset, indices: Dict[int, List[int]], bs: int, device,
                 opt_pose: bool = True, with_loss: bool = True, pose_solver: str = "pnp",
                 refine: Optional[str] = None, bop: bool = False, poses: bool = False,
                 select: Optional[str] = None, net_masks: bool = False, zoom: int = 0):
    """Run the eval path over {S: [crop indices]} in batches of <= bs; returns f64 [n, len(REC)]
    (rows in the order evaluated). Every batch's inputs, forward, pose and ADD(-S) are queued on
    the device without a host round trip; the per-crop records are read back once at the end (the
    same numbers as a per-batch read-back, without a stall per batch).

    Three streams: batch j+1's inputs are built on one side stream while batch j's forward runs on
    the caller's stream (fresh tensors from resident frames), and batch j's PnP-RANSAC + ADD(-S)
    run on another beside batch j+1's forward (one workgroup per crop: latency-bound launches that
    fill the CUs the forward leaves idle). The pose reads a copy of the forward's 3-channel xyz map
    (the plan's buffer is rewritten by the next forward of the same shape). Host draws keep the
    serial order: forward j's pool perms, then get_pose j's point subsets, then forward j+1's.

    pose_solver: "pnp" (get_pose, the reference's test loop) or "umeyama" (get_pose_umeyama: the base
    R / t from the depth-based Umeyama-RANSAC of tools/script/eval.py:151; everything else unchanged).

    refine: None (the reference's loop), or "icp": the base pose (base_r, base_t) and, with opt_pose, the
    final pose (base_r, pred_t) are each polished by pose.refine_pose_icp against the crop's cloud on the
    pose stream before their ADD(-S) and rotation / translation errors (two more launches per batch; the
    final pose then carries its own refined R). max_dist = icp.DIST_FRAC x the object's diameter. "depth" polishes
    the same two poses by pose.refine_pose_depth instead: render-based point-to-plane refinement against the observed
    depth frame (include/krrn_hip.h: krrn_pose_refine_depth_f32), with max_dist = depth_refine.DIST_FRAC x the
    diameter and the twist's radius = diameter / 2. It needs a dataset with meshes (ValueError otherwise) and builds
    its batches with verify=True.

    bop: also the BOP-19 errors (bop.bop_errors: VSD, MSSD, MSPD) of the final pose, i.e. (fin_r, pred_t) with
    opt_pose and the base pose without, as test_dis chooses; queued on the pose stream after add_metric and
    read back with everything else at the end. Needs a dataset with meshes. The return value is then the pair
    (records, f64 [n, len(bop.BOP_REC)] in the same row order); every number of `records` is unchanged.

    poses: also return an f64 [n, len(POSE_REC)] table in the same row order: crop, R row-major and t in metres of
    the pose that test_dis scores (the final pose with opt_pose, else the base pose). It is read back
    in the epoch's single read-back (the tensors are the ones the records are made from). The return value then
    ends with it: (records, poses) or (records, bop table, poses).

    select: None, or "depth" (needs opt_pose and a dataset with meshes; ValueError otherwise): the final pose is
    chosen per crop by pose.select_pose (render-and-compare against the observed depth and the crop's mask_label;
    include/krrn_hip.h: krrn_pose_score_f32) among, in priority order, 0 the pose test_dis scores today (fin_r,
    pred_t), the refined one with refine="icp" / "depth"; 1 the base pose; and with a refiner also 2 the unrefined
    (PnP R, raw pred_t) and 3 the unrefined base pose. The winner replaces the final pose for add_f, r_f / t_f,
    the BOP errors and the pose table; the base columns are untouched. One more launch per batch on the pose
    stream, no host round trip. The return value then ends with an f64 [n, len(SEL_REC)] table in the same row
    order, read back in the epoch's single read-back. With select=None nothing changes.

    net_masks (off by default: nothing changes; needs a dataset with layout="bop", whose frames share one size): also
    the network's own segmentation of every crop as a full-frame mask. Right after each forward, on its stream and
    so before the next forward rewrites the plan's buffer, rle.paste_masks decides every pixel of the view
    pred["mask"] for channel cls_id + 1 and places the crop's window (dataset.boxes: rows rmin .., columns cmin ..)
    into a plane of dataset.frame_hw, and rle.encode_gpu encodes the planes; chan and rc are built on the host. The
    runs are read back once the batch's pose step is queued (one read-back per batch, and one more encode for a
    batch in which a mask outgrows the encoder's default slot), so the planes live for one batch only. The return
    value then ends with a list [(crop, run list, info = the mask's five ints)] in the same row order.

    zoom (0 by default: no extra work is queued and every table is what it was, bit for bit; needs a dataset built
    with resize, ValueError otherwise, and is refused together with net_masks): the number of zoom-in passes per batch
    (DESIGN.md §3). Each takes the solver's own pose of the pass before, (base_r, pred_t) with opt_pose and (base_r,
    base_t) without, i.e. before `refine` and `select`; cuts every crop again about that pose's projection on the pose
    stream (dataset.zoom_batch: zoom.pose_windows, then dataset.build_inputs_windows; no read-back); runs the forward
    again on the caller's stream, which waits for the pose stream (the next batch's inputs are still built beside it);
    and runs the solver again. `refine`, `select`, ADD(-S), the BOP errors and the pose table read the last pass and
    its batch dict, so select_pose sees the new `bbox`. The return value then ends with an int64 [n] array in the same
    row order: the last pass's zoom status per crop (zoom.pose_windows), read back in the epoch's single read-back."""
    tabs, net, zstat = _eval_epoch(model, dataset, indices, bs, device, opt_pose, with_loss, pose_solver, refine, bop,
                                   poses, select, net_masks, zoom)
    extras = tuple(x for x in (net, zstat) if x is not None)
    if not extras:
        return tabs.legacy()
    return tuple(t for t in tabs if t is not None) + extras


@torch.no_grad()
def _eval_epoch(model, dataset, indices, bs, device, opt_pose, with_loss, pose_solver, refine, bop, poses, select,
                net_masks, zoom):
    """eval_records' epoch: (EpochTables, the net_masks run list or None, the zoom status array or None)."""
    _check_zoom(zoom, dataset)
    if zoom and net_masks:
        raise ValueError("zoom with net_masks is not built: the paste places the crop's pixels at dataset.boxes")
    if pose_solver not in ("pnp", "umeyama"):
        raise ValueError(f"pose_solver must be 'pnp' or 'umeyama', got {pose_solver!r}")
    if refine not in (None, "icp", "depth"):
        raise ValueError(f"refine must be None, 'icp' or 'depth', got {refine!r}")
    if select not in (None, "depth"):
        raise ValueError(f"select must be None or 'depth', got {select!r}")
    if select and not opt_pose:
        raise ValueError("select='depth' chooses the final pose: it needs opt_pose=True")
    if select:
        _require(dataset, "select='depth' renders the objects' meshes: it needs a dataset with meshes=True", meshes=True)
    if refine == "depth":
        _require(dataset, "refine='depth' renders the objects' meshes: it needs a dataset with meshes=True", meshes=True)
    if net_masks:
        _require(dataset, "net_masks pastes into a BOP tree's frames: it needs a PoseDataset with layout='bop'", layout=True)
    solve_pose = get_pose if pose_solver == "pnp" else get_pose_umeyama
    metric = Metric(dataset.sym_obj)
    pending = []
    bop_pending = []   # per batch, with bop: bop_errors' dict of device tensors
    sel_pending = []   # per batch, with select: select_pose's dict of device tensors
    net = []           # with net_masks: (crop, run list, info) per crop
    zoom_pending = []  # per batch, with zoom: the last pass's zoom_status, on the device
    bkw = {"zoom": True} if zoom else {}
    batches = list(_batches(indices, bs))
    device = torch.device(device)
    dia = torch.tensor(dataset.diameter, dtype=torch.float32).to(device) if refine else None  # [classes], metres
    main = torch.cuda.current_stream(device)
    side = torch.cuda.Stream(device)   # inputs
    pstr = torch.cuda.Stream(device)   # pose + metric

    def build(j):
        side.wait_stream(main)  # the inputs' pinned staging and allocations follow earlier work
        with torch.cuda.stream(side):
            if select or refine == "depth":
                d = dataset.batch(batches[j][1], device, verify=True, **bkw)
            else:
                d = (dataset.batch(batches[j][1], device, bop=True, **bkw) if bop else
                     dataset.batch(batches[j][1], device, **bkw))
            ev = torch.cuda.Event()
            ev.record(side)
        return d, ev

    def solve(pred, data, B):
        """Clone what the pose step reads from the plan's output buffers (the next forward of the same shape rewrites
        them), hand the copies over to the pose stream and solve there: (base_r, base_t, pred_t)."""
        xyz = pred["xyz"].clone()
        pred_t = pred["pred_t"].reshape(B, 3).clone() if opt_pose else None
        done = torch.cuda.Event()
        done.record(main)
        pstr.wait_event(done)
        xyz.record_stream(pstr)
        if pred_t is not None:
            pred_t.record_stream(pstr)
        with torch.cuda.stream(pstr):
            base_r, base_t = solve_pose({"xyz": xyz}, data)
        return base_r, base_t, pred_t

    nxt = build(0) if batches else None
    views = model.return_views
    model.return_views = True
    try:
        for j, (S, idx) in enumerate(batches):
            data, ev = nxt
            main.wait_event(ev)
            for v in data.values():
                if zoom and not v.is_cuda:  # zoom_depth_scale, a host scalar
                    continue
                v.record_stream(main)
                v.record_stream(pstr)
            if j + 1 < len(batches):
                nxt = build(j + 1)
            pred = model(data["img_croped"], data["cloud"], data["choose"], data["cls_id"], opt_pose=opt_pose)
            B = len(idx)
            pasted = enc = None
            if net_masks:  # pred["mask"] is a view of the plan's buffer: read here, on the forward's stream
                pasted = rle.paste_masks(pred["mask"], [dataset.objlist.index(dataset._meta(i)[0]) + 1 for i in idx],
                                         [[dataset.boxes[i][0], dataset.boxes[i][2]] for i in idx], *dataset.frame_hw)
                enc = rle.encode_gpu(pasted["mask"])
            lc = None
            if with_loss and "xyz" in data and "multi_cls_mask" in data:
                lc = map_losses(pred, data, per_crop=True)  # [B, 8]: xyz, normal, region, mask, counts
            base_r, base_t, pred_t = solve(pred, data, B)
            for _ in range(zoom):
                # cut again about the solver's own pose (pose stream), forward again (caller's stream, after the pose
                # stream), solve again (pose stream); the side stream goes on building the next batch's inputs
                with torch.cuda.stream(pstr):
                    data = dataset.zoom_batch(data, base_r, pred_t if opt_pose else base_t.reshape(B, 3))
                    cut = torch.cuda.Event()
                    cut.record(pstr)
                main.wait_event(cut)
                for k in ZOOM_KEYS:  # made on the pose stream, read by the forward on the caller's
                    data[k].record_stream(main)
                pred = model(data["img_croped"], data["cloud"], data["choose"], data["cls_id"], opt_pose=opt_pose)
                base_r, base_t, pred_t = solve(pred, data, B)
            if zoom:
                zoom_pending.append(data["zoom_status"])
            with torch.cuda.stream(pstr):
                fin_r = base_r
                r0, t0, raw_t = base_r, base_t, pred_t  # the solver's and TBase's own, before any refinement
                if refine:
                    d = dia[data["cls_id"].reshape(B)]
                    polish = ((lambda r, t: refine_pose_icp(r, t, data, diameter=d)) if refine == "icp" else
                              (lambda r, t: refine_pose_depth(r, t, data, dataset, d)))
                    base_r, base_t = polish(r0, base_t.reshape(B, 3))
                    if opt_pose:
                        fin_r, pred_t = polish(r0, pred_t)
                add_b = add_metric(base_r, base_t.reshape(B, 3), data["model_points"], data["target"],
                                   data["cls_id"], metric.sys)
                if select:
                    cands = [(fin_r, pred_t), (base_r, base_t.reshape(B, 3))]
                    if refine:
                        cands += [(r0, raw_t), (r0, t0.reshape(B, 3))]
                    sel = select_pose(cands, data, dataset)
                    fin_r, pred_t = sel["R"], sel["t"]
                    sel_pending.append(sel)
                # the pose test_dis scores, chosen here once: the final pose, or the base pose without opt_pose
                score_r, score_t = (fin_r, pred_t) if opt_pose else (base_r, base_t.reshape(B, 3))
                add_f = None
                if opt_pose:
                    # reg = final = (PnP R, TBase t) (trainer.py:198-201)
                    add_f = add_metric(fin_r, pred_t, data["model_points"], data["target"], data["cls_id"],
                                       metric.sys)
                if bop:
                    bop_pending.append(bop_errors(score_r, score_t, data, dataset))
            pending.append(_Batch(idx, data["cls_id"], data["target_r"], data["target_t"], base_r, base_t, score_r,
                                  score_t, add_b, add_f, lc))
            if net_masks:  # the host waits for this forward only now, with the pose step and the next inputs queued
                runs, info = rle.runs_of(pasted["mask"], enc), pasted["info"].cpu().numpy()
                net += [(int(i), runs[k], [int(v) for v in info[k]]) for k, i in enumerate(idx)]
    finally:
        model.return_views = views
    main.wait_stream(pstr)
    for p in pending:  # made on the pose stream, read back on the caller's
        for t in (p.base_r, p.base_t, p.add_b, p.add_f) + ((p.score_t, p.score_r) if refine or select else ()):
            if t is not None:
                t.record_stream(main)
    for e in bop_pending + sel_pending:
        for t in e.values():
            t.record_stream(main)
    for t in zoom_pending:
        t.record_stream(main)
    # one read-back and one vectorised host pass for the whole epoch: per batch, the rotation /
    # translation errors' six small copies and ~60 CPU ops ran after the GPU had drained (a serial
    # host tail of ~1 ms per batch); every quantity is per crop, so the values are the same
    n = sum(len(p.idx) for p in pending)
    rec, brec, prec, srec = (np.zeros((n, len(cols)), dtype=np.float64) if on else None for on, cols in
                             ((True, REC), (bop, BOP_REC), (poses, POSE_REC), (select, SEL_REC)))
    if pending:
        cat = lambda k, w: torch.cat([getattr(p, k).reshape(len(p.idx), w) for p in pending])  # noqa: E731
        crop = rec[:, _R["crop"]] = np.concatenate([np.asarray(p.idx, dtype=np.float64) for p in pending])
        rec[:, _R["cls"]] = cat("cls_id", 1).reshape(n).cpu().numpy()
        rec[:, _R["valid"]] = 1.0
        o = 0
        for p in pending:
            if p.lc is not None:
                rec[o:o + len(p.idx), [_R["l_xyz"], _R["l_normal"], _R["l_mask"]]] = p.lc.cpu().numpy()[:, [0, 1, 3]]
            o += len(p.idx)
        tr, tt, score_r, score_t = cat("target_r", 9), cat("target_t", 3), cat("score_r", 9), cat("score_t", 3)
        rec[:, _R["add_b"]] = cat("add_b", 1).reshape(n).cpu().numpy()
        rec[:, _R["r_b"]], rec[:, _R["t_b"]] = rt_errors(cat("base_r", 9), cat("base_t", 3), tr, tt)
        if opt_pose:
            rec[:, _R["add_f"]] = cat("add_f", 1).reshape(n).cpu().numpy()
            rec[:, _R["r_f"]], rec[:, _R["t_f"]] = rt_errors(score_r, score_t, tr, tt)
        if poses:
            prec[:, 0], prec[:, 1:10], prec[:, 10:13] = crop, score_r.double().cpu().numpy(), score_t.double().cpu().numpy()
        if select:
            best = torch.cat([e["best"] for e in sel_pending]).cpu().numpy().astype(np.int64)
            score = np.concatenate([e["score"].cpu().numpy() for e in sel_pending])      # [n, C]: one C per epoch
            counts = np.concatenate([e["counts"].cpu().numpy() for e in sel_pending])    # [n, C, 6]
            rows = np.arange(n)
            srec[:, 0], srec[:, 1], srec[:, 2], srec[:, -1] = crop, best, score[rows, best], 1.0
            srec[:, 3], srec[:, 4] = counts[rows, best, 4], counts[rows, best, 5]
        if bop:
            T = len(TAUS)
            brec[:, 0], brec[:, 1], brec[:, -1] = crop, rec[:, _R["cls"]], 1.0
            brec[:, 2:2 + T] = torch.cat([e["vsd"] for e in bop_pending]).cpu().numpy()
            brec[:, 2 + T] = torch.cat([e["mssd"] for e in bop_pending]).cpu().numpy()
            brec[:, 3 + T] = torch.cat([e["mspd"] for e in bop_pending]).cpu().numpy()
    zstat = None
    if zoom:
        zstat = torch.cat(zoom_pending).cpu().numpy().astype(np.int64) if zoom_pending else np.zeros(0, np.int64)
    return (EpochTables(*(None if t is None else torch.from_numpy(t) for t in (rec, brec, prec, srec))),
            net if net_masks else None, zstat)


def fold_records(records: torch.Tensor, objlist: Sequence[int], diameter: Sequence[float], opt_pose: bool,
                 metric: Metric) -> Dict[str, object]:
    """The reference's per-object bookkeeping (trainer.py:165-250) over per-crop records, in global
    crop order (independent of how crops were batched or sharded)."""
    rec = valid_by_crop(records)
    result = {k: {o: 0.0 for o in objlist} for k in _KEYS}
    cls = rec[:, _R["cls"]].astype(np.int64)
    col = lambda k: rec[:, _R[k]]  # noqa: E731

    def seq_sum(x):  # the reference's running `+=` in crop order (np.cumsum adds sequentially)
        return float(np.cumsum(x)[-1]) if len(x) else 0.0

    # first-appearance order of the objects, as the reference's dict of ADD lists fills
    order = [int(c) for c in dict.fromkeys(cls.tolist())]
    adds: Dict[int, List[float]] = {}
    for c in order:
        obj, dia = objlist[c], diameter[c]
        sel = cls == c
        n = float(sel.sum())
        result["all_num"][obj] = result["obj_num"][obj] = n
        ab, rb, tb = col("add_b")[sel], col("r_b")[sel], col("t_b")[sel]
        result["dis_base_rt"][obj] = seq_sum(ab)
        result["dis_base_r"][obj] = seq_sum(rb)
        result["dis_base_t"][obj] = seq_sum(tb)
        result["succ_base_rt"][obj] = float((ab < 0.1 * dia).sum())
        result["succ_base_r"][obj] = float((rb < ROT_THR_DEG).sum())
        result["succ_base_t"][obj] = float((tb < TRANS_THR_M).sum())
        result["dis_xyz"][obj] = seq_sum(col("l_xyz")[sel])
        result["dis_mask"][obj] = seq_sum(col("l_mask")[sel])
        result["dis_normal"][obj] = seq_sum(col("l_normal")[sel])
        if opt_pose:
            af, rf, tf = col("add_f")[sel], col("r_f")[sel], col("t_f")[sel]
            for k in ("reg", "final"):
                result[f"dis_{k}_rt"][obj] = seq_sum(af)
                result[f"dis_{k}_r"][obj] = seq_sum(rf)
                result[f"dis_{k}_t"][obj] = seq_sum(tf)
                result[f"succ_{k}_rt"][obj] = float((af < 0.1 * dia).sum())
                result[f"succ_{k}_r"][obj] = float((rf < ROT_THR_DEG).sum())
                result[f"succ_{k}_t"][obj] = float((tf < TRANS_THR_M).sum())
            adds[obj] = af.tolist()
        else:
            adds[obj] = ab.tolist()
    out = copy.copy(result)
    out["test_count"] = int(len(rec))
    out["test_dis"] = seq_sum(col("add_f") if opt_pose else col("add_b")) / max(len(rec), 1)
    out["auc"] = {o: metric.cal_auc(v) for o, v in adds.items()}
    out["auc_all"] = metric.cal_auc([a for v in adds.values() for a in v]) if adds else 0.0
    return out


def result_rows(pose_table, items, conf: Dict[int, float]) -> List[Dict[str, object]]:
    """The epoch's scored poses as BOP result rows (bop_scene.write_results' dicts, t in millimetres) in crop order:
    pose_table = the gathered POSE_REC rows plus a `valid` column, items = the BOP tree's (their scene, image and object
    ids), conf = {crop: score}; a crop without one scores 1.0, and time is -1 (not measured per image). What the result
    CSV, the matched recalls and the segmentation result file are all made from."""
    rows = []
    for row in valid_by_crop(pose_table):
        it = items[int(row[0])]
        rows.append({"scene_id": it["scene"], "im_id": it["im"], "obj_id": it["obj"], "score": conf.get(int(row[0]), 1.0),
                     "R": row[1:10], "t": row[10:13] * 1000.0, "time": -1.0})
    return rows


def gather_epoch_records(local: torch.Tensor, shard_sizes: Sequence[int], device, group=None) -> torch.Tensor:
    """All-gather every rank's [n_r, width] records (padded to max(shard_sizes) rows, pad rows have
    valid = 0) -> all ranks' records, rank-major. The width is the table's own: len(REC) for the epoch's
    records, len(bop.BOP_REC) for its BOP table; `valid` is the last column of both."""
    world = len(shard_sizes)
    if world == 1:
        return local
    m = max(shard_sizes)
    pad = torch.zeros((max(m, 1), local.shape[1]), dtype=torch.float64)
    pad[:local.shape[0]] = local
    backend = dist.get_backend(group)
    buf = pad.to(device) if backend == "nccl" else pad
    out = kd.gather_records(buf, group=group)
    return out.cpu()


@torch.no_grad()
def test_epoch(model: KRRN, dataset: PoseDataset, bs: int = 64, device=None, opt_pose: bool = True,
               criterion=None, world: Optional[int] = None, rank: Optional[int] = None,
               group=None, pose_solver: str = "pnp", refine: Optional[str] = None,
               bop: bool = False, bop_csv: Optional[str] = None, select: Optional[str] = None,
               match: bool = False, seg_json: Optional[str] = None, seg_source: str = "render",
               coco: bool = False, zoom: int = 0, vis_dir: Optional[str] = None,
               vis_diff: bool = False) -> Dict[str, object]:
    """Trainer.test_epoch over `dataset`. world/rank default to the initialised process group
    (1/0 without one). `criterion` enables the per-crop map-loss terms (dis_xyz / dis_mask /
    dis_normal) when the batches carry GT maps, i.e. for a PoseDataset built with gt_maps=True (a
    stock LineMOD tree is enough: the maps are rendered from its PLYs); without them the columns stay
    0. The reference always evaluates it (:167).
    `pose_solver` and `refine` as in eval_records. `bop` (off by default; needs a dataset with meshes) adds one
    key, "bop": bop.fold_bop's BOP-19 average recalls AR_VSD / AR_MSSD / AR_MSPD / AR of the final pose, per
    object and overall; every other key is unchanged, bit for bit.
    `bop_csv` (needs a dataset with layout="bop": the rows carry its scene and image ids) writes every crop's scored
    pose as BOP's result CSV (bop_scene.write_results; t in millimetres) in crop order. The pose table is gathered
    like the records and only rank 0 writes. score is 1.0 for every row: there is one estimate per target, so
    nothing ranks on it; time is -1 (not measured per image). The returned dict is unchanged.
    `select` as in eval_records: "depth" chooses every crop's final pose among the epoch's candidates by
    render-and-compare, and adds one key, "select": {"picked": {candidate index: crops}, "mean_score": the mean of
    the kept candidates' scores in crop order}; the final / reg keys, "bop" and the CSV's poses are then the chosen
    pose's, and the CSV's score column is its score (a confidence in [0, 1]). The base keys do not change.
    A dataset built with detections (PoseDataset(..., detections=...)) adds one key, "detections": {"targets" the
    kept GT targets, "estimated" those with a detection (the crops evaluated), "missed" those without, and the
    detection file's "rows", "unused", "dropped" (BopTree.det_stats)}; the missed targets enter every BOP recall's
    denominator (bop.fold_bop(missed=...): "bop" gains "targets"), and the CSV's score column is the detection's
    score unless `select` puts the verification score there. Every other key is computed as before.
    `match` (off by default: nothing changes; needs bop=True and a dataset with layout="bop") computes "bop" the way the
    BOP-19 protocol does instead of one estimate against the GT pose it was cropped from: the epoch's poses become
    result rows exactly as `bop_csv` writes them, and "bop" = bop_scene.eval_results(dataset, rows, device), which
    matches each target's `inst_count` best rows to its GT instances; every other key is as before. A dataset built
    with det_per_target="inst_count" has only a provisional crop-to-instance association, so bop=True without
    match=True raises ValueError on it. With world > 1 rank 0 evaluates the gathered rows and broadcasts the dict
    (dist.broadcast_object_list).
    `seg_json` (off by default: nothing changes; needs a dataset with layout="bop" and meshes=True, else ValueError)
    writes the estimates' masks as a segmentation result file: rank 0 builds the result rows exactly as `bop_csv`
    writes them and calls bop_scene.write_result_masks(seg_json, dataset, rows, device), which renders each pose's
    visible mask against the observed depth and encodes it on the GPU. The file is in the detection format, so
    PoseDataset(layout="bop", detections=seg_json) crops and masks a second pass from this pass's poses. One key is
    added, "seg": {"rows": the rows written, "empty": the estimates without a visible pixel}; no other key changes.
    `seg_source` says whose masks `seg_json` holds: "render" (the default) the rendered ones above; "net" the network's
    own segmentation, the mask head's logits that otherwise only the eval-time cross-entropy reads. It needs seg_json
    and a dataset with layout="bop" but no meshes, and world == 1 (gathering the ranks' ragged run lists is not built);
    ValueError otherwise, before any batch is built. Per batch eval_records(net_masks=True) pastes each crop's decided
    pixels (channel cls_id + 1 wins) into a full-frame plane and encodes it on the GPU; rank 0 builds the result rows
    exactly as `bop_csv` writes them, pairs them with the runs by crop and writes write_detections(seg_json,
    bop_scene.net_mask_rows(...)): a row's bbox is its mask's tight box, a crop without a set pixel gives no row and
    counts as "empty". "seg" is added as above; no other key changes. A dataset built with resize is refused
    (ValueError): the paste does not resample. Everything else here runs on such a dataset unchanged.
    `coco` (off by default: nothing changes; needs seg_json, else ValueError, and the tree's scene_gt_coco.json, which
    bop_scene.write_gt_coco writes) scores the file just written with COCO's average precision: rank 0 adds one key,
    "coco" = bop_scene.eval_coco((root, split), the rows written, device, "segm"); no other key changes. It runs where
    seg_json runs: the ranks' run lists are not gathered.
    `zoom` (0 by default: nothing changes, bit for bit; an integer >= 0, on a dataset built with resize, with
    world == 1; ValueError otherwise, before any batch is built) is the number of zoom-in passes of eval_records:
    every crop is cut again about its estimated pose's projection and the network runs again, `zoom` times, and
    every key above is computed from the last pass. One key is added, "zoom": {"passes": zoom, "recropped" the crops
    whose last pass cut a new window (zoom.pose_windows' status 0), "kept_bad_pose" those that kept their window because
    the pose put a point behind the camera or at a non-finite pixel (status 1), "kept_outside" those whose projection
    missed the frame (status 2)}. Whether the extra passes improve any accuracy figure is unmeasured.
    seg_source="net" is refused on every dataset built with resize, so it never meets zoom.
    `vis_dir` (None by default: nothing is queued, and every key is what it was, bit for bit; needs a dataset with
    layout="bop" and meshes=True and world == 1, which is all one GPU can test; ValueError otherwise, before any batch is
    built) draws the epoch's estimates on their frames: after the epoch the result rows, exactly as `bop_csv` writes
    them, go through bop_scene.vis_results(dataset, rows, vis_dir, device, diff=vis_diff), which writes one PNG per
    image that has a row (and with `vis_diff` one of the rendered against the observed depth). One key is added, "vis":
    what vis_results returned; no other key changes."""
    device = torch.device(device) if device is not None else next(model.parameters()).device
    _check_zoom(zoom, dataset)
    if seg_source not in ("render", "net"):
        raise ValueError(f"seg_source must be 'render' or 'net', got {seg_source!r}")
    net = seg_source == "net"
    if coco and not seg_json:
        raise ValueError("coco=True scores the segmentation file this epoch writes: it needs seg_json")
    if net:
        if getattr(dataset, "resize", None) is not None:
            raise ValueError("seg_source='net' on a dataset built with resize is not built: the paste places the "
                             "crop's pixels one to one and does not resample them to the source window")
        if not seg_json:
            raise ValueError("seg_source='net' writes the network's masks to a file: it needs seg_json")
        _require(dataset, "seg_source='net' writes BOP's scene / image ids: it needs a PoseDataset with layout='bop'",
                 layout=True)
    elif seg_json:
        _require(dataset, "seg_json renders the estimates' masks on a BOP tree: it needs a PoseDataset with layout='bop' "
                 "and meshes=True", layout=True, meshes=True)
    if match:
        msg = "match=True scores result rows against a BOP tree: it needs bop=True and a PoseDataset with layout='bop'"
        if not bop:
            raise ValueError(msg)
        _require(dataset, msg, layout=True)
    if bop and not match and getattr(getattr(dataset, "tree", None), "det_per_target", "best") == "inst_count":
        raise ValueError("a dataset built with det_per_target='inst_count' pairs crops with GT instances only "
                         "provisionally: bop=True needs match=True on it")
    if bop_csv:
        _require(dataset, "bop_csv writes BOP's scene / image ids: it needs a PoseDataset with layout='bop'", layout=True)
    if vis_dir:
        _require(dataset, "vis_dir draws the estimates on a BOP tree's frames: it needs a PoseDataset with layout='bop' "
                 "and meshes=True", layout=True, meshes=True)
    if world is None:
        world = dist.get_world_size(group) if dist.is_initialized() else 1
    if rank is None:
        rank = dist.get_rank(group) if dist.is_initialized() else 0
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside world {world}")
    if net and world > 1:
        raise ValueError("seg_source='net' runs on one rank: gathering the ranks' run lists is not built")
    if zoom and world > 1:
        raise ValueError("zoom runs on one rank: it is not tested across ranks, and the status counts are not gathered")
    if vis_dir and world > 1:
        raise ValueError("vis_dir runs on one rank: it is not tested across ranks")
    sizes = [dataset.crop_size(i) for i in range(len(dataset))]
    mine = kd.bucket_shard(sizes, world, rank)
    want_poses = bool(bop_csv or match or seg_json or vis_dir)
    local, runs, zstat = _eval_epoch(model, dataset, mine, bs, device, opt_pose, criterion is not None, pose_solver,
                                     refine, bool(bop), want_poses, select, net, int(zoom))
    net_runs = {crop: (r, info) for crop, r, info in runs or ()}
    shard_sizes = [sum(len(v) for v in kd.bucket_shard(sizes, world, r).values()) for r in range(world)]
    gather = lambda t: gather_epoch_records(t, shard_sizes, device, group) if world > 1 else t  # noqa: E731
    metric = Metric(dataset.sym_obj)
    out = fold_records(gather(local.rec), dataset.objlist, dataset.diameter, opt_pose, metric)
    if zoom:
        out["zoom"] = {"passes": int(zoom), "recropped": int((zstat == 0).sum()),
                       "kept_bad_pose": int((zstat == 1).sum()), "kept_outside": int((zstat == 2).sum())}
    det = bool(getattr(dataset, "detections", False))  # a detection-mode dataset: targets without an estimate count
    missed: Dict[int, int] = {}
    for _, _, obj in (dataset.tree.missed if det else ()):
        missed[obj] = missed.get(obj, 0) + 1
    if bop:  # a record table of its own, gathered by the same mechanism
        out["bop"] = fold_bop(gather(local.bop), dataset.objlist, dataset.diameter,
                              getattr(dataset, "frame_hw", (0, FRAME_W))[1], missed if det else None)
    conf = {}
    if det:
        st = dataset.tree.det_stats
        out["detections"] = {"targets": len(dataset) + len(dataset.tree.missed), "estimated": len(dataset),
                             "missed": len(dataset.tree.missed), "rows": st["rows"], "unused": st["unused"],
                             "dropped": st["dropped"]}
        conf = {i: float(it["score"]) for i, it in enumerate(dataset.tree.items)}
    if select:
        tab = valid_by_crop(gather(local.sel))
        picked = {int(c): int((tab[:, 1] == c).sum()) for c in sorted(set(tab[:, 1].tolist()))}
        out["select"] = {"picked": picked, "mean_score": float(np.cumsum(tab[:, 2])[-1]) / len(tab) if len(tab) else 0.0}
        conf = {int(r[0]): float(r[2]) for r in tab}
    if want_poses:
        # gather_epoch_records marks pad rows by a last column `valid` = 0
        allpose = gather(torch.cat([local.poses, torch.ones((local.poses.shape[0], 1), dtype=torch.float64)], 1))
        rows = result_rows(allpose, dataset.tree.items, conf) if rank == 0 else None
        if bop_csv and rank == 0:
            write_results(bop_csv, rows)
        if net:
            crops = [int(r[0]) for r in valid_by_crop(allpose)]  # result_rows' order
            det, st = net_mask_rows(rows, [net_runs[c][0] for c in crops], [net_runs[c][1] for c in crops],
                                    *dataset.frame_hw)
            write_detections(seg_json, det)
            out["seg"] = {"rows": len(det), "empty": st["empty"]}
            if coco:
                out["coco"] = eval_coco((dataset.tree.root, dataset.tree.split), det, device, "segm")
        elif seg_json:
            res = [None, None]
            if rank == 0:
                det, st = write_result_masks(seg_json, dataset, rows, device)
                res = [{"rows": len(det), "empty": st["empty"]},
                       eval_coco((dataset.tree.root, dataset.tree.split), det, device, "segm") if coco else None]
            if world > 1:
                dist.broadcast_object_list(res, src=0, group=group)
            out["seg"] = res[0]
            if coco:
                out["coco"] = res[1]
        if match:  # the protocol's recalls over the rows, in place of the 1 : 1 fold above
            res = [eval_results(dataset, rows, device)] if rank == 0 else [None]
            if world > 1:
                dist.broadcast_object_list(res, src=0, group=group)
            out["bop"] = res[0]
        if vis_dir:
            out["vis"] = vis_results(dataset, rows, vis_dir, device, diff=bool(vis_diff))
    if world > 1:
        # the ranks' own crop / success tallies, summed, must equal the gathered table's
        key = "add_f" if opt_pose else "add_b"
        dia = torch.tensor([dataset.diameter[int(c)] for c in local.rec[:, _R["cls"]]], dtype=torch.float64)
        mine_t = torch.tensor([float(local.rec.shape[0]), float((local.rec[:, _R[key]] < 0.1 * dia).sum())],
                              dtype=torch.float64)
        t = mine_t.to(device) if dist.get_backend(group) == "nccl" else mine_t
        dist.all_reduce(t, group=group)
        tot = t.cpu()
        succ_key = "succ_final_rt" if opt_pose else "succ_base_rt"
        assert int(tot[0]) == out["test_count"], (tot, out["test_count"])
        assert int(tot[1]) == int(sum(out[succ_key].values())), (tot, out[succ_key])
    return out
