"""krrn_bop_match_f64 (include/krrn_hip.h) and bop_scene.eval_results restated in numpy, cell by cell, from the
stated definition. Not a test.

match_cell: one (group, error function, threshold) cell. match_poses: the kernel's arrays in, its two outputs out.
eval_results: a BopTree and result rows in, the recalls out: every (estimate, instance) pair's errors come from
bop_ref.vsd / bop_ref.mssd_mspd one pair at a time, the thresholds from bop.THETAS / THETAS_PX, the matching from
match_cell, the averages in bop._recalls' order. It also returns every pair's VSD restatement and the MSSD / MSPD
errors with their thresholds, so that a test can assert the decision margins on them."""
import numpy as np

import bop_ref as br

MAX = 128


def order(scores, n_top):
    """The estimates that take part, in matching order: score descending, ties to the lower index, NaN as -inf."""
    s = [(-np.inf if np.isnan(x) else float(x)) for x in scores]
    idx = sorted(range(len(s)), key=lambda i: (-s[i], i))
    return idx if n_top <= 0 else idx[:n_top]


def match_cell(scores, err, thr, n_top):
    """scores [n_est], err [n_est, n_gt] (one error function), thr a scalar. Returns (match [n_gt] = local estimate
    index or -1, tp)."""
    err = np.asarray(err, np.float64)
    n_gt = err.shape[1] if err.ndim == 2 else 0
    match = np.full(n_gt, -1)
    with np.errstate(invalid="ignore"):
        below = err < thr                                # strict; False for a NaN error or a NaN threshold
    for e in order(scores, n_top) if n_gt else ():
        cand = below[e] & (match < 0)
        if cand.any():                                   # a candidate's error is < thr <= inf: never +inf
            match[int(np.argmin(np.where(cand, err[e], np.inf)))] = e   # argmin: the lowest j on ties
    return match.tolist(), int((match >= 0).sum())


def match_poses(score, err, est_range, gt_range, pair_off, thr, n_top, n_inst, max_est=MAX, max_gt=MAX, fill=None):
    """The kernel's outputs (match int32 [n_inst, C, NT], tp int32 [G, C, NT]) for its inputs; `fill` is what an
    instance that no group owns keeps."""
    score, err, thr = np.asarray(score, np.float64), np.asarray(err, np.float64), np.asarray(thr, np.float64)
    G, C, NT = thr.shape
    match = np.full((n_inst, C, NT), -7 if fill is None else fill, np.int32)
    tp = np.zeros((G, C, NT), np.int32)
    for g in range(G):
        (e0, ne), (g0, ng), p0 = (int(v) for v in est_range[g]), (int(v) for v in gt_range[g]), int(pair_off[g])
        gt_ok = g0 >= 0 and ng >= 0 and g0 + ng <= n_inst
        ok = (gt_ok and ng <= max_gt and e0 >= 0 and 0 <= ne <= max_est and e0 + ne <= len(score) and p0 >= 0
              and p0 + ne * ng <= len(err))
        if gt_ok:
            match[g0:g0 + ng] = -1
        if not ok or ne == 0 or ng == 0:
            continue
        block = err[p0:p0 + ne * ng].reshape(ne, ng, C)
        for c in range(C):
            for k in range(NT):
                m, n = match_cell(score[e0:e0 + ne], block[:, :, c], thr[g, c, k], int(n_top[g]))
                match[g0:g0 + ng, c, k] = [e0 + x if x >= 0 else -1 for x in m]
                tp[g, c, k] = n
    return match, tp


# ------------------------------------------------------------------------------------------ eval_results

def _mean_recall(tp, n):
    """bop._recalls' averages from integer tp [T + 2, NT] and the denominator n."""
    T = tp.shape[0] - 2
    if n == 0:
        return 0.0, 0.0, 0.0
    ar_vsd = float(np.mean([tp[:T, k].sum() / (n * T) for k in range(tp.shape[1])]))
    ar_mssd = float(np.mean([tp[T, k] / n for k in range(tp.shape[1])]))
    ar_mspd = float(np.mean([tp[T + 1, k] / n for k in range(tp.shape[1])]))
    return ar_vsd, ar_mssd, ar_mspd


def _entry(tp, n, count):
    if n == 0 or count == 0:
        return {"AR_VSD": 0.0, "AR_MSSD": 0.0, "AR_MSPD": 0.0, "AR": 0.0, "count": int(count), "targets": int(n)}
    v, s, p = _mean_recall(tp, n)
    return {"AR_VSD": v, "AR_MSSD": s, "AR_MSPD": p, "AR": (v + s + p) / 3.0, "count": int(count), "targets": int(n)}


def eval_results(tree, rows, thetas, thetas_px, delta=br.DELTA, taus=br.TAUS):
    """tree: a bop_scene.BopTree built with meshes=True. Returns the dict eval_results returns, plus "pairs": per
    (estimate row, instance index) the bop_ref.vsd restatement, the MSSD / MSPD errors and their threshold lists."""
    T, NT = len(taus), len(thetas)
    groups = {}
    for i, it in enumerate(tree.instances):
        groups.setdefault((int(it["scene"]), int(it["im"]), int(it["obj"])), []).append(i)
    est = {k: [] for k in groups}
    ignored = 0
    for r, row in enumerate(rows):
        key = (int(row["scene_id"]), int(row["im_id"]), int(row["obj_id"]))
        if key in est:
            est[key].append(r)
        else:
            ignored += 1
    width = tree.frame_hw[1]
    objs = list(dict.fromkeys(k[2] for k in groups))
    tp_obj = {o: np.zeros((T + 2, NT), np.int64) for o in objs}
    n_obj, c_obj = {o: 0 for o in objs}, {o: 0 for o in objs}
    matches = [-1] * len(tree.instances)
    pairs = {}
    depth = {}
    for key, inst in groups.items():
        sc, im, obj = key
        it0 = tree.instances[inst[0]]
        if (sc, im) not in depth:
            depth[(sc, im)] = tree.read_image(sc, im, float(it0["depth_scale"]))[1]
        v, f = tree.mesh[obj]
        dia = float(tree.info[obj]["diameter"]) / 1000.0
        thr = np.stack([np.asarray(thetas, np.float64)] * T + [np.asarray(thetas, np.float64) * dia]
                       + [np.asarray(thetas_px, np.float64) * (width / 640.0)])
        err = np.zeros((len(est[key]), len(inst), T + 2))
        for a, r in enumerate(est[key]):
            Re, te = np.asarray(rows[r]["R"], np.float64).reshape(3, 3), np.asarray(rows[r]["t"], np.float64) / 1000.0
            for b, i in enumerate(inst):
                it = tree.instances[i]
                res = br.vsd(v, f, Re, te, it["R"], it["t"], it["K4"], depth[(sc, im)], 1.0, dia, delta, taus)
                m3, m2 = br.mssd_mspd(v, Re, te, it["R"], it["t"], it["K4"], tree.symmetries[obj])[:2]
                err[a, b, :T], err[a, b, T], err[a, b, T + 1] = res["e_vsd"], m3, m2
                pairs[(r, i)] = {"vsd": res, "mssd": m3, "mspd": m2, "thr_mssd": thr[T], "thr_mspd": thr[T + 1]}
        scores = [float(rows[r]["score"]) for r in est[key]]
        n_top = tree.inst_count[key]
        n_obj[obj] += len(inst)
        c_obj[obj] += len(order(scores, n_top))
        for c in range(T + 2):
            for k in range(NT):
                m, n = match_cell(scores, err[:, :, c], thr[c, k], n_top)
                tp_obj[obj][c, k] += n
                if c == T and k == NT - 1:
                    for b, x in enumerate(m):
                        matches[inst[b]] = est[key][x] if x >= 0 else -1
    out = _entry(sum(tp_obj.values()) if objs else np.zeros((T + 2, NT), np.int64), sum(n_obj.values()),
                 sum(c_obj.values()))
    out["per_obj"] = {o: _entry(tp_obj[o], n_obj[o], c_obj[o]) for o in objs}
    out["ignored"], out["matches"], out["pairs"] = ignored, matches, pairs
    return out
