"""COCO's average precision restated in numpy (not a test), written loop by loop from the definition in
include/krrn_hip.h and pose_estimation_amd/coco.py (pycocotools' published evaluateImg / accumulate / summarize; not
cross-checked with pycocotools, which is not a dependency). Mask IoU goes through decoded planes (rle_ref.decode, `&`,
`|`, sum): an independent route from the kernel's run arithmetic."""
import numpy as np

import rle_ref as rf

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
AREA_RNG = np.array([[0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]])
MAX_DETS = (1, 10, 100)


def _ratio(num, den):
    return float(np.float64(num) / np.float64(den)) if den > 0 else 0.0


def mask_iou(planes, pair, crowd=None):
    """(inter int [P], iou f64 [P], area int [n]) of pairs of u8 planes; a pair index outside [0, n) gives 0."""
    n = len(planes)
    area = np.array([int(p.sum()) for p in planes], np.int64).reshape(n)
    inter, iou = np.zeros(len(pair), np.int64), np.zeros(len(pair), np.float64)
    for p, (a, b) in enumerate(pair):
        if not (0 <= a < n and 0 <= b < n):
            continue
        i = int((planes[a].astype(bool) & planes[b].astype(bool)).sum())
        u = int((planes[a].astype(bool) | planes[b].astype(bool)).sum())
        inter[p] = i
        iou[p] = _ratio(i, area[a]) if crowd is not None and crowd[p] else _ratio(i, u)
    return inter, iou, area


def box_iou(a, b, crowd=False):
    """bop_scene._box_iou's arithmetic restated, with COCO's crowd form."""
    ax, ay, aw, ah = (float(v) for v in a)
    bx, by, bw, bh = (float(v) for v in b)
    iw = max(0.0, min(ax + aw, bx + bw) - max(ax, bx))
    ih = max(0.0, min(ay + ah, by + bh) - max(ay, by))
    inter = iw * ih
    area_a = max(aw, 0.0) * max(ah, 0.0)
    den = area_a if crowd else area_a + max(bw, 0.0) * max(bh, 0.0) - inter
    return inter / den if den > 0.0 else 0.0


def order(score):
    """Indices by score descending, ties to the lower index, NaN as -inf."""
    key = [float("-inf") if s != s else float(s) for s in score]
    return sorted(range(len(key)), key=lambda i: (-key[i], i))


def evaluate_img(score, iou, det_area, gt_area, gt_flags, area_rng=AREA_RNG, iou_thr=IOU_THRS, max_det=100):
    """One group: iou [nd][ng]. Returns dt_match int [nd, A, T] (the group's local ground-truth index or -1), dt_ig
    [nd, A, T], gt_ig [ng, A], rank [nd]."""
    nd, ng, A, T = len(score), len(gt_area), len(area_rng), len(iou_thr)
    dt_match = -np.ones((nd, A, T), np.int64)
    dt_ig = np.ones((nd, A, T), np.uint8)
    gt_ig = np.zeros((ng, A), np.uint8)
    rank = -np.ones(nd, np.int64)
    dets = order(score)
    for r, d in enumerate(dets):
        if r < max_det:
            rank[d] = r
    dets = dets[:max_det]
    for a in range(A):
        lo, hi = float(area_rng[a][0]), float(area_rng[a][1])
        ig = [bool(gt_flags[j] != 0 or gt_area[j] < lo or gt_area[j] > hi) for j in range(ng)]
        for j in range(ng):
            gt_ig[j, a] = ig[j]
        walk = [j for j in range(ng) if not ig[j]] + [j for j in range(ng) if ig[j]]
        for t in range(T):
            taken = [False] * ng
            for d in dets:
                best, m = min(float(iou_thr[t]), 1 - 1e-10), -1
                for j in walk:
                    if taken[j] and not (gt_flags[j] & 1):
                        continue
                    if m >= 0 and not ig[m] and ig[j]:
                        break
                    v = float(iou[d][j])
                    if v != v or v < best:
                        continue
                    best, m = v, j
                if m >= 0:
                    dt_match[d, a, t], dt_ig[d, a, t], taken[m] = m, ig[m], True
                else:
                    dt_ig[d, a, t] = bool(det_area[d] < lo or det_area[d] > hi)
    return dt_match, dt_ig, gt_ig, rank


def hand_cases():
    """[(name, evaluate_img's arguments, what was worked out by hand: {"dt": {(d, a, t): (match, ig)}, "gt_ig": {(j,
    a): ig}, "rank": {d: rank}})]. Area ranges 0 .. 3 = all, small, medium, large; thresholds 0, 1, 3 = 0.5, 0.55,
    0.65. An area of 2000 is medium."""
    one = dict(score=[0.9], det_area=[2000.0], gt_area=[2000.0], gt_flags=[0])
    below = float(np.nextafter(0.5, 0.0))
    many = [0.5 + 0.001 * i for i in range(101)]         # detection 0 scores lowest
    return [
        ("iou_exactly_half", dict(one, iou=[[0.5]]), {"dt": {(0, 0, 0): (0, 0), (0, 2, 0): (0, 0), (0, 0, 1): (-1, 0),
                                                             (0, 1, 0): (0, 1)}}),    # not small: ignored there
        ("iou_just_below_half", dict(one, iou=[[below]]), {"dt": {(0, 0, 0): (-1, 0), (0, 2, 0): (-1, 0)}}),
        ("equal_iou_takes_the_later", dict(score=[0.9], iou=[[0.7, 0.7]], det_area=[2000.0], gt_area=[2000.0, 2000.0],
                                           gt_flags=[0, 0]), {"dt": {(0, 0, 0): (1, 0), (0, 0, 3): (1, 0)}}),
        ("crowd_matched_twice", dict(score=[0.9, 0.8], iou=[[0.8], [0.6]], det_area=[2000.0, 2000.0], gt_area=[2000.0],
                                     gt_flags=[1]), {"dt": {(0, 0, 0): (0, 1), (1, 0, 0): (0, 1), (1, 0, 3): (-1, 0)}}),
        ("two_detections_one_plain_gt", dict(score=[0.9, 0.8], iou=[[0.8], [0.6]], det_area=[2000.0, 2000.0],
                                             gt_area=[2000.0], gt_flags=[0]), {"dt": {(0, 0, 0): (0, 0), (1, 0, 0): (-1, 0)}}),
        # the counted match at 0.6 is kept although the ignored ground truth overlaps more; above 0.6 only that one is left
        ("stop_rule", dict(score=[0.9], iou=[[0.6, 0.9]], det_area=[2000.0], gt_area=[2000.0, 2000.0], gt_flags=[0, 2]),
         {"dt": {(0, 0, 0): (0, 0), (0, 0, 1): (0, 0), (0, 0, 3): (1, 1)}, "gt_ig": {(0, 0): 0, (1, 0): 1}}),
        # the walk takes the counted ground truth first although the ignored one has the lower index
        ("ignored_are_walked_last", dict(score=[0.9], iou=[[0.9, 0.6]], det_area=[2000.0], gt_area=[2000.0, 2000.0],
                                         gt_flags=[2, 0]), {"dt": {(0, 0, 0): (1, 0), (0, 0, 3): (0, 1)}}),
        ("area_of_32_squared_is_small_and_medium", dict(score=[0.9], iou=[[0.9]], det_area=[1024.0], gt_area=[1024.0],
                                                        gt_flags=[0]),
         {"gt_ig": {(0, 0): 0, (0, 1): 0, (0, 2): 0, (0, 3): 1}, "dt": {(0, 1, 0): (0, 0), (0, 2, 0): (0, 0), (0, 3, 0): (0, 1)}}),
        ("the_101st_detection", dict(score=many, iou=[[0.9]] * 101, det_area=[2000.0] * 101, gt_area=[2000.0],
                                     gt_flags=[0]), {"rank": {0: -1, 1: 99, 100: 0}, "dt": {(0, 0, 0): (-1, 1), (100, 0, 0): (0, 0),
                                                                                           (1, 0, 0): (-1, 0)}}),
        ("nan_iou_and_nan_score", dict(score=[float("nan"), 0.1], iou=[[0.9, float("nan")], [float("nan"), 0.9]],
                                       det_area=[2000.0, 2000.0], gt_area=[2000.0, 2000.0], gt_flags=[0, 0]),
         {"rank": {0: 1, 1: 0}, "dt": {(0, 0, 0): (0, 0), (1, 0, 0): (1, 0)}}),
    ]


def accumulate(groups, n_cat, max_dets=MAX_DETS):
    """groups: [{"cat": k, "score" [nd], "rank" [nd], "dt_match" [nd, A, T], "dt_ig" [nd, A, T], "gt_ig" [ng, A]}] in
    image order. Returns (precision [T, 101, n_cat, A, M], recall [T, n_cat, A, M])."""
    A, T = groups[0]["dt_match"].shape[1:] if groups else (len(AREA_RNG), len(IOU_THRS))
    M, R = len(max_dets), len(REC_THRS)
    precision = -np.ones((T, R, n_cat, A, M))
    recall = -np.ones((T, n_cat, A, M))
    for k in range(n_cat):
        E = [g for g in groups if g["cat"] == k]
        for a in range(A):
            for mi, max_det in enumerate(max_dets):
                npig = sum(int(not v) for g in E for v in g["gt_ig"][:, a])
                if npig == 0:
                    continue
                dets = []                                # (score, group, detection) in concatenation order
                for gi, g in enumerate(E):
                    ds = sorted((d for d in range(len(g["score"])) if 0 <= g["rank"][d] < max_det),
                                key=lambda d: g["rank"][d])
                    dets += [(float(g["score"][d]), gi, d) for d in ds]
                idx = np.argsort(-np.array([s for s, _, _ in dets], np.float64), kind="mergesort") if dets else []
                dets = [dets[i] for i in idx]
                nd = len(dets)
                for t in range(T):
                    tp, fp, ntp, nfp = np.zeros(nd), np.zeros(nd), 0, 0
                    for i, (_, gi, d) in enumerate(dets):
                        matched, ig = E[gi]["dt_match"][d, a, t] >= 0, bool(E[gi]["dt_ig"][d, a, t])
                        ntp += int(matched and not ig)
                        nfp += int(not matched and not ig)
                        tp[i], fp[i] = ntp, nfp
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, mi] = rc[-1] if nd else 0.0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, thr in enumerate(REC_THRS):
                        pi = 0
                        while pi < nd and rc[pi] < thr:  # searchsorted(rc, thr, side="left")
                            pi += 1
                        precision[t, ri, k, a, mi] = pr[pi] if pi < nd else 0.0
    return precision, recall


def _mean(values):
    v = np.array([x for x in values if x > -1], np.float64)
    return float(np.mean(v)) if len(v) else -1.0


def summarize(precision, recall, cats, iou_thr=IOU_THRS, max_dets=MAX_DETS):
    T, R, K = precision.shape[:3]
    last = len(max_dets) - 1
    t50 = int(np.argmin(np.abs(np.asarray(iou_thr) - 0.5)))
    t75 = int(np.argmin(np.abs(np.asarray(iou_thr) - 0.75)))

    def ap(a, ts=None, ks=None):
        return _mean(precision[t, r, k, a, last] for t in (ts or range(T)) for r in range(R) for k in (ks or range(K)))

    def ar(mi, ks=None):
        return _mean(recall[t, k, 0, mi] for t in range(T) for k in (ks or range(K)))

    out = {"AP": ap(0), "AP50": ap(0, [t50]), "AP75": ap(0, [t75]), "AP_small": ap(1), "AP_medium": ap(2),
           "AP_large": ap(3)}
    for mi, m in enumerate(max_dets):
        out[f"AR{m}"] = ar(mi)
    out["per_obj"] = {int(c): {"AP": ap(0, ks=[k]), f"AR{max_dets[last]}": ar(last, [k])} for k, c in enumerate(cats)}
    return out


def eval_rows(gts, rows, iou_type="segm", use_ignore=True, limit=128):
    """bop_scene.eval_coco restated on the host: gts = {scene: coco dict}, rows in the normal form (segmentation
    counts as run lists)."""
    from pose_estimation_amd import rle
    size, gt_by, det_by, ignored = {}, {}, {}, 0
    cats = sorted({int(c["id"]) for coco in gts.values() for c in coco["categories"]})
    for sc in gts:
        for im in gts[sc]["images"]:
            size[(int(sc), int(im["id"]))] = (int(im["height"]), int(im["width"]))
        for a in gts[sc]["annotations"]:
            gt_by.setdefault((int(sc), int(a["image_id"]), int(a["category_id"])), []).append(a)
    for r, row in enumerate(rows):
        key = (row["scene_id"], row["image_id"], row["category_id"])
        if key[:2] not in size or key[2] not in cats:
            ignored += 1
        else:
            det_by.setdefault(key, []).append(r)
    groups, count, targets = [], 0, 0
    for key in sorted(set(gt_by) | set(det_by)):
        H, W = size[key[:2]]
        rs, anns = det_by.get(key, []), gt_by.get(key, [])
        if len(rs) > limit:
            rs = sorted(order([rows[r]["score"] for r in rs])[:limit])
            rs = [det_by[key][i] for i in rs]
        crowd = [bool(a.get("iscrowd", 0)) for a in anns]
        if iou_type == "segm":
            dp = [rf.decode(rows[r]["segmentation"]["counts"], H, W) for r in rs]
            gp = [rf.decode(rle.counts_from_string(a["segmentation"]["counts"]) if isinstance(
                a["segmentation"]["counts"], str) else a["segmentation"]["counts"], H, W) for a in anns]
            pair = [(d, len(dp) + j) for d in range(len(dp)) for j in range(len(gp))]
            _, iou, area = mask_iou(dp + gp, pair, [crowd[j - len(dp)] for _, j in pair])
            iou = iou.reshape(len(dp), len(gp))
            det_area = [float(v) for v in area[:len(dp)]]
        else:
            iou = np.array([[box_iou(rows[r]["bbox"], a["bbox"], crowd[j]) for j, a in enumerate(anns)] for r in rs],
                           np.float64).reshape(len(rs), len(anns))
            det_area = [max(rows[r]["bbox"][2], 0.0) * max(rows[r]["bbox"][3], 0.0) for r in rs]
        flags = [int(crowd[j]) | (2 if use_ignore and a.get("ignore", False) else 0) for j, a in enumerate(anns)]
        score = [rows[r]["score"] for r in rs]
        dm, di, gi, rk = evaluate_img(score, iou, det_area, [float(a["area"]) for a in anns], flags)
        groups.append({"cat": cats.index(key[2]), "score": score, "rank": rk, "dt_match": dm, "dt_ig": di, "gt_ig": gi})
        count, targets = count + len(rs), targets + len(anns)
    out = summarize(*accumulate(groups, len(cats)), cats)
    out["count"], out["targets"], out["ignored"] = count, targets, ignored
    return out
