"""krrn_coco_match_f64 on the GPU: dt_match, dt_ig, gt_ig and rank equal to tests/coco_ref.py's evaluate_img, on the
hand-worked cases and on random groups at the sizes where the kernel changes path (0, 1, 2, the 64-bit halves of the
matched set, the limit of 128), with every output inside a guarded buffer (tests/guarded.py)."""
import numpy as np
import pytest
import torch

import coco_ref as cr
from guarded import Guarded
from pose_estimation_amd import _lib, coco
from pose_estimation_amd._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu

AREA8 = np.array([[0.0, 1e10], [0.0, 1024.0], [1024.0, 9216.0], [9216.0, 1e10], [500.0, 500.0], [0.0, 0.0], [600.0, 5000.0],
                  [1e10, 0.0]])
THR16 = np.concatenate([cr.IOU_THRS, [0.0, 0.25, 0.3, 0.999, 1.0, 1.5]])
FORMS = {"1x1": (cr.AREA_RNG[:1], cr.IOU_THRS[:1], 1), "4x10": (cr.AREA_RNG, cr.IOU_THRS, 100), "8x16": (AREA8, THR16, 128)}
SIZES = {"1x1": [(0, 0), (1, 1), (2, 2), (65, 63), (128, 64)],
         "4x10": [(0, 0), (0, 3), (3, 0), (1, 1), (2, 2), (63, 65), (64, 64), (65, 63), (128, 128), (128, 1), (1, 128), (2, 64)],
         "8x16": [(0, 0), (1, 1), (2, 2), (65, 63), (128, 64)]}


def _random_group(rng, nd, ng):
    grid = np.concatenate([cr.IOU_THRS, [0.0, 0.3, 0.5 - 2.0 ** -53, 1.0, float("nan")]])
    score = rng.choice([0.1, 0.3, 0.3, 0.6, 0.6, 0.6, 0.9], nd).astype(np.float64)
    if nd > 1:
        score[int(rng.integers(0, nd))] = float("nan")
    areas = [0.0, 500.0, 1024.0, 5000.0, 9216.0, 20000.0]
    return dict(score=score.tolist(), iou=rng.choice(grid, (nd, ng)), det_area=rng.choice(areas, nd).tolist(),
                gt_area=rng.choice(areas, ng).tolist(), gt_flags=[int(v) for v in rng.choice([0, 0, 0, 1, 2, 3], ng)])


def _launch(dev, groups, area_rng, iou_thr, max_det, lim_det=128, lim_gt=128):
    """The groups packed and matched, every output guarded. Returns host arrays and the groups' ranges."""
    f64 = lambda x: torch.tensor(np.asarray(x, np.float64).reshape(-1), dtype=torch.float64, device=dev)  # noqa: E731
    i32 = lambda x: torch.tensor(np.asarray(x, np.int64).reshape(-1), dtype=torch.int32, device=dev)      # noqa: E731
    dr, gr, po, d0, g0, p0 = [], [], [], 0, 0, 0
    for g in groups:
        nd, ng = len(g["score"]), len(g["gt_area"])
        dr.append((d0, nd)), gr.append((g0, ng)), po.append(p0)
        d0, g0, p0 = d0 + nd, g0 + ng, p0 + nd * ng
    cat = lambda k: np.concatenate([np.asarray(g[k], np.float64).reshape(-1) for g in groups])  # noqa: E731
    A, T = len(area_rng), len(iou_thr)
    ops = [f64(cat("score")), i32(dr), i32(gr), i32(po), f64(cat("iou")), f64(cat("det_area")), f64(cat("gt_area")),
           i32(cat("gt_flags")), f64(area_rng), f64(iou_thr)]
    out = {"dt_match": Guarded(dev, (d0, A, T)), "dt_ig": Guarded(dev, (d0, A, T), torch.uint8),
           "gt_ig": Guarded(dev, (g0, A), torch.uint8), "rank": Guarded(dev, (d0,))}
    sc, dr_t, gr_t, po_t, io, da, ga, gf, ar, th = ops
    _lib.call("krrn_coco_match_f64", ptr(sc), d0, ptr(dr_t), ptr(gr_t), ptr(po_t), ptr(io), p0, ptr(da), ptr(ga), ptr(gf),
              g0, ptr(ar), A, ptr(th), T, max_det, lim_det, lim_gt, len(groups), out["dt_match"].ptr, out["dt_ig"].ptr,
              out["gt_ig"].ptr, out["rank"].ptr, stream_ptr(dev))
    torch.cuda.synchronize()
    return {k: v.get() for k, v in out.items()}, dr, gr


def _reference(groups, area_rng, iou_thr, max_det):
    """evaluate_img per group, packed as the kernel packs: global ground-truth indices."""
    dm, di, gi, rk, g0 = [], [], [], [], 0
    for g in groups:
        m, i, q, r = cr.evaluate_img(area_rng=area_rng, iou_thr=iou_thr, max_det=max_det, **g)
        dm.append(np.where(m >= 0, m + g0, -1)), di.append(i), gi.append(q), rk.append(r)
        g0 += len(g["gt_area"])
    A, T = len(area_rng), len(iou_thr)
    return {"dt_match": np.concatenate(dm).reshape(-1, A, T), "dt_ig": np.concatenate(di).reshape(-1, A, T),
            "gt_ig": np.concatenate(gi).reshape(-1, A), "rank": np.concatenate(rk)}


def _equal(got, want, where):
    for k in ("rank", "gt_ig", "dt_ig", "dt_match"):
        assert got[k].shape == want[k].shape, (where, k)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (where, k, len(bad), bad[:5].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


_cache = {}


def _world(form):
    """The random groups of a form and their restatement, computed once."""
    if form not in _cache:
        rng = np.random.default_rng(sorted(FORMS).index(form))
        groups = [_random_group(rng, nd, ng) for nd, ng in SIZES[form]]
        _cache[form] = (groups, _reference(groups, *FORMS[form]))
    return _cache[form]


def test_hand_worked_cases(dev):
    cases = cr.hand_cases()
    groups = [c[1] for c in cases]
    got, dr, gr = _launch(dev, groups, cr.AREA_RNG, cr.IOU_THRS, 100)
    _equal(got, _reference(groups, cr.AREA_RNG, cr.IOU_THRS, 100), "hand")
    for (name, _, expect), (d0, _), (g0, _) in zip(cases, dr, gr):    # and against the figures worked out by hand
        for (d, a, t), (m, ig) in expect.get("dt", {}).items():
            assert got["dt_match"][d0 + d, a, t] == (g0 + m if m >= 0 else -1) and got["dt_ig"][d0 + d, a, t] == ig, name
        for (j, a), ig in expect.get("gt_ig", {}).items():
            assert got["gt_ig"][g0 + j, a] == ig, name
        for d, r in expect.get("rank", {}).items():
            assert got["rank"][d0 + d] == r, name


@pytest.mark.parametrize("form", sorted(FORMS))
def test_random_groups(dev, form):
    groups, want = _world(form)
    got, _, _ = _launch(dev, groups, *FORMS[form])
    _equal(got, want, form)
    assert (want["dt_match"] >= 0).any() and (want["dt_ig"] == 0).any() and (want["rank"] == -1).any() == (form != "8x16")


def test_a_group_alone_equals_the_group_in_the_batch(dev):
    groups, _ = _world("4x10")
    got, dr, gr = _launch(dev, groups, *FORMS["4x10"])
    for g in (5, 8, 10):                                 # 63 x 65, 128 x 128, 1 x 128
        alone, _, _ = _launch(dev, [groups[g]], *FORMS["4x10"])
        (d0, nd), (g0, ng) = dr[g], gr[g]
        m = got["dt_match"][d0:d0 + nd]
        assert np.array_equal(alone["dt_match"], np.where(m >= 0, m - g0, -1))
        assert np.array_equal(alone["dt_ig"], got["dt_ig"][d0:d0 + nd]) and np.array_equal(alone["rank"], got["rank"][d0:d0 + nd])
        assert np.array_equal(alone["gt_ig"], got["gt_ig"][g0:g0 + ng])


def test_a_group_past_a_limit_is_matched_as_empty(dev):
    groups, want = _world("1x1")
    area_rng, iou_thr, max_det = FORMS["1x1"]
    got, dr, gr = _launch(dev, groups, area_rng, iou_thr, max_det, lim_det=64, lim_gt=63)
    for g, ((d0, nd), (g0, ng)) in enumerate(zip(dr, gr)):
        d, q = slice(d0, d0 + nd), slice(g0, g0 + ng)
        assert np.array_equal(got["gt_ig"][q], want["gt_ig"][q]), g    # the ground truths keep their gt_ig
        if nd > 64 or ng > 63:
            assert (got["rank"][d] == -1).all() and (got["dt_match"][d] == -1).all() and (got["dt_ig"][d] == 1).all(), g
        else:
            for k in ("rank", "dt_match", "dt_ig"):
                assert np.array_equal(got[k][d], want[k][d]), (g, k)
    assert sum(nd > 64 or ng > 63 for (_, nd), (_, ng) in zip(dr, gr)) == 2


def test_wrapper_equals_the_raw_call(dev):
    groups, want = _world("4x10")
    dr, gr, po, d0, g0, p0 = [], [], [], 0, 0, 0
    for g in groups:
        nd, ng = len(g["score"]), len(g["gt_area"])
        dr.append((d0, nd)), gr.append((g0, ng)), po.append(p0)
        d0, g0, p0 = d0 + nd, g0 + ng, p0 + nd * ng
    cat = lambda k, t: np.concatenate([np.asarray(g[k], t).reshape(-1) for g in groups])  # noqa: E731
    res = coco.match(cat("score", np.float64), np.array(dr, np.int32), np.array(gr, np.int32), np.array(po, np.int32),
                     cat("iou", np.float64), cat("det_area", np.float64), cat("gt_area", np.float64),
                     cat("gt_flags", np.int32), device=dev)
    _equal({k: v.cpu().numpy() for k, v in res.items()}, want, "wrapper")
    with pytest.raises(ValueError, match="1 <= A <= 8"):
        coco.match([], np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32), [], [], [], [], [], np.zeros((9, 2)), device=dev)
