"""COCO AP without a GPU: hand-worked cases for the numpy restatement (tests/coco_ref.py), coco.accumulate /
coco.summarize against it bit for bit, every host-side refusal of krrn_rle_iou_f64 / krrn_box_iou_f64 /
krrn_coco_match_f64 (made before any HIP call, so the pointers are never dereferenced), their ABI signatures, and the
refusals of rle.iou / rle.box_iou / bop_scene.eval_coco that come before a device is touched."""
import ctypes
import json
import os

import numpy as np
import pytest

import coco_ref as cr
from pose_estimation_amd import _lib, bop_scene, coco, rle

EARG, ESHAPE = -1, -2
N = ctypes.c_void_p(0)


def _bits(x):
    return np.asarray(x, np.float64).tobytes()


# ---------------------------------------------------------------- the restatement, by hand

@pytest.mark.parametrize("name", [c[0] for c in cr.hand_cases()])
def test_hand_worked_matching(name):
    case = next(c for c in cr.hand_cases() if c[0] == name)
    dm, di, gi, rk = cr.evaluate_img(**case[1])
    for (d, a, t), (m, ig) in case[2].get("dt", {}).items():
        assert (dm[d, a, t], di[d, a, t]) == (m, ig), (name, d, a, t, dm[d, a, t], di[d, a, t])
    for (j, a), ig in case[2].get("gt_ig", {}).items():
        assert gi[j, a] == ig, (name, j, a)
    for d, r in case[2].get("rank", {}).items():
        assert rk[d] == r, (name, d, rk[d])


def _groups(cases, cat=0):
    out = []
    for kw in cases:
        dm, di, gi, rk = cr.evaluate_img(**kw)
        out.append({"cat": cat, "score": list(kw["score"]), "rank": rk, "dt_match": dm, "dt_ig": di, "gt_ig": gi})
    return out


def test_ignored_match_is_neither_tp_nor_fp():
    """The better-scored detection matches an ignored ground truth, the other one the only counted ground truth: were
    the first a false positive, precision at recall 1 would be 1/2."""
    kw = dict(score=[0.9, 0.8], iou=[[0.9, 0.0], [0.0, 0.9]], det_area=[2000.0, 2000.0], gt_area=[2000.0, 2000.0],
              gt_flags=[2, 0])
    dm, di, _, _ = cr.evaluate_img(**kw)
    assert (dm[0, 0, 0], di[0, 0, 0], dm[1, 0, 0], di[1, 0, 0]) == (0, 1, 1, 0)
    pr, rc = cr.accumulate(_groups([kw]), 1)
    s = cr.summarize(pr, rc, [7])
    assert s["AP50"] > 0.99 and s["AP75"] > 0.99         # the IoUs are 0.9: AP itself loses the 0.95 threshold
    assert _bits(rc[:, 0, 0, 2]) == _bits([1.0] * 9 + [0.0]) and s["AR1"] == 0.0   # maxDet 1 keeps the ignored match alone


def test_ground_truth_as_detections_scores_one():
    eye = np.eye(2).tolist()
    kw = dict(score=[1.0, 1.0], iou=eye, det_area=[500.0, 20000.0], gt_area=[500.0, 20000.0], gt_flags=[0, 0])
    pr, rc = cr.accumulate(_groups([kw, kw, kw]), 1)
    s = cr.summarize(pr, rc, [1])
    # every sampled precision is k / (k + spacing(1)) >= 1 - spacing(1); the mean adds a few roundings
    assert 0.0 <= 1.0 - s["AP"] <= 8 * np.spacing(1) and 0.0 <= 1.0 - s["AP50"] <= 8 * np.spacing(1)
    assert s["AR100"] == 1.0 and s["AR10"] == 1.0
    assert s["AP_medium"] == -1.0                                       # no ground truth of that size: npig == 0
    assert s["AP_small"] > 0.99 and s["AP_large"] > 0.99


def test_no_counted_ground_truth_gives_minus_one():
    kw = dict(score=[0.5], iou=[[0.9]], det_area=[2000.0], gt_area=[2000.0], gt_flags=[2])
    pr, rc = cr.accumulate(_groups([kw], cat=1), 2)
    assert (pr == -1).all() and (rc == -1).all()
    s = cr.summarize(pr, rc, [3, 4])
    assert s["AP"] == -1.0 and s["AR100"] == -1.0 and s["per_obj"] == {3: {"AP": -1.0, "AR100": -1.0},
                                                                         4: {"AP": -1.0, "AR100": -1.0}}


def _random_groups(seed, n_groups, n_cat):
    rng = np.random.default_rng(seed)
    grid = np.concatenate([cr.IOU_THRS, [0.0, 0.3, 1.0]])
    out = []
    for g in range(n_groups):
        nd, ng = int(rng.integers(0, 9)), int(rng.integers(0, 5))
        kw = dict(score=rng.choice([0.2, 0.5, 0.5, 0.9, 0.95], nd).tolist(), iou=rng.choice(grid, (nd, ng)),
                  det_area=rng.choice([500.0, 1024.0, 5000.0, 20000.0], nd).tolist(),
                  gt_area=rng.choice([500.0, 1024.0, 5000.0, 20000.0], ng).tolist(),
                  gt_flags=rng.choice([0, 0, 0, 1, 2], ng).tolist())
        out += _groups([kw], cat=int(rng.integers(0, n_cat)))
    return out


@pytest.mark.parametrize("seed,n_groups,n_cat", [(0, 12, 3), (1, 1, 1), (2, 40, 2)])
def test_accumulate_equals_the_restatement(seed, n_groups, n_cat):
    """coco.accumulate / summarize on packed arrays against the loop-by-loop restatement, bit for bit (both take the
    means with np.mean over the same values in the same order)."""
    groups = _random_groups(seed, n_groups, n_cat)
    pr, rc = cr.accumulate(groups, n_cat)
    want = cr.summarize(pr, rc, list(range(10, 10 + n_cat)))
    d_rng, g_rng, d0, g0 = [], [], 0, 0
    for g in groups:
        d_rng.append((d0, len(g["score"]))), g_rng.append((g0, g["gt_ig"].shape[0]))
        d0, g0 = d0 + len(g["score"]), g0 + g["gt_ig"].shape[0]
    A, T = len(cr.AREA_RNG), len(cr.IOU_THRS)
    cat = lambda k, shape: np.concatenate([np.asarray(g[k]).reshape(shape) for g in groups])  # noqa: E731
    acc = coco.accumulate([g["cat"] for g in groups], d_rng, g_rng, cat("score", (-1,)), cat("rank", (-1,)),
                          cat("dt_match", (-1, A, T)), cat("dt_ig", (-1, A, T)), cat("gt_ig", (-1, A)), n_cat)
    assert _bits(acc["precision"]) == _bits(pr) and _bits(acc["recall"]) == _bits(rc)
    got = coco.summarize(acc, cats=list(range(10, 10 + n_cat)))
    assert set(got) == set(want)
    for k in want:
        if k == "per_obj":
            assert {c: {m: _bits(v) for m, v in e.items()} for c, e in got[k].items()} == \
                {c: {m: _bits(v) for m, v in e.items()} for c, e in want[k].items()}
        else:
            assert _bits(got[k]) == _bits(want[k]), (k, got[k], want[k])


def test_constants():
    assert _bits(coco.IOU_THRS) == _bits(np.linspace(0.5, 0.95, 10))
    assert coco.AREA_RNG.tolist() == [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
    assert coco.MAX_DETS == (1, 10, 100)


# ---------------------------------------------------------------- the entry points' host checks

def test_abi_lists_the_entry_points():
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.SIGNATURES["krrn_rle_iou_ws"] == [I, P]
    assert _lib.SIGNATURES["krrn_rle_iou_f64"] == [P, I, P, I, P, P, I, P, P, P, P, P]
    assert _lib.SIGNATURES["krrn_box_iou_f64"] == [P, I, P, P, I, P, P, P]
    assert _lib.SIGNATURES["krrn_coco_match_f64"] == [P, I, P, P, P, P, L, P, P, P, I, P, I, P, I, I, I, I, I, P, P, P,
                                                      P, P]


def _fake(names):
    return {k: ctypes.c_void_p((i + 1) << 36) for i, k in enumerate(names)}    # never dereferenced


IOU_PTRS = ("counts", "offs", "pair", "crowd", "ws", "inter", "iou", "area")


def _iou(n=3, P=5, n_counts=12, **over):
    p = dict(_fake(IOU_PTRS), **over)
    return _lib.lib().krrn_rle_iou_f64(p["counts"], n_counts, p["offs"], n, p["pair"], p["crowd"], P, p["ws"],
                                       p["inter"], p["iou"], p["area"], N)


@pytest.mark.parametrize("name", [k for k in IOU_PTRS if k != "crowd"])
def test_rle_iou_null_pointer_is_earg(name):
    assert _iou(**{name: N}) == EARG
    assert _iou(n=-1, **{name: N}) == EARG               # pointers are checked first


def test_rle_iou_shapes_and_empty_call():
    assert _iou(n=-1) == ESHAPE and _iou(P=-1) == ESHAPE and _iou(n_counts=-1) == ESHAPE
    assert _iou(n=0, P=0) == 0 and _iou(n=0, P=0, crowd=N) == 0         # launches nothing
    fn = _lib.lib().krrn_rle_iou_ws
    out = ctypes.c_longlong(-1)
    assert fn(5, N) == EARG
    assert fn(-1, ctypes.byref(out)) == ESHAPE and out.value == -1
    assert fn(0, ctypes.byref(out)) == 0 and out.value == 0
    assert fn(0x7fffffff, ctypes.byref(out)) == 0 and out.value == 2 * 0x7fffffff          # past 2^31: no wrap


BOX_PTRS = ("box", "pair", "crowd", "iou", "area")


def _box(n=3, P=5, **over):
    p = dict(_fake(BOX_PTRS), **over)
    return _lib.lib().krrn_box_iou_f64(p["box"], n, p["pair"], p["crowd"], P, p["iou"], p["area"], N)


def test_box_iou_host_checks():
    for name in BOX_PTRS:
        if name != "crowd":
            assert _box(**{name: N}) == EARG and _box(n=-1, **{name: N}) == EARG
    assert _box(n=-1) == ESHAPE and _box(P=-1) == ESHAPE
    assert _box(n=0, P=0) == 0 and _box(n=0, P=0, crowd=N) == 0


MATCH_PTRS = ("score", "det_range", "gt_range", "pair_off", "iou", "det_area", "gt_area", "gt_flags", "area_rng",
              "iou_thr", "dt_match", "dt_ig", "gt_ig", "rank")


def _match(Dtot=4, Ptot=6, GTtot=3, A=4, T=10, max_det=100, lim_det=128, lim_gt=128, G=2, **over):
    p = dict(_fake(MATCH_PTRS), **over)
    return _lib.lib().krrn_coco_match_f64(p["score"], Dtot, p["det_range"], p["gt_range"], p["pair_off"], p["iou"],
                                          Ptot, p["det_area"], p["gt_area"], p["gt_flags"], GTtot, p["area_rng"], A,
                                          p["iou_thr"], T, max_det, lim_det, lim_gt, G, p["dt_match"], p["dt_ig"],
                                          p["gt_ig"], p["rank"], N)


@pytest.mark.parametrize("name", MATCH_PTRS)
def test_coco_match_null_pointer_is_earg(name):
    assert _match(**{name: N}) == EARG
    assert _match(G=-1, **{name: N}) == EARG             # pointers are checked first


def test_coco_match_optional_pointers_follow_their_extents():
    none_d = {k: N for k in ("score", "det_area", "dt_match", "dt_ig", "rank")}
    none_g = {k: N for k in ("gt_area", "gt_flags", "gt_ig")}
    assert _match(G=0, Dtot=0, Ptot=0, **none_d, iou=N) == 0
    assert _match(G=0, GTtot=0, Ptot=0, **none_g, iou=N) == 0
    assert _match(G=0, Dtot=0, **none_d, iou=N) == EARG                 # Ptot > 0 still needs iou


@pytest.mark.parametrize("bad", [dict(G=-1), dict(Dtot=-1), dict(GTtot=-1), dict(Ptot=-1), dict(Ptot=2 ** 31),
                                 dict(A=0), dict(A=9), dict(T=0), dict(T=17), dict(max_det=-1), dict(max_det=129),
                                 dict(lim_det=-1), dict(lim_det=129), dict(lim_gt=-1), dict(lim_gt=129)])
def test_coco_match_bad_shape_is_eshape(bad):
    assert _match(**bad) == ESHAPE
    assert _match(**dict(dict(G=0), **bad)) == ESHAPE    # shapes are checked before the G == 0 return


def test_coco_match_no_group_returns_ok_without_a_launch():
    assert _match(G=0) == 0 and _match(G=0, A=8, T=16, max_det=128) == 0 and _match(G=0, max_det=0) == 0


# ---------------------------------------------------------------- the wrappers' refusals

def test_rle_iou_validates_on_the_host():
    ok = dict(counts=[3, 2, 30, 35], offs=[0, 3, 4], pair=[[0, 1]])
    with pytest.raises(RuntimeError, match="HIP path only"):
        rle.iou(**ok, device="cpu")                      # every check passed: no host fallback
    with pytest.raises(ValueError, match="mask 1 has no run"):
        rle.iou([3, 2, 30], [0, 3, 3], [[0, 1]], device="cpu")
    with pytest.raises(ValueError, match="mask 0 has a negative count"):
        rle.iou([3, -2, 34, 35], [0, 3, 4], [[0, 1]], device="cpu")
    with pytest.raises(ValueError, match="mask 1.*does not fit an int32"):
        rle.iou([35, 2 ** 30, 2 ** 30], [0, 1, 3], [], device="cpu")
    with pytest.raises(ValueError, match="pair 1: mask 0 has 35 pixels and mask 1 36"):
        rle.iou([3, 2, 30, 36], [0, 3, 4], [[0, 0], [0, 1]], device="cpu")
    with pytest.raises(ValueError, match="mask 0.*lie outside"):
        rle.iou([3, 2], [0, 3], [], device="cpu")
    with pytest.raises(ValueError, match="crowd must hold one flag per pair"):
        rle.iou(**ok, crowd=[0, 1], device="cpu")
    with pytest.raises(ValueError, match=r"\[n, 4\]"):
        rle.box_iou([[0, 0, 1]], [], device="cpu")
    with pytest.raises(RuntimeError, match="HIP path only"):
        rle.box_iou([[0, 0, 1, 1]], [[0, 0]], device="cpu")


def _coco_dict(n_ann=1, H=5, W=7):
    ann = [{"id": i + 1, "image_id": 0, "category_id": 1, "iscrowd": 0, "area": 2, "bbox": [0, 0, 1, 1],
            "segmentation": {"counts": [3, 2, H * W - 5], "size": [H, W]}, "ignore": False} for i in range(n_ann)]
    return {"images": [{"id": 0, "file_name": "rgb/000000.png", "width": W, "height": H}], "annotations": ann,
            "categories": [{"id": 1, "name": "1"}]}


def test_eval_coco_refusals(tmp_path):
    row = {"scene_id": 1, "image_id": 0, "category_id": 1, "score": 1.0, "bbox": [0.0, 0.0, 1.0, 1.0]}
    seg = lambda H, W: dict(row, segmentation={"counts": [H * W], "size": [H, W]})  # noqa: E731
    gt = {1: _coco_dict()}
    with pytest.raises(ValueError, match="iou_type"):
        bop_scene.eval_coco(gt, [row], "cuda:0", iou_type="keypoints")
    with pytest.raises(ValueError, match="row 1 has no segmentation"):
        bop_scene.eval_coco(gt, [seg(5, 7), row], "cuda:0")
    with pytest.raises(ValueError, match="row 0: segmentation.size"):
        bop_scene.eval_coco(gt, [seg(7, 5)], "cuda:0")
    with pytest.raises(ValueError, match="129 ground truths > 128"):
        bop_scene.eval_coco({1: _coco_dict(129)}, [], "cuda:0", iou_type="bbox")
    with pytest.raises(ValueError, match=r"\(root, split\)"):
        bop_scene.eval_coco("nowhere", [], "cuda:0")
    os.makedirs(tmp_path / "test" / "000001")
    os.makedirs(tmp_path / "test" / "000002")
    with open(tmp_path / "test" / "000001" / "scene_gt_coco.json", "w") as f:
        json.dump(_coco_dict(), f)
    with pytest.raises(FileNotFoundError, match="000002.*scene_gt_coco.json.*write_gt_coco"):
        bop_scene.eval_coco((str(tmp_path), "test"), [], "cuda:0")
