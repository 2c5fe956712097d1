"""The eval path's shared host code without a GPU: which detection rows BopTree pairs with which kept target in both
det_per_target modes (ties, det_min_score, the three kinds of dropped row, rows for no kept target, a target short of
rows, NaN scores), evaluate.EpochTables' legacy return for every combination of tables, and the operand checks that
bop.stage_scene makes for vsd, visibility, verify.score_poses and depth_refine.refine.

The pairing's expected values are written out by hand from BopTree's class docstring and the trees' own files (the
boxes below are the bbox_visib entries that tests/bop_tree.py and tests/bop_multi_tree.py write)."""
import itertools
import math

import pytest
import torch

import bop_multi_tree
import bop_tree
from pose_estimation_amd import bop, bop_scene, depth_refine, verify
from pose_estimation_amd.evaluate import POSE_REC, REC, SEL_REC, EpochTables

H, W = 48, 64
NAN = float("nan")


def _row(scene, im, obj, score, bbox, counts=None):
    r = {"scene_id": scene, "image_id": im, "category_id": obj, "score": score, "bbox": list(bbox)}
    if counts is not None:
        r["segmentation"] = {"counts": counts, "size": [H, W]}
    return r


def _items(t):
    return [(it["scene"], it["im"], it["obj"], it["gt"], it["det"], it["score"], it["bbox"]) for it in t.items]


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    """tests/bop_tree.py: the kept instances are, in order, (scene, image, object) gt index
    (1, 3, 3) 0, (1, 3, 2) 1, (1, 7, 3) 0, (1, 7, 1) 2, (2, 0, 3) 1: one instance per target."""
    root = str(tmp_path_factory.mktemp("pair_single"))
    bop_tree.write_tree(root)
    return root


@pytest.fixture(scope="module")
def multi(tmp_path_factory):
    """tests/bop_multi_tree.py with its targets file: (1, 0, 2) inst_count 3 (gt 0, 2, 4), (1, 0, 3) inst_count 2
    (gt 1, 3), (1, 1, 3) and (1, 1, 1) inst_count 1 (gt 0 and 1)."""
    root = str(tmp_path_factory.mktemp("pair_multi"))
    return root, bop_multi_tree.write_tree(root)["targets"]


@pytest.mark.parametrize("mode", ["best", "inst_count"])
def test_pairing_one_instance_per_target(single, mode):
    """Every target holds one instance and inst_count is 1, so both modes must pair the same rows."""
    rows = [_row(1, 3, 3, 0.6, [23, 15, 15, 15]),                 # 0  used: the earlier row of the tie with row 1
            _row(1, 3, 3, 0.6, [20, 12, 18, 18]),                 # 1  unused
            _row(1, 3, 2, 0.05, [35, 23, 7, 8]),                  # 2  below det_min_score: unused
            _row(1, 3, 2, 0.3, [34, 22, 9, 9]),                   # 3  used
            _row(1, 7, 3, 0.9, [0, 0, 0, 13]),                    # 4  w = 0: dropped
            _row(1, 7, 3, 0.9, [0, 0, 12, -1]),                   # 5  h < 0: dropped
            _row(1, 7, 3, 0.9, [0, 0, 12, 13], [H * W]),          # 6  no set pixel: dropped, so (1, 7, 3) is missed
            _row(1, 7, 9, 0.8, [1, 1, 5, 5]),                     # 7  object 9 is no kept target: unused
            _row(1, 7, 1, 0.5, [33, 22, 16, 16])]                 # 8  used; nothing for (2, 0, 3): missed
    t = bop_scene.BopTree(single, n_model_pts=4, detections=rows, det_min_score=0.1, det_per_target=mode)
    assert _items(t) == [(1, 3, 3, 0, 0, 0.6, [23.0, 15.0, 15.0, 15.0]), (1, 3, 2, 1, 3, 0.3, [34.0, 22.0, 9.0, 9.0]),
                         (1, 7, 1, 2, 8, 0.5, [33.0, 22.0, 16.0, 16.0])]
    assert t.missed == [(1, 7, 3), (2, 0, 3)]
    assert t.det_stats == {"rows": 9, "used": 3, "unused": 3, "dropped": 3}


def test_pairing_inst_count(multi):
    root, targets = multi
    rows = [_row(1, 0, 2, 0.7, [28, 7, 9, 10]),                   # 0  rank 2 of (1, 0, 2): gt 2's own box
            _row(1, 0, 2, 0.9, [50, 7, 9, 9]),                    # 1  rank 1: gt 4's own box
            _row(1, 0, 2, 0.7, [60, 44, 2, 2]),                   # 2  rank 3, after row 0 of the same score; the box
                                                                  #    overlaps no instance: IoU 0 thrice, lowest gt = 0
            _row(1, 0, 2, 0.2, [5, 7, 10, 9]),                    # 3  a fourth row for inst_count 3: unused
            _row(1, 0, 3, 0.05, [14, 29, 11, 11]),                # 4  below det_min_score: unused
            _row(1, 0, 3, 0.8, [42, 28, 11, 11]),                 # 5  the only row of (1, 0, 3) that qualifies: gt 3's box
            _row(1, 0, 3, 0.95, [14, 29, 0, 11]),                 # 6  w = 0: dropped
            _row(1, 0, 3, 0.95, [14, 29, 11, 0]),                 # 7  h = 0: dropped
            _row(1, 0, 3, 0.95, [14, 29, 11, 11], [H * W]),       # 8  no set pixel: dropped
            _row(1, 0, 7, 0.9, [1, 1, 5, 5]),                     # 9  object 7 is no kept target: unused
            _row(1, 1, 1, 0.6, [0, 0, 1, 1])]                     # 10 (1, 1, 1)'s sole instance; nothing for (1, 1, 3)
    t = bop_scene.BopTree(root, n_model_pts=4, targets=targets, detections=rows, det_min_score=0.1,
                          det_per_target="inst_count")
    # target by target in the order of `instances`, each target's rows by rank
    assert _items(t) == [(1, 0, 2, 4, 1, 0.9, [50.0, 7.0, 9.0, 9.0]), (1, 0, 2, 2, 0, 0.7, [28.0, 7.0, 9.0, 10.0]),
                         (1, 0, 2, 0, 2, 0.7, [60.0, 44.0, 2.0, 2.0]), (1, 0, 3, 3, 5, 0.8, [42.0, 28.0, 11.0, 11.0]),
                         (1, 1, 1, 1, 10, 0.6, [0.0, 0.0, 1.0, 1.0])]
    assert t.missed == [(1, 0, 3), (1, 1, 3)]                     # one estimate short each: 5 items + 2 = 3 + 2 + 1 + 1
    assert t.det_stats == {"rows": 11, "used": 5, "unused": 3, "dropped": 3}
    with pytest.raises(ValueError, match=r"scene 1, image 0, object 2.*inst_count > 1"):
        bop_scene.BopTree(root, n_model_pts=4, targets=targets, detections=rows, det_min_score=0.1)


def test_pairing_nan_scores(single):
    """What a NaN score has meant since each mode was written, kept as it is. "best" scanned the rows with
    `score < det_min_score` to skip and a strict `>` to replace, and NaN compares false both ways: a NaN row qualifies,
    is never displaced when it is its target's first qualifying row, and is never picked otherwise. "inst_count" asks
    for `score >= det_min_score`, which a NaN never meets: the row stays unused."""
    box = [33, 22, 16, 16]
    pair = lambda rows, mode: bop_scene.BopTree(single, n_model_pts=4, objlist=[1], detections=rows,  # noqa: E731
                                                 det_min_score=0.1, det_per_target=mode)
    first = [_row(1, 7, 1, NAN, box), _row(1, 7, 1, 0.5, box)]
    t = pair(first, "best")
    assert [it["det"] for it in t.items] == [0] and math.isnan(t.items[0]["score"]) and t.missed == []
    assert t.det_stats == {"rows": 2, "used": 1, "unused": 1, "dropped": 0}
    t = pair(first, "inst_count")
    assert [(it["det"], it["score"]) for it in t.items] == [(1, 0.5)] and t.missed == []
    later = [_row(1, 7, 1, 0.5, box), _row(1, 7, 1, NAN, box), _row(1, 7, 1, 0.4, box)]
    for mode in ("best", "inst_count"):
        t = pair(later, mode)
        assert [(it["det"], it["score"]) for it in t.items] == [(0, 0.5)], mode
        assert t.det_stats == {"rows": 3, "used": 1, "unused": 2, "dropped": 0}
    t = pair([_row(1, 7, 1, NAN, box)], "best")
    assert [it["det"] for it in t.items] == [0] and t.missed == []
    t = pair([_row(1, 7, 1, NAN, box)], "inst_count")
    assert t.items == [] and t.missed == [(1, 7, 1)] and t.det_stats == {"rows": 1, "used": 0, "unused": 1, "dropped": 0}


@pytest.mark.parametrize("n", [0, 2])
@pytest.mark.parametrize("with_bop, with_poses, with_sel", list(itertools.product([False, True], repeat=3)))
def test_epoch_tables_legacy_return(n, with_bop, with_poses, with_sel):
    tab = lambda cols, fill: torch.full((n, len(cols)), fill, dtype=torch.float64)  # noqa: E731
    rec, brec, prec, srec = tab(REC, 1.0), tab(bop.BOP_REC, 2.0), tab(POSE_REC, 3.0), tab(SEL_REC, 4.0)
    bundle = EpochTables(rec, brec if with_bop else None, prec if with_poses else None, srec if with_sel else None)
    assert bundle._fields == ("rec", "bop", "poses", "sel")
    out = bundle.legacy()
    want = [rec] + [t for t, on in ((brec, with_bop), (prec, with_poses), (srec, with_sel)) if on]
    if len(want) == 1:
        assert out is rec                                         # the bare case: a lone tensor, not a tuple of one
    else:
        assert isinstance(out, tuple) and len(out) == len(want) and all(a is b for a, b in zip(out, want))
    widths = [len(REC)] + [len(bop.BOP_REC)] * with_bop + [len(POSE_REC)] * with_poses + [len(SEL_REC)] * with_sel
    assert [tuple(t.shape) for t in (out if isinstance(out, tuple) else (out,))] == [(n, w) for w in widths]
    assert EpochTables.of(out, with_bop, with_poses, with_sel) == bundle     # test_epoch's way back, by field name


@pytest.mark.parametrize("extra", ["plain", "net_masks", "zoom"])
@pytest.mark.parametrize("with_bop, with_poses, with_sel", list(itertools.product([False, True], repeat=3)))
def test_eval_records_return_shape(monkeypatch, extra, with_bop, with_poses, with_sel):
    """eval_records' documented return over a stubbed epoch: the tables that were asked for in the order rec, bop,
    poses, sel, rec alone as a lone tensor, and the net_masks run list or the zoom status array last."""
    from pose_estimation_amd import evaluate
    tab = lambda cols, fill: torch.full((2, len(cols)), fill, dtype=torch.float64)  # noqa: E731
    rec, brec, prec, srec = tab(REC, 1.0), tab(bop.BOP_REC, 2.0), tab(POSE_REC, 3.0), tab(SEL_REC, 4.0)
    runs, zstat = [(0, [3, 1], [0] * 5), (1, [4], [0] * 5)], torch.zeros(2, dtype=torch.int64).numpy()
    seen = []

    def stub(model, dataset, indices, bs, device, opt_pose, with_loss, pose_solver, refine, bop, poses, select,
             net_masks, zoom):
        seen.append((bop, poses, select, net_masks, zoom))
        return (EpochTables(rec, brec if bop else None, prec if poses else None, srec if select else None),
                runs if net_masks else None, zstat if zoom else None)

    monkeypatch.setattr(evaluate, "_eval_epoch", stub)
    out = evaluate.eval_records(None, None, {}, 2, "cpu", bop=with_bop, poses=with_poses,
                                select="depth" if with_sel else None, net_masks=extra == "net_masks",
                                zoom=1 if extra == "zoom" else 0)
    assert seen == [(with_bop, with_poses, "depth" if with_sel else None, extra == "net_masks", int(extra == "zoom"))]
    want = [rec] + [t for t, on in ((brec, with_bop), (prec, with_poses), (srec, with_sel)) if on]
    want += {"plain": [], "net_masks": [runs], "zoom": [zstat]}[extra]
    if len(want) == 1:
        assert out is rec                                         # the bare case: a lone tensor, not a tuple of one
    else:
        assert isinstance(out, tuple) and len(out) == len(want) and all(a is b for a, b in zip(out, want))


class _OnGpu(torch.Tensor):
    """A host tensor that claims to be on the GPU: the operand checks come before anything touches a device."""
    is_cuda = True


def _g(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype).as_subclass(_OnGpu)


def _wrappers(verts, depth, mask):
    """The four render-versus-depth entry points on B = 1 (name, whether it takes a mask, the call)."""
    z = torch.zeros
    faces, fr, K4, frame = _g(1, 3, dtype=torch.int32), z(1, 2, dtype=torch.int32), z(1, 4), z(1, dtype=torch.int32)
    R, t = z(1, 3, 3, dtype=torch.float64), z(1, 3, dtype=torch.float64)
    return [("vsd", False, lambda: bop.vsd(verts, faces, fr, R, t, R, t, K4, depth, frame, z(1))),
            ("visibility", False, lambda: bop.visibility(verts, faces, fr, R, t, K4, depth, frame)),
            ("score_poses", True, lambda: verify.score_poses(verts, faces, fr, R[:, None], t[:, None], K4, depth, frame,
                                                             mask=mask)),
            ("depth_refine.refine", True, lambda: depth_refine.refine(verts, faces, fr, R, t, K4, depth, frame, 0.01, 0.05,
                                                                      mask=mask))]


def test_scene_operand_checks_through_each_wrapper():
    for name, masked, call in _wrappers(torch.zeros(4, 3), _g(1, 8, 8), None):          # verts on the host
        text = f"{name} runs on the HIP path only \\(verts / faces / depth{' / mask' if masked else ''} must be GPU tensors\\)"
        with pytest.raises(RuntimeError, match=text):
            call()
    for name, masked, call in _wrappers(_g(4, 3), _g(1, 8, 8), torch.zeros(1, 8, 8, dtype=torch.uint8)):   # a host mask
        if masked:
            with pytest.raises(RuntimeError, match=f"{name} runs on the HIP path only .* / mask must be GPU tensors"):
                call()
    for name, _, call in _wrappers(_g(4, 3), _g(8, 8), None):                           # a single frame without its axis
        with pytest.raises(ValueError, match=r"depth must be \[F, H, W\], got \(8, 8\)"):
            call()
    for bad, text in ((_g(1, 8, 8, dtype=torch.int32), r"mask must be uint8 \(1, 8, 8\), got torch.int32 \(1, 8, 8\)"),
                      (_g(1, 8, 4, dtype=torch.uint8), r"mask must be uint8 \(1, 8, 8\), got torch.uint8 \(1, 8, 4\)")):
        for name, masked, call in _wrappers(_g(4, 3), _g(1, 8, 8), bad):
            if masked:
                with pytest.raises(ValueError, match=text):
                    call()


def test_per_crop_staging_checks():
    with pytest.raises(ValueError, match=r"max_dist must be a float or a \[B\] tensor with B = 3, got \(2,\)"):
        bop.per_crop(torch.zeros(2), 3, "cpu", "max_dist")
    assert bop.per_crop(0.25, 3, "cpu", "tau").tolist() == [0.25] * 3 and bop.per_crop(0.25, 3, "cpu", "tau").dtype == torch.float64
    assert bop.per_crop(torch.tensor([[1], [2]], dtype=torch.float32), 2, "cpu", "tau").tolist() == [1.0, 2.0]
