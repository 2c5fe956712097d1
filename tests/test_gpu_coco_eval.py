"""bop_scene.eval_coco on the synthetic BOP trees of tests/bop_tree.py and tests/bop_multi_tree.py: every returned
number against tests/coco_ref.py's eval_rows on the same rows (mask IoU through decoded planes, the matching and the
accumulation loop by loop), bit for bit, and evaluate.test_epoch(seg_json=..., coco=True)."""
import copy

import numpy as np
import pytest
import torch

import bop_multi_tree as mt
import bop_tree
import coco_ref as cr
import rle_ref as rf
from pose_estimation_amd import bop_scene, rle
from pose_estimation_amd.dataset import PoseDataset
from pose_estimation_amd.evaluate import test_epoch as run_epoch

pytestmark = pytest.mark.gpu


def _ds(root, **kw):
    return PoseDataset("test", 500, False, root, 0.0, 8, n_model_pts=4, layout="bop", meshes=True, **kw)


def _same(a, b, path=""):
    """Bitwise equality of nested dicts of tensors / floats / anything comparable."""
    if isinstance(a, dict):
        assert set(a) == set(b), (path, set(a) ^ set(b))
        for k in a:
            _same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
    elif isinstance(a, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), (path, a, b)
    else:
        assert a == b, (path, a, b)


def _rows(tree):
    """The tree's ground truth as detections with falling scores, plus a lower-scored duplicate of the first row, the
    second row's mask shifted by three columns, a row of a category and one of an image the tree does not hold."""
    rows = bop_scene.gt_detections(tree)
    for i, r in enumerate(rows):
        r["score"] = 0.95 - 0.05 * (i % 7)
    dup = copy.deepcopy(rows[0])
    dup["score"] = 0.4
    moved = copy.deepcopy(rows[1])
    H, W = moved["segmentation"]["size"]
    plane = np.roll(rf.decode(moved["segmentation"]["counts"], H, W), 3, axis=1)
    moved.update(score=0.97, segmentation={"counts": rle.encode(plane), "size": [H, W]},
                 bbox=[moved["bbox"][0] + 3.0] + moved["bbox"][1:])
    alien = dict(copy.deepcopy(rows[0]), category_id=99)
    nowhere = dict(copy.deepcopy(rows[0]), image_id=12345)
    return bop_scene._check_rows(rows[:2] + [dup, alien] + rows[2:] + [moved, nowhere], "rows")


@pytest.mark.parametrize("which", ["multi", "tiny"])
def test_eval_coco_equals_the_restatement(dev, tmp_path, which):
    root = str(tmp_path / "tree")
    (mt if which == "multi" else bop_tree).write_tree(root)
    gts = bop_scene.write_gt_coco(root, "test", dev, min_visib=0.1 if which == "multi" else 0.75)
    rows = _rows(_ds(root).tree)
    marked = copy.deepcopy(gts)                          # the same ground truth with an ignored and a crowd annotation
    first = marked[sorted(marked)[0]]["annotations"]
    first[0]["ignore"], first[-1]["iscrowd"] = True, 1
    n_ann = sum(len(c["annotations"]) for c in gts.values())
    for name, gt in (("written", gts), ("marked", marked)):
        for iou_type in ("segm", "bbox"):
            for use_ignore in (True, False):
                got = bop_scene.eval_coco(gt, rows, dev, iou_type, use_ignore)
                want = cr.eval_rows(gt, rows, iou_type, use_ignore)
                print(which, name, iou_type, use_ignore, {k: v for k, v in got.items() if k != "per_obj"})
                _same(got, want, f"{which}/{name}/{iou_type}/{use_ignore}")
                assert got["ignored"] == 2 and got["count"] == len(rows) - 2 and got["targets"] == n_ann
                assert set(got) == {"AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "AR100",
                                    "per_obj", "count", "targets", "ignored"}
                # the kept instances' ground truth as detections: something is found (the tiny tree keeps 5 of 8)
                assert 0.0 < got["AP50"] <= 1.0 and 0.0 < got["AR100"] <= 1.0
    whole = bop_scene.eval_coco(marked, rows, dev, "segm")
    _same(bop_scene.eval_coco(marked, rows, dev, "segm", chunk_images=1), whole, "chunks")
    _same(bop_scene.eval_coco((root, "test"), rows, dev, "segm"), bop_scene.eval_coco(gts, rows, dev, "segm"), "files")
    none = bop_scene.eval_coco(gts, [], dev, "bbox")     # no detection at all: recall 0 everywhere a ground truth counts
    assert none["count"] == 0 and none["AR100"] == 0.0 and none["AP"] == 0.0


def _model(dev, num_cls):
    from pose_estimation_amd import KRRN, make_config
    from pose_estimation_amd.synthetic import init_weights
    m = KRRN(cfg=make_config(num_cls=num_cls, backbone="w18"))
    init_weights(m, 0)
    return m.to(dev).eval()


def _reset():
    from pose_estimation_amd import pose as kpose
    torch.manual_seed(5)
    kpose._seeds.clear()


def test_epoch_scores_its_segmentation_file(dev, tmp_path):
    """test_epoch(seg_json=..., coco=True) adds exactly "coco", which is eval_coco of the file read back; every other
    key is bitwise what the run without it gives."""
    root = str(tmp_path / "tree")
    bop_tree.write_tree(root)
    bop_scene.write_gt_coco(root, "test", dev)
    m = _model(dev, 3)
    a, b = str(tmp_path / "a_seg.json"), str(tmp_path / "b_seg.json")
    _reset()
    plain = run_epoch(m, _ds(root), bs=3, device=dev, seg_json=a)
    _reset()
    out = run_epoch(m, _ds(root), bs=3, device=dev, seg_json=b, coco=True)
    assert set(out) - set(plain) == {"coco"}
    _same({k: v for k, v in out.items() if k != "coco"}, plain)
    det = bop_scene.read_detections(b)
    assert det == bop_scene.read_detections(a) and len(det) >= 1
    _same(out["coco"], bop_scene.eval_coco((root, "test"), det, dev, "segm"))
    _same(out["coco"], cr.eval_rows(bop_scene._coco_gt((root, "test")), det, "segm"))
    print("coco:", {k: v for k, v in out["coco"].items() if k != "per_obj"})
    assert out["coco"]["count"] == len(det) and out["coco"]["ignored"] == 0
    c = str(tmp_path / "c_seg.json")                     # the network's own masks are scored the same way
    _reset()
    net = run_epoch(m, _ds(root), bs=3, device=dev, seg_json=c, seg_source="net", coco=True)
    assert set(net) - set(plain) == {"coco"}
    _same(net["coco"], bop_scene.eval_coco((root, "test"), bop_scene.read_detections(c), dev, "segm"))
    assert net["coco"]["count"] == net["seg"]["rows"]
    with pytest.raises(ValueError, match="coco=True.*seg_json"):
        run_epoch(torch.nn.Linear(1, 1), _ds(root), bs=3, device=dev, coco=True)
