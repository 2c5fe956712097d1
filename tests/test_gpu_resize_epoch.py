"""An epoch over a dataset built with resize: mixed source sides run as one bucket through one plan, a dataset whose
sides already equal T gives the records it gives without resize, and a BOP tree with detections writes its CSV."""
import csv

import numpy as np
import pytest
import torch

import bop_tree
from pose_estimation_amd import KRRN, bop_scene, make_config
from pose_estimation_amd import pose as kpose
from pose_estimation_amd.dataset import BucketBatcher, PoseDataset
from pose_estimation_amd.evaluate import eval_records
from pose_estimation_amd.evaluate import test_epoch as run_epoch
from pose_estimation_amd.synthetic import init_weights

pytestmark = pytest.mark.gpu


def _model(dev, num_cls):
    m = KRRN(cfg=make_config(num_cls=num_cls, backbone="w18"))
    init_weights(m, 0)
    return m.to(dev).eval()


def _reset():
    torch.manual_seed(5)
    kpose._seeds.clear()


def _ds(sizes, **kw):
    return PoseDataset("test", 500, False, None, 0.0, 8, cls_type="all", num_frames=12, sizes=sizes, **kw)


@pytest.fixture(scope="module")
def model(dev):
    return _model(dev, 13)


def test_mixed_sides_run_as_one_bucket_through_one_plan(dev, model):
    ds = _ds([80, 120, 160], resize=80)
    assert sorted({b[1] - b[0] for b in ds.boxes}) == [80, 120, 160] and len(BucketBatcher(ds, bs=4)) == 3
    model.invalidate_plans()
    res = run_epoch(model, ds, bs=4, device=dev)
    assert res["test_count"] == 12 and sum(res["all_num"].values()) == 12
    assert [k[:2] for k in model._plans] == [(4, 80)], list(model._plans)
    # the same frames at their own sizes: three buckets of four, a plan each
    model.invalidate_plans()
    res = run_epoch(model, _ds([80, 120, 160]), bs=4, device=dev)
    assert res["test_count"] == 12 and sorted(k[:2] for k in model._plans) == [(4, 80), (4, 120), (4, 160)]
    model.invalidate_plans()


def test_identity_end_to_end(dev, model):
    """Every side is 80 already: the epoch's record table with resize=80 equals the one without, bit for bit."""
    tabs = []
    for kw in ({}, {"resize": 80}):
        ds = _ds([80], **kw)
        _reset()
        tabs.append(eval_records(model, ds, {80: list(range(len(ds)))}, 4, dev, with_loss=False).numpy())
    assert tabs[0].shape[0] == 12 and np.array_equal(tabs[0], tabs[1])
    d = _ds([80], resize=80).batch([0, 1, 2], dev)
    assert d["point_mask"].shape == (3, 1, 80, 80) and d["resize_scale"].tolist() == [1.0, 1.0, 1.0]
    assert d["resize_intrinsic"].shape == (3, 4) and d["resize_intrinsic"].dtype == torch.float32


def test_bop_tree_with_detections_writes_its_csv(dev, tmp_path):
    """layout="bop" with detections and resize=80 (the tree's windows are 40 wide: enlarged 2x): one CSV row per
    item, and the batch's bbox stays the source window."""
    root = str(tmp_path / "tree")
    bop_tree.write_tree(root)
    kw = dict(n_model_pts=4, layout="bop")
    rows = bop_scene.gt_detections(PoseDataset("test", 500, False, root, 0.0, 8, **kw).tree)
    ds = PoseDataset("test", 500, False, root, 0.0, 8, detections=rows, resize=80, **kw)
    assert len(ds) == 5 and {ds.crop_size(i) for i in range(5)} == {80}
    d = ds.batch([0, 1, 2, 3, 4], dev)
    assert d["img_croped"].shape == (5, 3, 80, 80) and d["bbox"].cpu().tolist() == [list(map(float, b)) for b in ds.boxes]
    assert d["resize_scale"].tolist() == [0.5] * 5 and int(d["mask_count"].min()) > 0
    out = str(tmp_path / "res.csv")
    res = run_epoch(_model(dev, len(ds.objlist)), ds, bs=3, device=dev, bop_csv=out)
    assert res["test_count"] == 5
    with open(out) as fh:
        got = list(csv.reader(fh))
    assert len(got) == 1 + 5 and got[0][0] == "scene_id"
