"""The zoom-in pass in the eval epoch: zoom=0 is the epoch it was, bit for bit; zoom=1 runs every crop through the same
single plan twice and reports what became of each window; one batch driven by hand reproduces the epoch's pose rows;
zoom=2 runs. Nothing here is about accuracy: the weights are init_weights', and whether a second pass helps is
unmeasured."""
import numpy as np
import pytest
import torch

from pose_estimation_amd import KRRN, get_pose, make_config
from pose_estimation_amd import pose as kpose
from pose_estimation_amd.dataset import PoseDataset
from pose_estimation_amd.evaluate import EpochTables, eval_records
from pose_estimation_amd.evaluate import test_epoch as run_epoch
from pose_estimation_amd.synthetic import init_weights

pytestmark = pytest.mark.gpu


def _reset():
    torch.manual_seed(5)
    kpose._seeds.clear()


def _ds(num_frames=12):
    return PoseDataset("test", 500, False, None, 0.0, 8, cls_type="all", num_frames=num_frames, sizes=[80, 120, 160],
                       resize=80)


@pytest.fixture(scope="module")
def model(dev):
    m = KRRN(cfg=make_config(num_cls=13, backbone="w18"))
    init_weights(m, 0)
    return m.to(dev).eval()


def test_zoom_0_is_the_call_without_the_argument(dev, model):
    tabs = []
    for kw in ({}, {"zoom": 0}):
        ds = _ds()
        _reset()
        tabs.append(eval_records(model, ds, {80: list(range(len(ds)))}, 4, dev, with_loss=False, poses=True, **kw))
    assert isinstance(tabs[1], tuple) and len(tabs[0]) == len(tabs[1]) == 2
    for a, b in zip(tabs[0], tabs[1]):
        assert a.shape[0] == 12 and np.array_equal(a.numpy().view(np.uint64), b.numpy().view(np.uint64))


def test_zoom_1_epoch(dev, model):
    """`passes` is 1 and the three status counts account for all 12 crops."""
    ds = _ds()
    model.invalidate_plans()
    _reset()
    res = run_epoch(model, ds, bs=4, device=dev, zoom=1)
    assert res["test_count"] == 12 and sum(res["all_num"].values()) == 12
    z = res["zoom"]
    assert sorted(z) == ["kept_bad_pose", "kept_outside", "passes", "recropped"] and z["passes"] == 1
    assert z["recropped"] + z["kept_bad_pose"] + z["kept_outside"] == 12
    assert all(isinstance(v, int) and v >= 0 for v in z.values())
    assert [k[:2] for k in model._plans] == [(4, 80)], list(model._plans)
    _reset()
    out = eval_records(model, _ds(), {80: list(range(12))}, 4, dev, with_loss=False, zoom=1)
    rec, zstat = out
    assert rec.shape[0] == 12 and (rec[:, -1] == 1.0).all()  # every record is marked valid
    assert zstat.shape == (12,) and zstat.dtype == np.int64 and set(zstat.tolist()) <= {0, 1, 2}
    assert [int((zstat == s).sum()) for s in (0, 1, 2)] == [z["recropped"], z["kept_bad_pose"], z["kept_outside"]]
    model.invalidate_plans()


def test_one_batch_by_hand_reproduces_the_epoch_s_pose_rows(dev, model):
    """A one-batch epoch, so the host draws come in the same order on both sides: batch(zoom=True) -> model ->
    get_pose -> zoom_batch -> model -> get_pose."""
    idx = [0, 1, 2, 3]
    _reset()
    out = eval_records(model, _ds(4), {80: idx}, 4, dev, with_loss=False, poses=True, zoom=1)
    tabs, zstat = EpochTables.of(out[:-1], False, True, False), out[-1]
    assert tabs.poses.shape == (4, 13)
    ds = _ds(4)
    _reset()
    data = ds.batch(idx, dev, zoom=True)
    pred = model(data["img_croped"], data["cloud"], data["choose"], data["cls_id"], opt_pose=True)
    R1, _ = get_pose({"xyz": pred["xyz"].clone()}, data)
    t1 = pred["pred_t"].reshape(4, 3).clone()
    data2 = ds.zoom_batch(data, R1, t1)
    pred = model(data2["img_croped"], data2["cloud"], data2["choose"], data2["cls_id"], opt_pose=True)
    R2, _ = get_pose({"xyz": pred["xyz"].clone()}, data2)
    t2 = pred["pred_t"].reshape(4, 3).clone()
    torch.cuda.synchronize()
    assert np.array_equal(data2["zoom_status"].cpu().numpy(), zstat)
    want = np.concatenate([np.asarray(idx, np.float64)[:, None], R2.reshape(4, 9).double().cpu().numpy(),
                           t2.double().cpu().numpy()], 1)
    assert np.array_equal(tabs.poses.numpy().view(np.uint64), want.view(np.uint64))
    # and the second pass is a pass of its own: with a new window the crop, and so the pose, differs from the first
    if (zstat == 0).any():
        assert not torch.equal(data2["img_croped"], data["img_croped"])


def test_zoom_2_runs(dev, model):
    _reset()
    res = run_epoch(model, _ds(4), bs=4, device=dev, zoom=2)
    z = res["zoom"]
    assert res["test_count"] == 4 and z["passes"] == 2
    assert z["recropped"] + z["kept_bad_pose"] + z["kept_outside"] == 4
    model.invalidate_plans()
