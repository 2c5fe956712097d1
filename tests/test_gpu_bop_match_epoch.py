"""evaluate.test_epoch(..., match=True) on the GPU, on the multi-instance tree of tests/bop_multi_tree.py with a
detection-driven dataset (det_per_target="inst_count"): the epoch's poses become result rows, and "bop" is
bop_scene.eval_results over them, i.e. what scoring the written CSV gives. The tree's own ground truth serves as
detections (bop_scene.gt_detections), with distinct scores."""
import numpy as np
import pytest
import torch

import bop_multi_tree as mt
from pose_estimation_amd import bop_scene
from pose_estimation_amd.dataset import PoseDataset
from pose_estimation_amd.evaluate import test_epoch as run_epoch

pytestmark = pytest.mark.gpu


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


def _same(a, b, path=""):
    """Bitwise equality of nested dicts of floats / anything comparable."""
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


def _ds(root, **kw):
    return PoseDataset("test", 500, False, root, 0.0, 8, n_model_pts=4, layout="bop", meshes=True, **kw)


@pytest.fixture(scope="module")
def multi(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("epoch_multi"))
    mt.write_tree(root)
    rows = bop_scene.gt_detections(_ds(root).tree)
    for r, s in zip(rows, (0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3)):
        r["score"] = s
    return root, rows


def test_match_epoch(dev, multi, tmp_path):
    root, det = multi
    counts = {(1, 0, 2): 3, (1, 0, 3): 2, (1, 1, 3): 1, (1, 1, 1): 1}
    m = _model(dev, 3)
    csv = str(tmp_path / "krrn_multi-test.csv")
    ds = _ds(root, detections=det, det_per_target="inst_count")
    assert len(ds) == 7 and ds.tree.inst_count == counts and ds.tree.missed == []
    _reset()
    out = run_epoch(m, ds, bs=4, device=dev, bop=True, match=True, bop_csv=csv)
    rows = bop_scene.read_results(csv)
    per_key = {}
    for r in rows:
        k = (r["scene_id"], r["im_id"], r["obj_id"])
        per_key[k] = per_key.get(k, 0) + 1
    assert per_key == counts                             # inst_count rows per fully detected target
    assert sorted(r["score"] for r in rows) == sorted(d["score"] for d in det)
    want = bop_scene.eval_results(ds, rows, dev)
    print({k: out["bop"][k] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR", "count", "targets")}, out["bop"]["matches"])
    _same(out["bop"], want)
    assert out["bop"]["targets"] == 7 and out["bop"]["count"] == 7 and out["bop"]["ignored"] == 0
    assert out["test_count"] == 7
    assert out["detections"] == {"targets": 7, "estimated": 7, "missed": 0, "rows": 7, "unused": 0, "dropped": 0}
    assert out["detections"]["targets"] == sum(counts.values())
    # every other key is as before: the same epoch without bop (bop=True, match=False is refused on this dataset)
    _reset()
    base = run_epoch(m, _ds(root, detections=det, det_per_target="inst_count"), bs=4, device=dev)
    assert "bop" not in base
    _same({k: v for k, v in out.items() if k != "bop"}, base)

    # one detection of the tripled object dropped: one target instance is missed, the denominator stays
    less = [d for j, d in enumerate(det) if j != 2]
    ds2 = _ds(root, detections=less, det_per_target="inst_count")
    assert len(ds2) == 6 and ds2.tree.missed == [(1, 0, 2)]
    _reset()
    out2 = run_epoch(m, ds2, bs=4, device=dev, bop=True, match=True)
    assert out2["detections"] == {"targets": 7, "estimated": 6, "missed": 1, "rows": 6, "unused": 0, "dropped": 0}
    assert out2["bop"]["targets"] == 7 and out2["bop"]["count"] == 6 and out2["test_count"] == 6
    assert out2["bop"]["per_obj"][2]["targets"] == 3 and out2["bop"]["per_obj"][2]["count"] == 2
    assert len(out2["bop"]["matches"]) == 7


def test_refusals(dev, multi):
    root, det = multi
    m = torch.nn.Linear(1, 1)                            # refused before the model is touched
    ds = _ds(root, detections=det, det_per_target="inst_count")
    with pytest.raises(ValueError, match="det_per_target='inst_count'.*match=True"):
        run_epoch(m, ds, bs=4, device=dev, bop=True, match=False)
    with pytest.raises(ValueError, match="match=True.*needs bop=True"):
        run_epoch(m, ds, bs=4, device=dev, match=True)
