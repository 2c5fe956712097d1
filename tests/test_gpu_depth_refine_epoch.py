"""Depth refinement through the pose layer and the eval epoch (pose.refine_pose_depth, evaluate.eval_records /
test_epoch(refine="depth")) on the generated BOP tree of test_gpu_verify_epoch.py (tests/bop_tree.py): one object,
three frames, crop sizes 40 / 80 / 40.

The epoch's refined poses must equal, bit for bit, pose.refine_pose_depth applied to the poses of a refine=None run
of the same crops (same seeds, same batches), and with select="depth" the selection sees four candidates. With the
base solver replaced by one that returns the GT pose a few millimetres and degrees off, the refined base pose must
also be closer to GT in translation and ADD."""
import numpy as np
import pytest
import torch

import bop_tree
from pose_estimation_amd import depth_refine

pytestmark = pytest.mark.gpu

OFF_T = (0.002, -0.0015, 0.0025)   # metres
OFF_DEG = 2.0                      # about the camera's (1, 1, 0) / sqrt(2)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def bop_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("depth_refine_trees")
    lm, bp = str(root / "lm"), str(root / "bop")
    bop_tree.write_twin(lm, bp)
    return bp


def _dataset(root, **kw):
    from pose_estimation_amd.dataset import PoseDataset
    return PoseDataset("test", 500, False, root, 0.0, 8, cls_type="cat", n_model_pts=150, layout="bop", **kw)


def _model(dev):
    from pose_estimation_amd import KRRN, make_config
    from pose_estimation_amd.synthetic import init_weights
    m = KRRN(cfg=make_config(num_cls=1, backbone="w18"))
    init_weights(m, 0)
    return m.to(dev).eval()


def _reset():
    from pose_estimation_amd import pose as kpose
    torch.manual_seed(5)
    kpose._seeds.clear()


def _near_gt(pred, data):
    """The GT pose OFF_DEG / OFF_T away: what a sound solver would hand to the refiner."""
    Rg, tg = data["target_r"], data["target_t"]
    a = np.deg2rad(OFF_DEG)
    k = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    dR = torch.tensor(np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx), dtype=Rg.dtype, device=Rg.device)
    return (dR @ Rg.reshape(-1, 3, 3)).contiguous(), tg.reshape(-1, 3) + torch.tensor(OFF_T, dtype=tg.dtype, device=tg.device)


def _buckets(d):
    b = {}
    for i in range(len(d)):
        b.setdefault(d.crop_size(i), []).append(i)
    return b


@pytest.mark.parametrize("opt_pose", [False, True])
def test_epoch_refine_depth_equals_the_eager_call(dev, bop_root, monkeypatch, opt_pose):
    from pose_estimation_amd import evaluate
    from pose_estimation_amd.evaluate import POSE_REC, REC, eval_records
    from pose_estimation_amd.pose import refine_pose_depth
    monkeypatch.setattr(evaluate, "get_pose", _near_gt)
    m, d = _model(dev), _dataset(bop_root, meshes=True)
    buckets = _buckets(d)
    _reset()                                                     # a fresh dataset per run: the same `choose` draws
    rec0, poses0 = eval_records(m, _dataset(bop_root, meshes=True), buckets, 2, dev, opt_pose=opt_pose, poses=True)
    _reset()
    rec1, poses1 = eval_records(m, _dataset(bop_root, meshes=True), buckets, 2, dev, opt_pose=opt_pose, poses=True,
                                refine="depth")
    torch.cuda.synchronize()
    assert poses1.shape == poses0.shape == (3, len(POSE_REC)) and poses0[:, 0].tolist() == poses1[:, 0].tolist()
    poses0, poses1 = poses0.numpy(), poses1.numpy()
    dia = torch.tensor(d.diameter, dtype=torch.float32).to(dev)
    o, statuses = 0, []
    for _, idx in evaluate._batches(buckets, 2):                 # the epoch's own batches, in its order
        assert poses0[o:o + len(idx), 0].tolist() == [float(i) for i in idx]
        data = d.batch(idx, dev, verify=True)
        R = torch.from_numpy(poses0[o:o + len(idx), 1:10]).to(torch.float32).reshape(-1, 3, 3).to(dev)
        t = torch.from_numpy(poses0[o:o + len(idx), 10:13]).to(torch.float32).to(dev)
        Rn, tn, info = refine_pose_depth(R, t, data, d, dia[data["cls_id"].reshape(len(idx))], return_info=True)
        torch.cuda.synchronize()
        statuses += info["status"].tolist()
        print(idx, "status", info["status"].tolist(), "passes", info["passes"].tolist(), "pairs", info["pairs"].tolist(),
              "rmse", info["rmse"].tolist())
        assert np.array_equal(_bits(poses1[o:o + len(idx), 1:10]), _bits(Rn.reshape(-1, 9).double().cpu().numpy())), idx
        assert np.array_equal(_bits(poses1[o:o + len(idx), 10:13]), _bits(tn.double().cpu().numpy())), idx
        o += len(idx)
    assert o == 3
    col = lambda r, k: r.numpy()[:, REC.index(k)]  # noqa: E731
    print("t_b", col(rec0, "t_b").tolist(), "->", col(rec1, "t_b").tolist(), " r_b", col(rec0, "r_b").tolist(), "->",
          col(rec1, "r_b").tolist(), " add_b", col(rec0, "add_b").tolist(), "->", col(rec1, "add_b").tolist())
    if not opt_pose:
        # the scored pose is the base pose: 3.5 mm and 2 degrees from GT, on the tree's millimetre depth. Every crop
        # refines (none starves) and ends closer to GT in translation and ADD. The tree's objects are icospheres,
        # whose rotation the depth hardly observes (bop_ref's `sphere`): r_b is printed, not bounded
        assert all(s in (depth_refine.STATUS.index("CONVERGED"), depth_refine.STATUS.index("MAX_ITER")) for s in statuses)
        assert (col(rec1, "t_b") < col(rec0, "t_b")).all() and (col(rec1, "add_b") < col(rec0, "add_b")).all()
    # nothing but the pose columns moved
    same = [REC.index(k) for k in ("crop", "cls", "l_xyz", "l_mask", "l_normal", "valid")]
    assert np.array_equal(_bits(rec0.numpy()[:, same]), _bits(rec1.numpy()[:, same]))
    with pytest.raises(ValueError, match="verify=True"):
        refine_pose_depth(R, t, d.batch(idx, dev, bop=True), d, 0.06)


def test_epoch_select_sees_four_candidates(dev, bop_root, monkeypatch):
    from pose_estimation_amd import evaluate
    from pose_estimation_amd.evaluate import SEL_REC
    from pose_estimation_amd.evaluate import test_epoch as run_epoch
    monkeypatch.setattr(evaluate, "get_pose", _near_gt)
    seen, real = [], evaluate.select_pose

    def spy(cands, data, dataset, tau=None):
        seen.append(len(cands))
        return real(cands, data, dataset, tau)

    monkeypatch.setattr(evaluate, "select_pose", spy)
    m = _model(dev)
    _reset()
    out = run_epoch(m, _dataset(bop_root, meshes=True), bs=2, device=dev, refine="depth", select="depth")
    assert seen == [4, 4]
    picked = out["select"]["picked"]
    assert sum(picked.values()) == 3 and set(picked) <= {0, 1, 2, 3} and 0.0 <= out["select"]["mean_score"] <= 1.0
    d = _dataset(bop_root, meshes=True)
    _reset()
    srec = evaluate.eval_records(m, d, _buckets(d), 2, dev, refine="depth", select="depth")[-1]
    assert srec.shape == (3, len(SEL_REC)) and set(srec[:, 1].tolist()) <= {0.0, 1.0, 2.0, 3.0}
    _reset()
    plain = run_epoch(m, _dataset(bop_root, meshes=True), bs=2, device=dev)
    assert "select" not in plain and plain["test_count"] == out["test_count"] == 3
    with pytest.raises(ValueError, match="meshes=True"):
        run_epoch(m, _dataset(bop_root), bs=2, device=dev, refine="depth")
