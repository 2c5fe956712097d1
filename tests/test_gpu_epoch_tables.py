"""evaluate.eval_records' tables for every combination of (bop, poses, select) on the GPU: three crops of the
multi-instance tree of tests/bop_multi_tree.py (both instances of object 3 in image 0 and object 1 of image 1, kept by a
targets file of its own), bs = 2, meshes on. get_pose is replaced by test_gpu_depth_refine_epoch's near-GT stand-in, so
no RANSAC draw is involved and every run of a dataset sees the same base pose.

Asserted: the return's layout (a lone tensor, else rec, bop, poses, sel in that order, by width); `rec` bit for bit the
same whatever other tables are asked for, as long as select is None; and that the pose table holds the pose test_dis
scores: the base pose without opt_pose (the stand-in's own output, bit for bit), else the final pose, i.e. the one whose
rotation / translation errors are the record's r_f / t_f."""
import itertools
import json

import numpy as np
import pytest
import torch

import bop_multi_tree as mt
from test_gpu_depth_refine_epoch import _near_gt

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("epoch_tables")
    mt.write_tree(str(root))
    targets = str(root / "three.json")
    with open(targets, "w") as f:
        json.dump([{"scene_id": 1, "im_id": 0, "obj_id": 3, "inst_count": 2},
                   {"scene_id": 1, "im_id": 1, "obj_id": 1, "inst_count": 1}], f)
    return str(root), targets


def _dataset(tree):
    from pose_estimation_amd.dataset import PoseDataset
    return PoseDataset("test", 500, False, tree[0], 0.0, 8, n_model_pts=4, layout="bop", meshes=True, targets=tree[1])


@pytest.mark.parametrize("opt_pose", [False, True])
def test_tables_of_every_combination(dev, tree, monkeypatch, opt_pose):
    from pose_estimation_amd import KRRN, evaluate, make_config
    from pose_estimation_amd import pose as kpose
    from pose_estimation_amd.bop import BOP_REC
    from pose_estimation_amd.evaluate import POSE_REC, REC, SEL_REC, eval_records
    from pose_estimation_amd.metric import rt_errors
    from pose_estimation_amd.synthetic import init_weights
    monkeypatch.setattr(evaluate, "get_pose", _near_gt)
    model = KRRN(cfg=make_config(num_cls=2, backbone="w18"))
    init_weights(model, 0)
    model = model.to(dev).eval()
    probe = _dataset(tree)
    assert len(probe) == 3 and [it["obj"] for it in probe.tree.items] == [3, 3, 1]
    buckets = {}
    for i in range(3):
        buckets.setdefault(probe.crop_size(i), []).append(i)
    order = [i for _, idx in evaluate._batches(buckets, 2) for i in idx]
    # the GT poses and what the stand-in makes of them, over the epoch's own batches in its order
    gt = [probe.batch(idx, dev) for _, idx in evaluate._batches(buckets, 2)]
    Rg, tg = torch.cat([d["target_r"].reshape(-1, 9) for d in gt]), torch.cat([d["target_t"].reshape(-1, 3) for d in gt])
    near = [_near_gt(None, d) for d in gt]
    Rn, tn = torch.cat([r.reshape(-1, 9) for r, _ in near]), torch.cat([t.reshape(-1, 3) for _, t in near])
    col = lambda rec, k: rec.numpy()[:, REC.index(k)]  # noqa: E731
    first = None
    for bop, poses, select in itertools.product([False, True], [False, True], [None, "depth"]):
        if select and not opt_pose:
            continue                                             # refused: select chooses the final pose
        torch.manual_seed(5)
        kpose._seeds.clear()                                     # a fresh dataset per run: the same `choose` draws
        out = eval_records(model, _dataset(tree), buckets, 2, dev, opt_pose=opt_pose, bop=bop, poses=poses, select=select)
        torch.cuda.synchronize()
        widths = [len(REC)] + [len(BOP_REC)] * bop + [len(POSE_REC)] * poses + [len(SEL_REC)] * bool(select)
        if len(widths) == 1:
            assert isinstance(out, torch.Tensor)
            out = (out,)
        else:
            assert isinstance(out, tuple)
        assert [tuple(t.shape) for t in out] == [(3, w) for w in widths], (bop, poses, select)
        assert all(t.dtype == torch.float64 and t[:, 0].tolist() == [float(i) for i in order] for t in out)
        rec = out[0]
        if select is None:
            first = rec if first is None else first
            assert np.array_equal(_bits(rec.numpy()), _bits(first.numpy())), (bop, poses)
        if poses:
            tab = out[1 + bop]
            R, t = tab[:, 1:10].to(torch.float32).to(dev), tab[:, 10:13].to(torch.float32).to(dev)
            assert torch.equal(R.double().cpu(), tab[:, 1:10]) and torch.equal(t.double().cpu(), tab[:, 10:13])   # f32 poses
            if not opt_pose:
                assert np.array_equal(_bits(R.cpu().numpy()), _bits(Rn.float().cpu().numpy()))
                assert np.array_equal(_bits(t.cpu().numpy()), _bits(tn.float().cpu().numpy()))
            elif select is None:
                assert np.array_equal(_bits(R.cpu().numpy()), _bits(Rn.float().cpu().numpy()))   # (the solver's R, TBase's t)
            r_err, t_err = rt_errors(R, t, Rg, tg)
            kr, kt = ("r_f", "t_f") if opt_pose else ("r_b", "t_b")
            assert np.array_equal(_bits(r_err), _bits(col(rec, kr))) and np.array_equal(_bits(t_err), _bits(col(rec, kt)))
    assert first is not None
    if opt_pose:
        assert not np.array_equal(col(first, "t_f"), col(first, "t_b"))   # the final t is TBase's, not the stand-in's
