"""bop_scene.eval_results on the GPU against its numpy restatement (tests/bop_match_ref.py: one pair at a time through
bop_ref.vsd / bop_ref.mssd_mspd, then the matching cell by cell) on the multi-instance tree of tests/bop_multi_tree.py:
one image holds object 2 three times and object 3 twice; the rows hold perturbed GT poses, a near-duplicate pair aimed
at one instance, a gross pose, a row for an unknown target, and one target has no row. The inputs' conditions (no
undecided VSD pixel in any pair, no MSSD / MSPD error within 1e-9 relative of a threshold) are asserted on the
restatement, so the integer counts must agree exactly and the recalls to rounding. Then the 1 : 1 case on
tests/bop_tree.py's tree: eval_results equals bop.fold_bop(missed=...) on the same poses."""
import numpy as np
import pytest
import torch

import bop_match_ref as mr
import bop_multi_tree as mt
import bop_ref as br
import bop_tree
from pose_estimation_amd import bop, bop_scene
from pose_estimation_amd.dataset import PoseDataset

pytestmark = pytest.mark.gpu
RECALLS = ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")


def _ds(root, **kw):
    return PoseDataset("test", 500, False, root, 0.0, 8, n_model_pts=4, layout="bop", meshes=True, **kw)


@pytest.fixture(scope="module")
def multi(tmp_path_factory):
    """(dataset, rows, tags, the restatement's result): built and restated once for the module."""
    root = str(tmp_path_factory.mktemp("eval_multi"))
    made = mt.write_tree(root)
    ds = _ds(root, targets=made["targets"])
    rows, tags = mt.result_rows(made)
    return ds, rows, tags, mr.eval_results(ds.tree, rows, bop.THETAS, bop.THETAS_PX)


def _close(got, want):
    for k in RECALLS:
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
    assert got["count"] == want["count"] and got["targets"] == want["targets"]


def test_inputs_are_decided(multi):
    ds, rows, tags, ref = multi
    assert ds.tree.inst_count == {(1, 0, 2): 3, (1, 0, 3): 2, (1, 1, 3): 1, (1, 1, 1): 1} and len(ds.tree.instances) == 7
    assert len(ref["pairs"]) == 4 * 3 + 2 * 2 + 1
    worst = np.inf
    for (r, i), p in ref["pairs"].items():
        br.check_conditions(p["vsd"])                    # no undecided VSD pixel
        for e, thr in ((p["mssd"], p["thr_mssd"]), (p["mspd"], p["thr_mspd"])):
            worst = min(worst, float(np.min(np.abs(e - thr) / thr)))
    print("worst relative distance of an MSSD / MSPD error from a threshold:", worst)
    assert worst > 1e-9
    # the rows do what the module doc says: the duplicate pair competes for one instance, the gross pose and the
    # row beyond n_top match nothing, the unknown target is ignored, the bare target counts
    m = ref["matches"]
    assert ref["ignored"] == 1 and ref["targets"] == 7 and ref["count"] == 3 + 2 + 1
    assert m[0] in tags["dup"] and tags["gross"] not in m and tags["unknown"] not in m and 4 not in m
    assert m.count(-1) == 3 and ref["per_obj"][tags["bare"][2]]["AR"] == 0.0 and 0.0 < ref["AR"] < 1.0


def test_eval_results_equals_restatement(dev, multi):
    ds, rows, tags, ref = multi
    got = bop_scene.eval_results(ds, rows, dev)
    torch.cuda.synchronize()
    print({k: (got[k], ref[k]) for k in RECALLS}, got["matches"], ref["matches"])
    assert set(got) == set(RECALLS) | {"count", "targets", "per_obj", "ignored", "matches"}
    _close(got, ref)
    assert got["matches"] == ref["matches"] and got["ignored"] == ref["ignored"] == 1
    assert set(got["per_obj"]) == set(ref["per_obj"]) == {1, 2, 3}
    for o in got["per_obj"]:
        _close(got["per_obj"][o], ref["per_obj"][o])
    # one image per chunk: the same numbers bit for bit (integer sums, a group does not depend on the batch)
    assert bop_scene.eval_results(ds, rows, dev, chunk_images=1) == got
    # shuffled rows: nothing changes but the row indices in `matches`
    perm = [5, 2, 7, 0, 6, 3, 1, 4]
    back = bop_scene.eval_results(ds, [rows[p] for p in perm], dev)
    assert [perm[x] if x >= 0 else -1 for x in back["matches"]] == got["matches"]
    assert {k: v for k, v in back.items() if k != "matches"} == {k: v for k, v in got.items() if k != "matches"}
    # no rows at all: every target still counts
    none = bop_scene.eval_results(ds, [], dev)
    assert none["AR"] == 0.0 and none["count"] == 0 and none["targets"] == 7 and none["matches"] == [-1] * 7
    with pytest.raises(ValueError, match="layout='bop' and meshes=True"):
        bop_scene.eval_results(PoseDataset("test", 500, False, ds.root, 0.0, 8, n_model_pts=4, layout="bop"), rows, dev)


def test_one_to_one_equals_fold_bop(dev, tmp_path):
    """Every target with one instance and at most one row: fold_bop over the per-crop errors of the same poses."""
    root = str(tmp_path / "tiny")
    bop_tree.write_tree(root)
    ds = _ds(root)
    n = len(ds)
    assert n == 5 and all(v == 1 for v in ds.tree.inst_count.values())
    rng = np.random.default_rng(8)
    poses = [br.perturbed(rng, it["R"], it["t"], deg=2.0 + 3.0 * i, mm=3.0 + 4.0 * i) for i, it in enumerate(ds.tree.items)]
    rows = [{"scene_id": it["scene"], "im_id": it["im"], "obj_id": it["obj"], "score": 1.0, "R": R, "t": t * 1000.0,
             "time": -1.0} for it, (R, t) in zip(ds.tree.items, poses)]
    T = len(bop.TAUS)
    rec = np.zeros((n, len(bop.BOP_REC)))
    for idx in ([0, 1, 2], [3, 4]):                      # one crop size per batch
        data = ds.batch(idx, dev, bop=True)
        R = torch.from_numpy(np.stack([rows[i]["R"] for i in idx])).to(dev)
        t = torch.from_numpy(np.stack([rows[i]["t"] / 1000.0 for i in idx])).to(dev)      # what eval_results reads
        e = bop.bop_errors(R, t, data, ds)
        rec[idx, 0], rec[idx, 1], rec[idx, -1] = idx, data["cls_id"].reshape(-1).cpu().numpy(), 1.0
        rec[idx, 2:2 + T], rec[idx, 2 + T], rec[idx, 3 + T] = (e[k].cpu().numpy() for k in ("vsd", "mssd", "mspd"))
    for keep in (list(range(n)), [0, 1, 3]):             # every target estimated; two targets without a row
        missed = {}
        for i in set(range(n)) - set(keep):
            missed[ds.tree.items[i]["obj"]] = missed.get(ds.tree.items[i]["obj"], 0) + 1
        want = bop.fold_bop(rec[keep], ds.objlist, ds.diameter, ds.frame_hw[1], missed=missed)
        got = bop_scene.eval_results(ds, [rows[i] for i in keep], dev)
        print(keep, {k: (got[k], want[k]) for k in RECALLS})
        _close(got, want)
        assert set(got["per_obj"]) == set(want["per_obj"])
        for o in want["per_obj"]:
            _close(got["per_obj"][o], want["per_obj"][o])
        assert got["ignored"] == 0 and all(m == -1 or keep[m] == i for i, m in enumerate(got["matches"]))
        assert sum(m >= 0 for m in got["matches"]) >= 1
    assert 0.0 < want["AR"] < 1.0
