"""BOP detection files without a GPU, on the tiny multi-instance tree of tests/bop_tree.py: read_detections /
write_detections and every ValueError of theirs, how BopTree pairs the kept GT instances with detection rows (and what
it counts in det_stats / missed), the inst_count > 1 refusal, PoseDataset's constructor refusals, and
bop.fold_bop(missed=...)."""
import json
import os
import shutil

import numpy as np
import pytest

import bop_tree
import rle_ref as rf
from pose_estimation_amd import bop, bop_scene, rle
from pose_estimation_amd.dataset import PoseDataset, get_square_bbox


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("det_host"))
    bop_tree.write_tree(root)
    return root


def _row(scene, im, obj, score, bbox, counts=None, size=None, **extra):
    r = {"scene_id": scene, "image_id": im, "category_id": obj, "score": score, "bbox": list(bbox)}
    if counts is not None:
        r["segmentation"] = {"counts": counts, "size": list(size)}
    r.update(extra)
    return r


def test_detections_round_trip(tmp_path):
    c = [6, 1, 40, 4, 5, 4, 5, 4, 21]                    # a 9 x 10 mask
    rows = [_row(1, 3, 2, 0.75, [1, 2, 3, 4], c, (9, 10), time=0.25),
            _row(1, 3, 5, 0.5, [0.5, 1.5, 7.25, 2.0]),                       # box only, no time
            _row(2, 0, 2, 1, [4, 4, 2, 2], rle.counts_to_string(c), (9, 10))]
    p = str(tmp_path / "det.json")
    bop_scene.write_detections(p, rows)
    back = bop_scene.read_detections(p)
    assert back[0] == {"scene_id": 1, "image_id": 3, "category_id": 2, "score": 0.75, "bbox": [1.0, 2.0, 3.0, 4.0],
                       "segmentation": {"counts": c, "size": [9, 10]}, "time": 0.25}
    assert back[1] == {"scene_id": 1, "image_id": 3, "category_id": 5, "score": 0.5, "bbox": [0.5, 1.5, 7.25, 2.0]}
    assert back[2]["segmentation"] == {"counts": c, "size": [9, 10]} and back[2]["score"] == 1.0
    with open(p) as f:
        on_disk = json.load(f)
    assert isinstance(on_disk, list) and on_disk[2]["segmentation"]["counts"] == c   # masks are written as run lists
    with open(p, "w") as f:                              # a file as a detector writes it: compressed strings
        json.dump(rows, f)
    assert bop_scene.read_detections(p) == back
    bop_scene.write_detections(p, back)
    assert bop_scene.read_detections(p) == back


def test_read_detections_errors(tmp_path):
    p = str(tmp_path / "bad.json")
    good = _row(1, 3, 2, 0.75, [1, 2, 3, 4], [6, 1, 83], (9, 10))

    def reading(rows):
        with open(p, "w") as f:
            json.dump(rows, f)
        return bop_scene.read_detections(p)

    assert len(reading([good, good])) == 2
    for k in ("scene_id", "image_id", "category_id", "score", "bbox"):
        with pytest.raises(ValueError, match=f"entry 1 has no '{k}'"):
            reading([good, {a: b for a, b in good.items() if a != k}])
    for bb in ([1, 2, 3], [1, 2, 3, 4, 5], [1, 2, "3", 4], "1234", None, [1, 2, 3, True]):
        with pytest.raises(ValueError, match="entry 2: bbox must be 4 numbers"):
            reading([good, good, dict(good, bbox=bb)])
    for seg in ({"counts": [6, 1, 83]}, {"size": [9, 10]}, [6, 1, 83]):
        with pytest.raises(ValueError, match="entry 0: segmentation needs both"):
            reading([dict(good, segmentation=seg)])
    with pytest.raises(ValueError, match="entry 0: bad segmentation"):
        reading([dict(good, segmentation={"counts": "6 1", "size": [9, 10]})])
    with pytest.raises(ValueError, match=r"entry 0: segmentation.size must be \[H, W\]"):
        reading([dict(good, segmentation={"counts": [90], "size": [9, 10, 3]})])
    with pytest.raises(ValueError, match="a list of detections"):
        reading({"0": good})
    with pytest.raises(ValueError, match="entry 1 is not an object"):
        reading([good, 5])


def test_pairing(tiny, tmp_path):
    plain = bop_scene.BopTree(tiny, n_model_pts=4)
    assert plain.det_stats is None and plain.missed == []
    H, W = plain.frame_hw
    key = lambda it: (it["scene"], it["im"], it["obj"])  # noqa: E731
    assert [key(it) for it in plain.items] == [(1, 3, 3), (1, 3, 2), (1, 7, 3), (1, 7, 1), (2, 0, 3)]
    gt = bop_scene.gt_detections(plain)
    assert [(r["scene_id"], r["image_id"], r["category_id"]) for r in gt] == [key(it) for it in plain.items]
    for i, (r, it) in enumerate(zip(gt, plain.items)):
        assert r["score"] == 1.0 and r["bbox"] == it["bbox"] and r["segmentation"]["size"] == [H, W]
        assert np.array_equal(rf.decode(r["segmentation"]["counts"], H, W), plain.read_mask(i))
    seg = lambda i: dict(counts=gt[i]["segmentation"]["counts"], size=(H, W))  # noqa: E731
    rows = [
        _row(1, 3, 3, 0.5, gt[0]["bbox"], **seg(0)),             # 0  out-scored by row 2
        _row(1, 3, 2, 0.7, [20, 10, 9, 9]),                      # 1  wins the tie with row 3: the earlier one
        _row(1, 3, 3, 0.9, [5, 6, 12, 14]),                      # 2  the higher score wins; box only
        _row(1, 3, 2, 0.7, gt[1]["bbox"], **seg(1)),             # 3
        _row(1, 7, 3, 0.05, gt[2]["bbox"], **seg(2)),            # 4  below det_min_score
        _row(1, 7, 3, 0.3, gt[2]["bbox"], **seg(2)),             # 5  used
        _row(1, 7, 9, 0.8, [1, 1, 5, 5]),                        # 6  an object that is no target: unused
        _row(1, 7, 1, 0.99, gt[3]["bbox"], [H * W], (H, W)),     # 7  no set pixel: dropped
        _row(1, 7, 1, 0.98, [3, 3, 0, 5]),                       # 8  w = 0: dropped
        _row(1, 7, 1, 0.4, gt[3]["bbox"], **seg(3)),             # 9  used
        _row(5, 0, 3, 0.9, [1, 1, 5, 5]),                        # 10 a scene the tree does not hold: unused
    ]                                                            # and no row for (2, 0, 3): missed
    p = str(tmp_path / "det.json")
    bop_scene.write_detections(p, rows)
    for src in (p, rows):                                        # a path or the rows themselves
        t = bop_scene.BopTree(tiny, n_model_pts=4, detections=src, det_min_score=0.1)
        assert [key(it) for it in t.items] == [(1, 3, 3), (1, 3, 2), (1, 7, 3), (1, 7, 1)]
        assert [it["det"] for it in t.items] == [2, 1, 5, 9] and [it["score"] for it in t.items] == [0.9, 0.7, 0.3, 0.4]
        assert t.missed == [(2, 0, 3)] and t.objlist == [1, 2, 3]
        assert t.det_stats == {"rows": 11, "used": 4, "unused": 5, "dropped": 2}
        assert t.items[0]["bbox"] == [5.0, 6.0, 12.0, 14.0] and t.items[0]["rle"] == rle.box_counts(5, 6, 12, 14, H, W)
        assert t.items[2]["bbox"] == gt[2]["bbox"] and t.items[2]["rle"] == gt[2]["segmentation"]["counts"]
        for it, old in zip(t.items, plain.items):                # the GT side is the paired instance's
            assert it["gt"] == old["gt"] and np.array_equal(it["R"], old["R"]) and it["K4"] == old["K4"]
    t = bop_scene.BopTree(tiny, n_model_pts=4, detections=rows)  # det_min_score 0: row 5 still out-scores row 4
    assert [it["det"] for it in t.items] == [2, 1, 5, 9] and t.det_stats["unused"] == 5
    t = bop_scene.BopTree(tiny, n_model_pts=4, detections=rows, det_min_score=0.35)
    assert [it["det"] for it in t.items] == [2, 1, 9] and t.missed == [(1, 7, 3), (2, 0, 3)]
    assert t.det_stats == {"rows": 11, "used": 3, "unused": 6, "dropped": 2}
    full = bop_scene.BopTree(tiny, n_model_pts=4, detections=gt)
    assert full.det_stats == {"rows": 5, "used": 5, "unused": 0, "dropped": 0} and full.missed == []
    assert [it["bbox"] for it in full.items] == [it["bbox"] for it in plain.items]
    with pytest.raises(ValueError, match=r"detection 0: segmentation.size \[48, 32\] is not the tree's frame size"):
        bop_scene.BopTree(tiny, n_model_pts=4, detections=[_row(1, 3, 3, 0.5, [1, 1, 5, 5], [5, 4, H * W - 9], (48, 32))])
    with pytest.raises(ValueError, match="detection 0: its runs do not fill"):
        bop_scene.BopTree(tiny, n_model_pts=4, detections=[_row(1, 3, 3, 0.5, [1, 1, 5, 5], [5, 4, 7], (H, W))])
    with pytest.raises(ValueError, match="without detections"):
        bop_scene.gt_detections(full)
    # the dataset: the crop is snapped from the detection's box; the refusals
    ds = PoseDataset("test", 500, False, tiny, 0.0, 8, layout="bop", n_model_pts=4, detections=rows, det_min_score=0.1)
    assert len(ds) == 4 and ds.detections and ds.boxes[0] == get_square_bbox([5.0, 6.0, 12.0, 14.0], H, W)
    assert ds.objlist == [1, 2, 3] and not PoseDataset("test", 500, False, tiny, 0.0, 8, layout="bop", n_model_pts=4).detections
    with pytest.raises(ValueError, match="layout='bop'"):
        PoseDataset("test", 500, False, tiny, 0.0, 8, detections=rows)
    with pytest.raises(ValueError, match="masks='render'"):
        PoseDataset("test", 500, False, tiny, 0.0, 8, layout="bop", n_model_pts=4, meshes=True, masks="render",
                    detections=rows)


def test_two_instances_of_one_object_are_refused(tiny, tmp_path):
    root = str(tmp_path / "twice")
    shutil.copytree(tiny, root)
    sdir = os.path.join(root, "test", "000001")
    for name in ("scene_gt.json", "scene_gt_info.json"):
        with open(os.path.join(sdir, name)) as f:
            content = json.load(f)
        content["3"].append(content["3"][0])             # image 3 now holds object 3 twice
        with open(os.path.join(sdir, name), "w") as f:
            json.dump(content, f)
    assert len(bop_scene.BopTree(root, n_model_pts=4).items) == 6            # fine without detections, as before
    with pytest.raises(ValueError, match=r"scene 1, image 3, object 3.*inst_count > 1"):
        bop_scene.BopTree(root, n_model_pts=4, detections=[])
    assert len(bop_scene.BopTree(root, n_model_pts=4, detections=[], objlist=[2]).items) == 0   # not a kept target


def test_fold_bop_missed():
    T = len(bop.TAUS)
    rec = np.zeros((4, len(bop.BOP_REC)))                # errors 0: correct at every threshold
    rec[:, 0], rec[:, -1] = np.arange(4), [1, 1, 1, 0]   # three records and a pad row
    base = bop.fold_bop(rec, [5], [0.1], 64.0)
    assert base == {"AR_VSD": 1.0, "AR_MSSD": 1.0, "AR_MSPD": 1.0, "AR": 1.0, "count": 3,
                    "per_obj": {5: {"AR_VSD": 1.0, "AR_MSSD": 1.0, "AR_MSPD": 1.0, "AR": 1.0, "count": 3}}}
    assert bop.fold_bop(rec, [5], [0.1], 64.0, missed=None) == base
    out = bop.fold_bop(rec, [5], [0.1], 64.0, missed={5: 1})
    want = {"AR_VSD": 0.75, "AR_MSSD": 0.75, "AR_MSPD": 0.75, "AR": 0.75, "count": 3, "targets": 4}
    assert out == dict(want, per_obj={5: want})
    none = bop.fold_bop(rec, [5], [0.1], 64.0, missed={})
    assert none == dict(base, targets=3, per_obj={5: dict(base["per_obj"][5], targets=3)})
    # two objects, one of them with missed targets only: it occurs in per_obj with recall 0
    rec2 = rec.copy()
    rec2[1, 1] = 1
    rec2[1, 2 + T] = 1.0                                 # an MSSD of 1 m: wrong at every threshold
    out = bop.fold_bop(rec2, [5, 7, 9], [0.1, 0.1, 0.1], 64.0, missed={9: 2, 5: 1, 7: 0})
    assert out["count"] == 3 and out["targets"] == 6 and list(out["per_obj"]) == [5, 7, 9]
    ap = lambda d: pytest.approx(d, rel=1e-15, abs=0)    # noqa: E731  (a mean of ten equal thirds rounds once more)
    assert out["per_obj"][5] == ap({"AR_VSD": 2 / 3, "AR_MSSD": 2 / 3, "AR_MSPD": 2 / 3, "AR": 2 / 3, "count": 2, "targets": 3})
    assert out["per_obj"][7] == ap({"AR_VSD": 1.0, "AR_MSSD": 0.0, "AR_MSPD": 1.0, "AR": 2 / 3, "count": 1, "targets": 1})
    assert out["per_obj"][9] == {"AR_VSD": 0.0, "AR_MSSD": 0.0, "AR_MSPD": 0.0, "AR": 0.0, "count": 0, "targets": 2}
    assert out["AR_MSSD"] == ap(2 / 6) and out["AR_VSD"] == 3 / 6
