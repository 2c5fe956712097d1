"""Detection-mode datasets and epochs on the GPU. The anchor is an exact equivalence: bop_scene.gt_detections writes a
tree's own bbox_visib / mask_visib as detections, so a dataset built on them must equal the tree's PNG mode bit for
bit, for every batch key and every epoch number: that pins the RLE decode, the box path and the plumbing at once. Then
box-only rows, a missed target's place in the recalls' denominator, and the result CSV's score column."""
import numpy as np
import pytest
import torch

import bop_tree
import rle_ref as rf
from pose_estimation_amd import bop, bop_scene
from pose_estimation_amd.dataset import PoseDataset
from pose_estimation_amd.evaluate import eval_records
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


def _same(a, b, path="", skip=()):
    """Bitwise equality of nested dicts of tensors / floats / anything comparable, but for the keys in `skip`."""
    if isinstance(a, dict):
        ka, kb = set(a) - set(skip), set(b) - set(skip)
        assert ka == kb, (path, ka ^ kb)
        for k in ka:
            _same(a[k], b[k], f"{path}/{k}", skip)
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
    elif isinstance(a, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), (path, a, b)
    else:
        assert a == b, (path, a, b)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("det_tiny"))
    bop_tree.write_tree(root)
    return root


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("det_twin")
    bop_tree.write_twin(str(d / "lm"), str(d / "bop"))
    return str(d / "bop")


def _ds(root, small, **kw):
    """The tiny multi-instance tree (4 model points) or the one-object twin tree (150)."""
    if small:
        return PoseDataset("test", 500, False, root, 0.0, 8, n_model_pts=4, layout="bop", meshes=True, **kw)
    return PoseDataset("test", 500, False, root, 0.0, 8, cls_type="cat", n_model_pts=150, layout="bop", meshes=True, **kw)


@pytest.mark.parametrize("which", ["twin", "tiny"])
def test_oracle_detections_equal_png_mode(dev, which, tiny, twin):
    small = which == "tiny"
    root = tiny if small else twin
    rows = bop_scene.gt_detections(_ds(root, small).tree)
    groups = ([0, 1, 2], [3, 4]) if small else ([0, 2], [1])     # one crop size per batch
    for kw in ({"bop": True}, {"verify": True}):
        png, det = _ds(root, small), _ds(root, small, detections=rows)
        assert len(png) == len(det) == (5 if small else 3) and png.boxes == det.boxes and png.objlist == det.objlist
        for idx in groups:
            a, b = png.batch(idx, dev, **kw), det.batch(idx, dev, **kw)
            torch.cuda.synchronize()
            assert set(b) - set(a) == {"det_score", "det_info"} and set(a) <= set(b)
            _same(a, {k: b[k] for k in a})
            assert b["det_score"].dtype == torch.float32 and b["det_score"].tolist() == [1.0] * len(idx)
            want = np.stack([rf.info(png.tree.read_mask(i)) for i in idx])
            assert b["det_info"].dtype == torch.int32 and np.array_equal(b["det_info"].cpu().numpy(), want)
            if "verify_mask" in b:
                assert np.array_equal(b["verify_mask"].cpu().numpy(), np.stack([png.tree.read_mask(i) for i in idx]))
    m = _model(dev, len(png.objlist))
    _reset()
    ra = run_epoch(m, _ds(root, small), bs=2, device=dev, bop=True)
    _reset()
    rb = run_epoch(m, _ds(root, small, detections=rows), bs=2, device=dev, bop=True)
    n = len(png)
    assert ra["test_count"] == n and "detections" not in ra and "targets" not in ra["bop"]
    assert rb["detections"] == {"targets": n, "estimated": n, "missed": 0, "rows": n, "unused": 0, "dropped": 0}
    assert rb["bop"]["targets"] == n and all(v["targets"] == v["count"] for v in rb["bop"]["per_obj"].values())
    _same(ra, rb, skip=("detections", "targets"))


def test_box_only_detections(dev, tiny):
    """Rows without `segmentation`: mask_label is the filled box, clipped to the frame; the epoch runs."""
    rows = [{k: v for k, v in r.items() if k != "segmentation"} for r in bop_scene.gt_detections(_ds(tiny, True).tree)]
    rows[0]["bbox"] = [-3.0, 30.0, 20.0, 40.0]           # cut by the left and bottom borders
    ds = _ds(tiny, True, detections=rows)
    H, W = ds.frame_hw
    sizes = {ds.crop_size(i) for i in range(len(ds))}
    idx = [i for i in range(len(ds)) if ds.crop_size(i) == ds.crop_size(0)]
    assert 0 in idx and len(sizes) >= 1
    b = ds.batch(idx, dev, verify=True)
    torch.cuda.synchronize()
    got = b["verify_mask"].cpu().numpy()
    for j, i in enumerate(idx):
        x, y, w, h = rows[ds.tree.items[i]["det"]]["bbox"]
        ref = np.zeros((H, W), np.uint8)
        ref[max(0, round(y)):min(H, round(y + h)), max(0, round(x)):min(W, round(x + w))] = 1
        assert ref.any() and np.array_equal(got[j], ref), i
        assert np.array_equal(b["det_info"][j].cpu().numpy(), rf.info(ref)), i
    _reset()
    out = run_epoch(_model(dev, 3), _ds(tiny, True, detections=rows), bs=3, device=dev, bop=True)
    assert out["test_count"] == 5 and out["bop"]["count"] == out["bop"]["targets"] == 5
    assert out["detections"]["rows"] == 5 and out["detections"]["missed"] == 0


def test_missed_target_stays_in_the_denominator(dev, tiny):
    """The last target's row removed from the file: one crop fewer is evaluated, the targets stay five, and every
    AR is the full run's correct counts of the four remaining crops over the five targets. Batches of one crop,
    and the shorter dataset's draw seed set to the full one's (PoseDataset seeds its draws from its length), so the
    four crops see the same draws in both runs: their records are then the same, which is printed, not assumed."""
    rows = bop_scene.gt_detections(_ds(tiny, True).tree)
    m = _model(dev, 3)
    full = _ds(tiny, True, detections=rows)
    _reset()
    rec_f, brec_f = eval_records(m, full, {40: list(range(5))}, 1, dev, bop=True)
    _reset()
    ref = run_epoch(m, _ds(tiny, True, detections=rows), bs=1, device=dev, bop=True)
    red = _ds(tiny, True, detections=rows[:-1])
    assert len(red) == 4 and red.tree.missed == [(2, 0, 3)] and red.objlist == full.objlist
    red._seed_for(dev).fill_(int(np.random.SeedSequence(len(full)).generate_state(1)[0]))
    _reset()
    out = run_epoch(m, red, bs=1, device=dev, bop=True)
    assert ref["test_count"] == 5 and out["test_count"] == 4
    assert out["bop"]["targets"] == ref["bop"]["targets"] == 5 and out["bop"]["count"] == 4
    assert out["detections"] == {"targets": 5, "estimated": 4, "missed": 1, "rows": 4, "unused": 0, "dropped": 0}
    assert out["bop"]["per_obj"][3]["targets"] == 3 and out["bop"]["per_obj"][3]["count"] == 2
    keep = brec_f.numpy()[:4]
    assert keep[:, 0].tolist() == [0.0, 1.0, 2.0, 3.0]
    T = len(bop.TAUS)
    dia = np.asarray(full.diameter)[keep[:, 1].astype(int)]
    width = full.frame_hw[1]
    want = {"AR_VSD": np.mean([(keep[:, 2:2 + T] < t).sum() / (5 * T) for t in bop.THETAS]),
            "AR_MSSD": np.mean([(keep[:, 2 + T] < t * dia).sum() / 5 for t in bop.THETAS]),
            "AR_MSPD": np.mean([(keep[:, 3 + T] < t * (width / 640.0)).sum() / 5 for t in bop.THETAS_PX])}
    print("full-run correct shares over 5 targets:", want, " epoch without the row:",
          {k: out["bop"][k] for k in want}, " full epoch:", {k: ref["bop"][k] for k in want})
    for k, v in want.items():
        assert out["bop"][k] == float(v), k
    assert out["bop"]["AR"] == (out["bop"]["AR_VSD"] + out["bop"]["AR_MSSD"] + out["bop"]["AR_MSPD"]) / 3.0


def test_csv_score_column(dev, tiny, tmp_path):
    """The CSV's score column: the detections' scores; with select="depth" the verification scores, as without
    detections."""
    rows = bop_scene.gt_detections(_ds(tiny, True).tree)
    scores = [0.9, 0.25, 0.5, 0.125, 0.75]
    for r, s in zip(rows, scores):
        r["score"] = s
    m = _model(dev, 3)
    p_det, p_sel, p_png = (str(tmp_path / f"krrn_{k}-test.csv") for k in ("det", "sel", "png"))
    _reset()
    plain = run_epoch(m, _ds(tiny, True, detections=rows), bs=3, device=dev, bop=True)
    _reset()
    out = run_epoch(m, _ds(tiny, True, detections=rows), bs=3, device=dev, bop=True, bop_csv=p_det)
    _same(plain, out)                                            # bop_csv changes no returned number
    got = bop_scene.read_results(p_det)
    ds = _ds(tiny, True, detections=rows)
    assert [(r["scene_id"], r["im_id"], r["obj_id"]) for r in got] == [(it["scene"], it["im"], it["obj"]) for it in ds.tree.items]
    assert [r["score"] for r in got] == scores and all(r["time"] == -1.0 for r in got)
    _reset()
    run_epoch(m, _ds(tiny, True, detections=rows), bs=3, device=dev, bop=True, bop_csv=p_sel, select="depth")
    _reset()
    run_epoch(m, _ds(tiny, True), bs=3, device=dev, bop=True, bop_csv=p_png, select="depth")
    sel, png = bop_scene.read_results(p_sel), bop_scene.read_results(p_png)
    assert [r["score"] for r in sel] == [r["score"] for r in png] and all(0.0 <= r["score"] <= 1.0 for r in sel)
    assert [r["score"] for r in sel] != scores
    for a, b in zip(sel, png):
        assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"])
