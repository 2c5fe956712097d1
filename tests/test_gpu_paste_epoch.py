"""evaluate.test_epoch(seg_json=..., seg_source="net") on the tiny BOP tree of tests/bop_tree.py with the w18 model:
the file against tests/paste_ref.py + rle.encode over the mask head's logits, which a forward hook copies to the host
with each call's class ids (exact: integer output), the epoch's other keys against a run without seg_json, the
"render" default, a dataset without meshes, and a second pass's dataset built on the file."""
import numpy as np
import pytest
import torch

import bop_tree
import paste_ref as pr
import rle_ref as rf
from pose_estimation_amd import bop_scene, rle
from pose_estimation_amd import distributed as kd
from pose_estimation_amd.dataset import PoseDataset
from pose_estimation_amd.evaluate import _batches
from pose_estimation_amd.evaluate import test_epoch as run_epoch

pytestmark = pytest.mark.gpu

SEED = 0                                                 # init_weights' seed: test_the_file_is_not_vacuous holds it to account
BS = 3


def _ds(root, meshes=True, **kw):
    return PoseDataset("test", 500, False, root, 0.0, 8, n_model_pts=4, layout="bop", meshes=meshes, **kw)


def _reset():
    from pose_estimation_amd import pose as kpose
    torch.manual_seed(5)
    kpose._seeds.clear()


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


def _plane(seg):
    return rf.decode(seg["counts"], *seg["size"])


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    """One plain epoch and one with seg_source="net" on the same model, the second under a forward hook."""
    from pose_estimation_amd import KRRN, make_config
    from pose_estimation_amd.synthetic import init_weights
    tmp = tmp_path_factory.mktemp("paste_epoch")
    root = str(tmp / "tree")
    bop_tree.write_tree(root)
    m = KRRN(cfg=make_config(num_cls=3, backbone="w18"))
    init_weights(m, SEED)
    m = m.to(dev).eval()
    seg, csv = str(tmp / "krrn_tiny-test_seg.json"), str(tmp / "krrn_tiny-test.csv")
    _reset()
    plain = run_epoch(m, _ds(root), bs=BS, device=dev, bop=True)
    calls = []

    def hook(module, args, pred):
        calls.append((pred["mask"].detach().clone().cpu().numpy(), args[3].detach().cpu().numpy().reshape(-1)))

    h = m.register_forward_hook(hook)
    try:
        _reset()
        out = run_epoch(m, _ds(root), bs=BS, device=dev, bop=True, bop_csv=csv, seg_json=seg, seg_source="net")
    finally:
        h.remove()
    return {"root": root, "model": m, "plain": plain, "out": out, "calls": calls, "seg": seg, "csv": csv, "tmp": tmp}


def _reference(run):
    """(detection rows, per-crop windows, stats) from the hooked logits: paste_ref + rle.encode + net_mask_rows."""
    ds = _ds(run["root"])
    H, W = ds.frame_hw
    sizes = [ds.crop_size(i) for i in range(len(ds))]
    batches = list(_batches(kd.bucket_shard(sizes, 1, 0), BS))
    assert len(batches) == len(run["calls"]) and sum(len(idx) for _, idx in batches) == len(ds)
    runs, info, win = {}, {}, {}
    for (S, idx), (logits, cls) in zip(batches, run["calls"]):
        assert logits.shape == (len(idx), 4, S, S) and logits.dtype == np.float32     # background + 3 classes
        assert cls.tolist() == [ds.objlist.index(int(ds.tree.items[i]["obj"])) for i in idx]
        rc = [(ds.boxes[i][0], ds.boxes[i][2]) for i in idx]
        mask, q = pr.paste(logits, cls + 1, rc, H, W)
        for k, i in enumerate(idx):
            runs[i], info[i], win[i] = rle.encode(mask[k]), q[k], (rc[k][0], rc[k][1], S)
    rows = bop_scene.read_results(run["csv"])
    assert [(r["scene_id"], r["im_id"], r["obj_id"]) for r in rows] == [(it["scene"], it["im"], it["obj"]) for it in ds.tree.items]
    order = list(range(len(ds)))
    det, st = bop_scene.net_mask_rows(rows, [runs[i] for i in order], [info[i] for i in order], H, W)
    return det, [win[i] for i in order if info[i][0] > 0], st, info


def test_the_file_is_the_reference(run):
    want, windows, st, info = _reference(run)
    det = bop_scene.read_detections(run["seg"])
    out = run["out"]
    print("seg:", out["seg"], "pixels per crop:", [int(info[i][0]) for i in sorted(info)],
          "runs per row:", [len(d["segmentation"]["counts"]) for d in det])
    assert det == want
    assert out["seg"] == {"rows": len(det), "empty": st["empty"]} and len(det) + st["empty"] == out["test_count"] == 5
    H, W = _ds(run["root"]).frame_hw
    for d, (rmin, cmin, S) in zip(det, windows):
        assert d["segmentation"]["size"] == [H, W] and d["time"] == -1.0 and d["score"] == 1.0
        p = _plane(d["segmentation"])
        inside = np.zeros((H, W), bool)
        inside[max(rmin, 0):max(rmin + S, 0), max(cmin, 0):max(cmin + S, 0)] = True
        assert p.any() and not p[~inside].any()
        assert d["bbox"] == [float(v) for v in rf.info(p)[1:5]]


def test_the_file_is_not_vacuous(run):
    """Seed SEED's weights must leave a real segmentation: at least one row, and a row that is neither empty nor its
    whole window."""
    det = bop_scene.read_detections(run["seg"])
    px = [int(_plane(d["segmentation"]).sum()) for d in det]
    S = _ds(run["root"]).crop_size(0)
    print(f"seed {SEED}: {len(det)} rows, pixels {px}, window {S} x {S}")
    assert len(det) >= 1 and any(0 < n < S * S for n in px)


def test_no_other_key_changes(run):
    out, plain = run["out"], run["plain"]
    assert set(out) - set(plain) == {"seg"} and set(out["seg"]) == {"rows", "empty"}
    _same({k: v for k, v in out.items() if k != "seg"}, plain)


def test_render_is_the_default(run, dev):
    root, m, tmp = run["root"], run["model"], run["tmp"]
    a, b = str(tmp / "default.json"), str(tmp / "render.json")
    _reset()
    out_a = run_epoch(m, _ds(root), bs=BS, device=dev, seg_json=a)
    _reset()
    out_b = run_epoch(m, _ds(root), bs=BS, device=dev, seg_json=b, seg_source="render")
    with open(a, "rb") as fa, open(b, "rb") as fb:
        assert fa.read() == fb.read()
    _same(out_a, out_b)


def test_net_needs_no_meshes(run, dev):
    root, m, tmp = run["root"], run["model"], run["tmp"]
    path = str(tmp / "nomesh.json")
    _reset()
    out = run_epoch(m, _ds(root, meshes=False), bs=BS, device=dev, seg_json=path, seg_source="net")
    assert out["seg"] == run["out"]["seg"] and "bop" not in out
    assert bop_scene.read_detections(path) == bop_scene.read_detections(run["seg"])   # the masks do not depend on the pose


def test_second_pass(run, dev):
    """A dataset built on the file: its batch's verify_mask planes are the file's decoded masks."""
    det = bop_scene.read_detections(run["seg"])
    ds2 = _ds(run["root"], detections=run["seg"])
    usable = [d for d in det if d["bbox"][2] > 0 and d["bbox"][3] > 0]
    assert len(ds2) == len(usable) and ds2.tree.det_stats["rows"] == len(det)
    assert len(ds2) >= 1
    idx = [i for i in range(len(ds2)) if ds2.crop_size(i) == ds2.crop_size(0)]
    b = ds2.batch(idx, dev, verify=True)
    torch.cuda.synchronize()
    for j, i in enumerate(idx):
        d = det[ds2.tree.items[i]["det"]]
        assert np.array_equal(b["verify_mask"][j].cpu().numpy(), _plane(d["segmentation"])), i
        assert np.array_equal(b["det_info"][j].cpu().numpy(), rf.info(_plane(d["segmentation"]))), i
