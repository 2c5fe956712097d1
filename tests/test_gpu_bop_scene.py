"""BOP-layout scenes on the GPU: krrn_bop_visib_u8 through bop.visibility against its numpy f64 restatement
(tests/bop_scene_ref.py), bop_scene.write_gt_info on the tiny tree of tests/bop_tree.py, PoseDataset(layout="bop")
against the LineMOD layout on twin trees, masks="render", and the eval epoch's BOP result CSV.

Visibility: both planes, the 11 info ints and visib_fract are compared exactly, which the restatement's margins
license (no undecided pixel in any image of the family: test_bop_scene_host.py asserts it on the reference alone, and
_check again here); visib_fract is one f64 division of two of the integers, so bit equality is expected and asserted.
Images (frame, what each pins): stack / other / half (64 x 48: twelve whole tiles, planes whose rows are 16-byte
aligned, i.e. the row-store path; a partly and a fully occluded instance, holes in the observed depth, frame borders,
an instance behind the camera, an empty face range, a second camera matrix, depth_scale 0.5), ragged (50 x 41: tiles
cut by the right and bottom borders, rows not 16-byte aligned, i.e. the per-pixel store path), mixed (the nine
instances of the three 64 x 48 images in one launch over their three frames)."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import bop_scene_ref as sr
import bop_tree
from pose_estimation_amd import bop, bop_scene

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dt))


@pytest.fixture(scope="module")
def mesh(dev):
    v, f, rng = sr.concat_meshes()
    return _t(v, np.float32).to(dev), _t(f, np.int32).to(dev), rng


def _visib(dev, mesh, inst, frames, frame_idx, K4, face_range=None, **kw):
    """bop.visibility over `inst` (instance dicts of the family) as host numpy arrays."""
    v, f, rng = mesh
    fr = face_range if face_range is not None else [rng[i["obj"]] if len(i["faces"]) else (rng[i["obj"]][0], 0) for i in inst]
    out = bop.visibility(v, f, _t(fr, np.int32), _t(np.stack([i["R"] for i in inst]), np.float64),
                         _t(np.stack([i["t"] for i in inst]), np.float64), _t(K4, np.float32),
                         _t(frames, np.float32).to(dev), _t(frame_idx, np.int32), **kw)
    torch.cuda.synchronize()
    assert out["info"].dtype == torch.int32 and out["visib_fract"].dtype == torch.float64
    return {k: t.cpu().numpy() for k, t in out.items()}


def _image(dev, mesh, name, **kw):
    im = sr.image(name)
    n = len(im["inst"])
    return _visib(dev, mesh, im["inst"], im["depth"][None], [0] * n, np.tile(im["K4"], (n, 1)), **kw)


def _check(tag, got, b, ref):
    sr.check_conditions(ref)
    print(f"{tag}: info {got['info'][b].tolist()}  visib_fract {got['visib_fract'][b]!r}  "
          f"mask diff {int((got['mask'][b] != ref['mask']).sum())}  visib diff {int((got['mask_visib'][b] != ref['mask_visib']).sum())}")
    assert got["mask"].dtype == np.uint8 and got["mask"][b].max() <= 1 and got["mask_visib"][b].max() <= 1
    assert np.array_equal(got["mask"][b], ref["mask"].astype(np.uint8)), tag
    assert np.array_equal(got["mask_visib"][b], ref["mask_visib"].astype(np.uint8)), tag
    assert np.array_equal(got["info"][b], ref["info"]), (tag, got["info"][b].tolist(), ref["info"].tolist())
    assert np.array_equal(_bits(got["visib_fract"][b]), _bits(np.float64(ref["visib_fract"]))), tag


def _mixed(dev, mesh, order=None, **kw):
    inst, frames, fidx, K4 = [], [], [], []
    for k, name in enumerate(sr.IMAGES):
        im = sr.image(name)
        frames.append(im["depth"])
        for i in im["inst"]:
            inst.append(i), fidx.append(k), K4.append(im["K4"])
    order = list(range(len(inst))) if order is None else order
    return _visib(dev, mesh, [inst[j] for j in order], np.stack(frames), [fidx[j] for j in order],
                  np.stack([K4[j] for j in order]), **kw)


@pytest.mark.parametrize("name", sr.IMAGES + sr.EXTRA)
def test_visibility_image_parity(dev, mesh, name):
    got = _image(dev, mesh, name)
    for b, (i, ref) in enumerate(zip(sr.image(name)["inst"], sr.reference(name))):
        _check(f"{name}/{i['name']}", got, b, ref)


def test_visibility_mixed_batch_and_invariance(dev, mesh):
    """Nine instances over three frames with per-instance K4 in one launch: each equals its restatement, its own
    single-instance launch and the masks=False launch bit for bit, also with the batch permuted."""
    got = _mixed(dev, mesh)
    refs = [r for name in sr.IMAGES for r in sr.reference(name)]
    names = [f"{name}/{i['name']}" for name in sr.IMAGES for i in sr.image(name)["inst"]]
    assert len(refs) == 9
    for b, ref in enumerate(refs):
        _check(f"mixed[{b}] {names[b]}", got, b, ref)
    nomask = _mixed(dev, mesh, masks=False)
    assert set(nomask) == {"info", "visib_fract"}
    assert np.array_equal(nomask["info"], got["info"]) and np.array_equal(_bits(nomask["visib_fract"]), _bits(got["visib_fract"]))
    for b in range(9):
        one = _mixed(dev, mesh, order=[b])
        for k in ("mask", "mask_visib", "info", "visib_fract"):
            assert np.array_equal(_bits(one[k][0]), _bits(got[k][b])), (b, k)
    perm = [4, 8, 0, 3, 7, 1, 6, 2, 5]
    gp = _mixed(dev, mesh, order=perm)
    for k in ("mask", "mask_visib", "info", "visib_fract"):
        assert np.array_equal(_bits(gp[k]), _bits(got[k][perm])), k


def test_visibility_guards_and_delta(dev, mesh):
    im = sr.image("stack")
    inst, K4 = im["inst"], np.tile(im["K4"], (3, 1))
    base = _image(dev, mesh, "stack")
    for fi in (-1, 1, 7):                                        # a frame index outside [0, F) observes nothing
        got = _visib(dev, mesh, inst, im["depth"][None], [fi] * 3, K4)
        for b, i in enumerate(inst):
            ref = sr.visibility(i["verts"], i["faces"], i["R"], i["t"], im["K4"], np.zeros_like(im["depth"]))
            _check(f"frame {fi}/{i['name']}", got, b, ref)
            assert np.array_equal(got["mask_visib"][b], got["mask"][b]) and got["info"][b, 1] == 0
    F0, n = mesh[2][3]
    Ftot = int(mesh[1].shape[0])
    for bad in ((F0, 0), (-1, n), (F0, -4), (Ftot + 1, 4)):      # an empty or bad face range draws nothing
        got = _visib(dev, mesh, inst[:1], im["depth"][None], [0], K4[:1], face_range=[bad])
        assert not got["mask"].any() and not got["mask_visib"].any() and got["visib_fract"][0] == 0.0, bad
        assert got["info"][0].tolist() == [0, 0, 0] + [-1] * 8, bad
    # a larger delta sees the rear sphere through the front one's rim; equal to the restatement at that delta
    wide = _visib(dev, mesh, inst, im["depth"][None], [0] * 3, K4, delta=0.5)
    for b, i in enumerate(inst):
        ref = sr.visibility(i["verts"], i["faces"], i["R"], i["t"], im["K4"], im["depth"], delta=0.5)
        _check(f"delta 0.5/{i['name']}", wide, b, ref)
    assert wide["info"][2, 2] > 0 == base["info"][2, 2]          # the hidden tetrahedron counts as visible at 0.5 m
    # depth_scale: the raw uint16 image with 2000 raw units per metre, against the restatement at that scale (which
    # has no undecided pixel either: _check)
    half = sr.image("half")
    raw = _visib(dev, mesh, half["inst"], half["raw"].astype(np.float32)[None], [0] * 3, np.tile(half["K4"], (3, 1)),
                 depth_scale=1000.0 / half["depth_scale"])
    for b, i in enumerate(half["inst"]):
        ref = sr.visibility(i["verts"], i["faces"], i["R"], i["t"], half["K4"], half["raw"].astype(np.float32),
                            depth_scale=1000.0 / half["depth_scale"])
        _check(f"raw scale/{i['name']}", raw, b, ref)


def _png(path):
    with Image.open(path) as im:
        return np.array(im)


def test_write_gt_info_on_the_tiny_tree(dev, tmp_path):
    """A tree without scene_gt_info.json and mask folders gets the ones tests/bop_tree.py writes from the restatement."""
    root = str(tmp_path)
    w = bop_tree.write_tree(root, gt_info=False, masks=False)
    res = bop_scene.write_gt_info(root, "test", dev, masks=True, batch=4)    # scene 1's six instances: two batches
    for sc, per_im in w["info"].items():
        with open(os.path.join(root, "test", f"{sc:06d}", "scene_gt_info.json")) as f:
            on_disk = {int(k): v for k, v in json.load(f).items()}
        assert on_disk == per_im == res[sc], sc
        for entries in on_disk.values():
            assert all(set(e) == set(bop_scene.INFO_KEYS) for e in entries)
    for (sc, im, g), (m, mv) in w["masks"].items():
        for sub, exp in (("mask", m), ("mask_visib", mv)):
            got = _png(os.path.join(root, "test", f"{sc:06d}", sub, f"{im:06d}_{g:06d}.png"))
            assert got.dtype == np.uint8 and np.array_equal(got, exp.astype(np.uint8) * 255), (sc, im, g, sub)
    with pytest.raises(FileExistsError):
        bop_scene.write_gt_info(root, "test", dev)
    again = bop_scene.write_gt_info(root, "test", dev, overwrite=True, batch=64)
    assert again == res                                          # any batch size, with or without the planes
    assert len(bop_scene.BopTree(root, n_model_pts=4).items) == 5


# ------------------------------------------------------------------------------------------- dataset, epoch

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


def test_layout_equivalence(dev, tmp_path):
    """A LineMOD tree and its BOP twin: bitwise identical batches for every key (gt_maps and bop on) and identical
    test_epoch(bop=True) result dicts."""
    from pose_estimation_amd.dataset import PoseDataset
    from pose_estimation_amd.evaluate import test_epoch as run_epoch
    lm, bp = str(tmp_path / "lm"), str(tmp_path / "bop")
    bop_tree.write_twin(lm, bp)

    def pair(**kw):
        return (PoseDataset("test", 500, False, lm, 0.0, 8, cls_type="cat", n_model_pts=150, **kw),
                PoseDataset("test", 500, False, bp, 0.0, 8, cls_type="cat", n_model_pts=150, layout="bop", **kw))

    a, b = pair(gt_maps=True)
    assert len(a) == len(b) == 3 and a.boxes == b.boxes and a.objlist == b.objlist == [6] and a.diameter == b.diameter
    assert a.sym_obj == b.sym_obj == []
    for idx in ([0, 2], [1]):                                    # crop sizes 40, 40 and 80
        da, db = a.batch(idx, dev, bop=True), b.batch(idx, dev, bop=True)
        torch.cuda.synchronize()
        assert "xyz" in da and "bop_depth" in da and "region_point" in da
        _same(da, db)
    m = _model(dev, 1)
    a, b = pair(meshes=True)
    _reset()
    ra = run_epoch(m, a, bs=2, device=dev, bop=True)
    _reset()
    rb = run_epoch(m, b, bs=2, device=dev, bop=True)
    assert ra["test_count"] == 3 and ra["bop"]["count"] == 3
    _same(ra, rb)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("bop_tiny"))
    return root, bop_tree.write_tree(root)


def _tiny_ds(root, **kw):
    from pose_estimation_amd.dataset import PoseDataset
    return PoseDataset("test", 500, False, root, 0.0, 8, n_model_pts=4, layout="bop", **kw)


def test_rendered_masks_equal_the_pngs(dev, tiny):
    """masks="render" on the multi-instance tree: its PNGs come from the same definition, so every key is bitwise the
    same; the intrinsics are each image's own."""
    root, _ = tiny
    png, ren = _tiny_ds(root, meshes=True), _tiny_ds(root, meshes=True, masks="render")
    assert len(png) == len(ren) == 5
    for idx in ([0, 1, 2], [3, 4]):                              # the first batch holds two instances of one image
        da, db = png.batch(idx, dev, bop=True), ren.batch(idx, dev, bop=True)
        torch.cuda.synchronize()
        _same(da, db)
        assert int(da["mask_count"].min()) > 0
        K = da["intrinsic"].cpu().numpy()
        for j, i in enumerate(idx):
            assert np.array_equal(K[j], np.float32(png.tree.items[i]["K4"]))
    assert not np.array_equal(np.float32(png.tree.items[2]["K4"]), np.float32(png.tree.items[0]["K4"]))


def test_epoch_writes_the_result_csv(dev, tiny, tmp_path):
    from pose_estimation_amd.evaluate import POSE_REC, eval_records
    from pose_estimation_amd.evaluate import test_epoch as run_epoch
    root, _ = tiny
    m = _model(dev, 3)
    path = str(tmp_path / "krrn_tiny-test.csv")
    _reset()
    plain = run_epoch(m, _tiny_ds(root, meshes=True), bs=3, device=dev, bop=True)
    _reset()
    out = run_epoch(m, _tiny_ds(root, meshes=True), bs=3, device=dev, bop=True, bop_csv=path)
    _same(plain, out)                                            # bop_csv changes no returned number
    assert plain["test_count"] == plain["bop"]["count"] == 5 and set(plain["bop"]["per_obj"]) == {1, 2, 3}
    rows = bop_scene.read_results(path)
    ds = _tiny_ds(root, meshes=True)
    assert [(r["scene_id"], r["im_id"], r["obj_id"]) for r in rows] == [(it["scene"], it["im"], it["obj"]) for it in ds.tree.items]
    assert all(r["score"] == 1.0 and r["time"] == -1.0 for r in rows)
    _reset()
    buckets = {40: list(range(len(ds)))}
    rec, brec, poses = eval_records(m, ds, buckets, 3, dev, bop=True, poses=True)
    assert poses.shape == (5, len(POSE_REC)) == (5, 13) and poses.dtype == torch.float64
    assert poses[:, 0].tolist() == rec[:, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    for r, p in zip(rows, poses.numpy()):
        assert np.array_equal(_bits(r["R"].reshape(9)), _bits(p[1:10])) and np.array_equal(_bits(r["t"]), _bits(p[10:13] * 1000.0))
    _reset()
    rec2, brec2 = eval_records(m, _tiny_ds(root, meshes=True), buckets, 3, dev, bop=True)
    assert torch.equal(rec, rec2) and torch.equal(brec, brec2)   # poses=True changes no record
    Rm = poses[:, 1:10].reshape(5, 3, 3)
    assert torch.isfinite(poses).all() and (torch.linalg.det(Rm) - 1.0).abs().max() < 1e-4
    with pytest.raises(ValueError, match="layout='bop'"):
        from pose_estimation_amd.dataset import PoseDataset
        run_epoch(m, PoseDataset("test", 500, False, None, 0.0, 8, cls_type="all", num_frames=2), bs=2, device=dev,
                  bop_csv=path)
