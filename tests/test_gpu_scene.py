"""scene.render / overlay / depth_diff, bop_scene.vis_results and evaluate.test_epoch(vis_dir=...) on the GPU against
tests/scene_ref.py. The generic scenes are compared exactly on every pixel: each test asserts first that its scene has
no undecided pixel in the reference (scene_ref.check_conditions); the tie scene's answers are exact by construction.

  scene    frames        instances                                              what it pins
  overlap  1 of 40 x 72  3 overlapping spheres out of depth order, 1 behind     partial tiles, one object hiding another,
                         the camera, 1 off the frame                            culled and empty instances
  ties     2 of 48 x 64  a sphere twice under one pose; a dyadic grid 3 times   equal depths go to the lowest index
  frames   7 of 40 x 72  counts 2 (320 faces: two chunks), 0, 3, bad ranges     range guards, frames independent of the batch
"""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import bop_multi_tree as mt
import scene_ref as sf
from pose_estimation_amd import bop_scene, scene
from pose_estimation_amd.dataset import PoseDataset
from pose_estimation_amd.evaluate import test_epoch as run_epoch

pytestmark = pytest.mark.gpu


def _render(dev, sc, inst_range=None):
    res = scene.render(torch.from_numpy(sc["verts"]).to(dev), torch.from_numpy(sc["faces"]).to(dev), sc["face_range"],
                       sc["R"], sc["t"], sc["K4"], sc["inst_range"] if inst_range is None else inst_range, sc["H"], sc["W"])
    return {k: v.cpu().numpy() for k, v in res.items()}


def _equal(got, ref, where=""):
    assert got["inst"].dtype == np.int32 and got["depth"].dtype == np.float32 and got["shade"].dtype == np.uint8
    bad = got["inst"] != ref["inst"]
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert np.array_equal(got["shade"], ref["shade"]), where
    assert got["depth"].tobytes() == ref["depth"].astype(np.float32).tobytes(), where    # (float)z, bit for bit


def test_one_frame_of_overlapping_instances(dev):
    sc, ref = sf.scene("overlap"), sf.reference("overlap")
    sf.check_conditions(ref)
    assert set(np.unique(ref["inst"])) == {-1, 0, 1, 2}                  # 3 behind the camera, 4 off the frame
    hid = sf.render(sc["verts"], sc["faces"], sc["face_range"][:1], sc["R"][:1], sc["t"][:1], sc["K4"][:1], [(0, 1)],
                    sc["H"], sc["W"], margins=False)["inst"]
    assert ((hid == 0) & (ref["inst"] == 1)).any()                       # instance 1 hides part of instance 0
    _equal(_render(dev, sc), ref)


def test_exact_ties_go_to_the_lowest_index(dev):
    sc, ref = sf.scene("ties"), sf.reference("ties")
    got = _render(dev, sc)
    # frame 0: one sphere twice under one pose: the lower index on every covered pixel, and the planes of one copy
    assert set(np.unique(got["inst"][0])) == {-1, 0} and (got["inst"][0] == 0).sum() > 100
    one = _render(dev, sc, [(1, 1)])
    assert np.array_equal(one["inst"][0] >= 0, got["inst"][0] >= 0) and set(np.unique(one["inst"])) == {-1, 1}
    assert one["depth"].tobytes() == got["depth"][0].tobytes() and np.array_equal(one["shade"][0], got["shade"][0])
    alone = sf.render(sc["verts"], sc["faces"], sc["face_range"], sc["R"], sc["t"], sc["K4"], [(1, 1)], sc["H"], sc["W"])
    sf.check_conditions(alone)                                           # the copy on its own is a generic scene
    _equal(one, alone, "sphere")
    # frame 1: every coordinate dyadic, every depth exactly 1: equal to the reference without margins
    assert set(np.unique(ref["inst"][1])) == {-1, 2, 3} and set(np.unique(ref["z"][1])) == {0.0, 1.0}
    _equal({k: v[1] for k, v in got.items()}, {k: v[1] for k, v in ref.items()}, "grid")
    assert (got["inst"][1][8:41, 24:49] == 2).all() and (got["inst"][1][8:41, 16:24] == 3).all()
    assert (got["shade"][1][got["inst"][1] >= 0] == 255).all()


def test_three_frames_and_bad_ranges(dev):
    sc, ref = sf.scene("frames"), sf.reference("frames")
    sf.check_conditions(ref)
    assert [int((p >= 0).any()) for p in ref["inst"]] == [1, 0, 1, 0, 0, 1, 0]
    assert sc["face_range"][0][1] == 320                                 # two face chunks
    got = _render(dev, sc)
    _equal(got, ref)
    assert set(np.unique(got["inst"][5])) == {-1, 4}                     # (4, 5) is cut at N = 5
    for f, row in enumerate(sc["inst_range"]):                           # alone = in the batch, bit for bit
        alone = _render(dev, sc, [tuple(int(x) for x in row)])
        for k in ("inst", "depth", "shade"):
            assert alone[k][0].tobytes() == got[k][f].tobytes(), (f, k)
    # no instance at all: the empty planes, written without a memset
    none = scene.render(torch.from_numpy(sc["verts"]).to(dev), torch.from_numpy(sc["faces"]).to(dev), [], np.zeros((0, 9)),
                        np.zeros((0, 3)), np.zeros((0, 4), np.float32), [(0, 0), (0, 3)], 40, 72)
    assert (none["inst"] == -1).all() and not none["depth"].any() and not none["shade"].any()


def test_overlay_and_depth_diff(dev):
    sc, ref = sf.scene("overlap"), sf.reference("overlap")
    rng = np.random.default_rng(17)
    F, H, W = 1, sc["H"], sc["W"]
    rgb = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    tint = scene.palette([1, 2, 3, 4, 5])
    est, shade = ref["inst"].astype(np.int32), ref["shade"]
    gt = np.roll(est, (2, -3), (1, 2))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    for alpha, radius, g in ((128, 1, gt), (128, 4, None), (0, 1, None), (256, 4, gt), (77, 2, None)):
        got = scene.overlay(up(rgb), up(est), up(shade), tint, alpha, radius, gt=None if g is None else up(g),
                            gt_colour=(9, 250, 31)).cpu().numpy()
        assert np.array_equal(got, sf.overlay(rgb, est, shade, tint, alpha, radius, g, (9, 250, 31))), (alpha, radius)
    # random id planes: ids outside [0, N) on both sides, every pixel an edge candidate; three frames
    F = 3
    rgb = rng.integers(0, 256, (F, 23, 37, 3), dtype=np.uint8)
    est = rng.integers(-2, 7, (F, 23, 37)).astype(np.int32)
    est[1] = np.repeat(np.repeat(rng.integers(-1, 5, (6, 10)), 4, 0), 4, 1)[:23, :37]    # blocks: interiors and borders
    gt = np.repeat(np.repeat(rng.integers(-1, 3, (F, 5, 8)), 5, 1), 5, 2)[:, :23, :37].astype(np.int32)
    shade = rng.integers(0, 256, (F, 23, 37), dtype=np.uint8)
    for alpha, radius, g in ((128, 1, gt), (200, 4, gt), (31, 1, None), (128, 4, None)):
        got = scene.overlay(up(rgb), up(est), up(shade), torch.from_numpy(tint).to(dev), alpha, radius,
                            gt=None if g is None else up(g)).cpu().numpy()
        assert np.array_equal(got, sf.overlay(rgb, est, shade, tint, alpha, radius, g)), (alpha, radius)
    # depth_diff: the rendered depth against an observed one with holes, a NaN, a negative and exact agreement
    ren = ref["depth"]
    obs = (ren.astype(np.float64) + rng.uniform(-0.03, 0.03, ren.shape)).astype(np.float32)
    obs[ren == 0] = (0.9 + 0.2 * rng.random(int((ren == 0).sum()))).astype(np.float32)
    ys, xs = np.nonzero(ren[0] > 0)
    obs[0, ys[:40], xs[:40]] = 0.0
    obs[0, ys[40], xs[40]] = np.nan
    obs[0, ys[41], xs[41]] = -0.5
    obs[0, ys[42:60], xs[42:60]] = ren[0, ys[42:60], xs[42:60]]
    for scale, tol in ((1.0, 0.02), (1.0, 0.005), (0.5, 0.02)):
        got = scene.depth_diff(up(ren), up(obs), scale, tol).cpu().numpy()
        want = sf.depth_diff(ren, obs, scale, tol)
        assert np.array_equal(got, want), (scale, tol)
    assert {tuple(c) for c in want.reshape(-1, 3)} >= {(0, 0, 0), (128, 128, 128)}
    want = sf.depth_diff(ren, obs)
    assert (want[0, ys[42], xs[42]] == 255).all() and (want[0, ys[40], xs[40]] == 128).all()
    with pytest.raises(ValueError, match="alpha"):
        scene.overlay(up(rgb), up(est), up(shade), tint, alpha=257)
    with pytest.raises(ValueError, match="radius"):
        scene.overlay(up(rgb), up(est), up(shade), tint, radius=5)
    with pytest.raises(ValueError, match="tol"):
        scene.depth_diff(up(ren), up(obs), tol=0.0)


# ----------------------------------------------------------------------------------------------- pictures of a tree

def _ds(root, **kw):
    return PoseDataset("test", 500, False, root, 0.0, 8, n_model_pts=4, layout="bop", meshes=True, **kw)


@pytest.fixture(scope="module")
def multi(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("scene_multi"))
    return root, mt.write_tree(root)


def composite(ds, rows, tol=0.02):
    """What vis_results must write, from scene_ref: {(scene, im): (overlay u8 [H, W, 3], diff u8 [H, W, 3])}. Asserts
    that neither the estimates' scene nor the ground truth's has an undecided pixel."""
    tree = ds.tree
    cam = {(int(it["scene"]), int(it["im"])): (it["K4"], float(it["depth_scale"])) for it in tree.instances}
    objs = sorted(tree.mesh)
    verts, faces, rng = sf.concat([tree.mesh[o] for o in objs])
    out = {}
    for key in dict.fromkeys((int(r["scene_id"]), int(r["im_id"])) for r in rows):
        if key not in cam:
            continue
        rgb, depth = tree.read_image(key[0], key[1], cam[key][1])
        H, W = depth.shape
        est = [(int(r["obj_id"]), np.asarray(r["R"], np.float64).reshape(9), np.asarray(r["t"], np.float64) / 1000.0)
               for r in rows if (int(r["scene_id"]), int(r["im_id"])) == key]
        gt = [(int(it["obj"]), np.asarray(it["R"]).reshape(9), np.asarray(it["t"])) for it in tree.instances
              if (int(it["scene"]), int(it["im"])) == key]
        res = []
        for inst in (est, gt):
            r = sf.render(verts, faces, [rng[objs.index(o)] for o, _, _ in inst], [R for _, R, _ in inst],
                          [t for _, _, t in inst], [cam[key][0]] * len(inst), [(0, len(inst))], H, W)
            sf.check_conditions(r)
            res.append(r)
        pic = sf.overlay(rgb[None], res[0]["inst"], res[0]["shade"], scene.palette([o for o, _, _ in est]), 128, 1,
                         res[1]["inst"])
        out[key] = (pic[0], sf.depth_diff(res[0]["depth"], depth[None], 1.0, tol)[0])
    return out


def _png(path):
    with Image.open(path) as im:
        return np.array(im)


def test_vis_results(dev, multi, tmp_path):
    root, made = multi
    ds = _ds(root)
    rows, meta = mt.result_rows(made)
    want = composite(ds, rows)
    assert sorted(want) == [(1, 0), (1, 1)]
    out = str(tmp_path / "vis")
    st = bop_scene.vis_results(ds, rows, out, dev, diff=True, chunk_images=1)
    assert st == {"images": 2, "drawn": len(rows) - 1, "ignored": 1}     # the row of an image the tree does not hold
    for (sc, im), (pic, diff) in want.items():
        assert np.array_equal(_png(os.path.join(out, f"{sc:06d}", f"{im:06d}.png")), pic), (sc, im)
        assert np.array_equal(_png(os.path.join(out, f"{sc:06d}", f"{im:06d}_diff.png")), diff), (sc, im)
    assert sorted(os.listdir(os.path.join(out, "000001"))) == ["000000.png", "000000_diff.png", "000001.png",
                                                               "000001_diff.png"]
    rgb0 = ds.tree.read_image(1, 0, 1.0)[0]
    assert (want[(1, 0)][0] != rgb0).any(2).sum() > 200 and (want[(1, 0)][0] == (0, 255, 0)).all(2).sum() > 50
    # a second call refuses to overwrite, before anything is written, and leaves the files as they were
    stamp = {n: os.stat(os.path.join(out, "000001", n)).st_mtime_ns for n in os.listdir(os.path.join(out, "000001"))}
    with pytest.raises(FileExistsError):
        bop_scene.vis_results(ds, rows[::-1], out, dev, gt=False)
    assert stamp == {n: os.stat(os.path.join(out, "000001", n)).st_mtime_ns for n in stamp}
    assert np.array_equal(_png(os.path.join(out, "000001", "000000.png")), want[(1, 0)][0])
    # overwrite=True, both images in one chunk, no outline layer: the estimates' overlay alone
    st = bop_scene.vis_results(ds, rows, out, dev, gt=False, overwrite=True)
    assert st == {"images": 2, "drawn": len(rows) - 1, "ignored": 1}
    got = _png(os.path.join(out, "000001", "000000.png"))
    assert not np.array_equal(got, want[(1, 0)][0])
    assert bop_scene.vis_results(ds, [], str(tmp_path / "none"), dev) == {"images": 0, "drawn": 0, "ignored": 0}


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


def test_epoch_writes_pictures(dev, multi, tmp_path):
    root, _ = multi
    m = _model(dev, 3)
    out, csv = str(tmp_path / "vis"), str(tmp_path / "rows.csv")
    _reset()
    res = run_epoch(m, _ds(root), bs=4, device=dev, bop_csv=csv, vis_dir=out, vis_diff=True)
    assert res["vis"] == {"images": 2, "drawn": 7, "ignored": 0}
    assert sorted(os.listdir(os.path.join(out, "000001"))) == ["000000.png", "000000_diff.png", "000001.png",
                                                               "000001_diff.png"]
    assert _png(os.path.join(out, "000001", "000001.png")).shape == (mt.H, mt.W, 3)
    # the pictures are vis_results of the rows that bop_csv wrote
    again = str(tmp_path / "again")
    bop_scene.vis_results(_ds(root), bop_scene.read_results(csv), again, dev, diff=True)
    for n in os.listdir(os.path.join(out, "000001")):
        assert np.array_equal(_png(os.path.join(out, "000001", n)), _png(os.path.join(again, "000001", n))), n
    # every other key is what it is without vis_dir, bit for bit, and the default adds no key
    _reset()
    base = run_epoch(m, _ds(root), bs=4, device=dev)
    assert "vis" not in base
    _same({k: v for k, v in res.items() if k != "vis"}, base)
