"""BOP-layout scenes without a GPU: the numpy restatement of GT visibility (tests/bop_scene_ref.py) on its scene
family (zero undecided pixels, what each instance pins, a ray-cast cross-check of its depth images), the BopTree index
over the tiny tree of tests/bop_tree.py, the result CSV's round trip, the host-side argument checks of
krrn_bop_visib_u8 (they run before any HIP call) and PoseDataset's layout="bop" constructor errors."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import bop_scene_ref as sr
import bop_tree
import raster_ref as rr
from pose_estimation_amd import _lib, bop, bop_scene
from pose_estimation_amd.dataset import PoseDataset, get_square_bbox


# ------------------------------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("name", sr.IMAGES + sr.EXTRA)
def test_family_conditions(name):
    """Zero undecided pixels in every image of the family: a condition, not a tolerance."""
    im, refs = sr.image(name), sr.reference(name)
    assert im["raw"].dtype == np.uint16 and im["depth"].dtype == np.float32 and len(refs) == 3
    for i, r in zip(im["inst"], refs):
        print(name, i["name"], r["info"].tolist(), r["visib_fract"], {k: float(v.min()) for k, v in r["margins"].items()})
        sr.check_conditions(r)
        assert r["info"][2] <= r["info"][0] and r["info"][1] <= r["info"][0]


def test_family_pins_what_it_says():
    by = {i["name"]: (i, r, sr.image(n)) for n in sr.IMAGES + sr.EXTRA for i, r in zip(sr.image(n)["inst"], sr.reference(n))}
    front, rear, hidden = by["front"][1], by["rear"][1], by["hidden"][1]
    assert front["visib_fract"] == 1.0 and 0.1 < rear["visib_fract"] < 0.9         # the front sphere hides part of the rear
    assert (rear["mask"] & ~rear["mask_visib"] & front["mask"]).any()
    assert hidden["info"][0] > 0 and hidden["info"][2] == 0 and hidden["info"][7:].tolist() == [-1] * 4
    assert hidden["visib_fract"] == 0.0 and not (hidden["mask"] & ~front["mask"]).any()
    hole = front["mask"] & (by["front"][2]["depth"] == 0)                           # the obs == 0 rule
    assert hole.sum() >= 5 and front["mask_visib"][hole].all() and front["info"][1] == front["info"][0] - hole.sum()
    border = by["border"][1]
    assert border["info"][3] == 0 and border["info"][4] == 0 and border["info"][0] > 50   # cut by the left and top borders
    b2 = by["border2"][1]
    assert b2["info"][3] + b2["info"][5] == sr.W - 1 and 0 < b2["visib_fract"] < 0.1      # the right border; under min_visib
    for k in ("behind", "norange"):
        assert not by[k][1]["info"][:3].any() and by[k][1]["info"][3:].tolist() == [-1] * 8 and by[k][1]["visib_fract"] == 0.0
    assert by["behind"][0]["t"][2] < 0 and len(by["norange"][0]["faces"]) == 0
    assert by["plain2"][2]["depth_scale"] == 0.5 and tuple(by["plain"][2]["K4"]) != tuple(by["front"][2]["K4"])
    assert (sr.image("ragged")["H"], sr.image("ragged")["W"]) == (41, 50)
    assert sr.bbox(np.zeros((4, 4), bool)) == [-1] * 4 and sr.bbox(np.eye(4, dtype=bool)[:, :1]) == [0, 0, 0, 0]


@pytest.mark.parametrize("name", ["stack", "ragged"])
def test_visibility_against_ray_casting(name):
    """The same planes, counts and boxes from depth images made by 3-D ray / triangle intersection, which shares no
    code with the rasteriser's 2-D edge functions (every instance of these images lies in front of the camera)."""
    im = sr.image(name)
    S = max(im["H"], im["W"])
    for i, ref in zip(im["inst"], sr.reference(name)):
        _, d = rr.raycast(i["verts"], i["faces"], i["R"], i["t"], im["K4"], 0, 0, S)
        d = d[:im["H"], :im["W"]]
        assert np.abs(d - ref["depth"]).max() < 1e-12
        res = sr.visibility(i["verts"], i["faces"], i["R"], i["t"], im["K4"], im["depth"], image=d)
        assert np.array_equal(res["mask"], ref["mask"]) and np.array_equal(res["mask_visib"], ref["mask_visib"])
        assert np.array_equal(res["info"], ref["info"]) and res["visib_fract"] == ref["visib_fract"]


# ------------------------------------------------------------------------------------------ the index

@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("bop_host"))
    return root, bop_tree.write_tree(root)


def _key(it):
    return (it["scene"], it["im"], it["gt"])


def test_boptree_index(tree):
    root, w = tree
    t = bop_scene.BopTree(root, n_model_pts=4, meshes=True)
    # hidden (px_count_visib 0), behind (visib_fract 0) and border2 (under 0.1) are dropped: BOP-19's rule
    assert [_key(it) for it in t.items] == [(1, 3, 0), (1, 3, 1), (1, 7, 0), (1, 7, 2), (2, 0, 1)]
    assert [it["obj"] for it in t.items] == [3, 2, 3, 1, 3] and t.objlist == [1, 2, 3] and t.frame_hw == (sr.H, sr.W)
    for it in t.items:
        name = {im_id: nm for nm, im_id in bop_tree.SCENES[it["scene"]]}[it["im"]]
        im = sr.image(name)
        inst = im["inst"][it["gt"]]
        assert np.array_equal(it["R"], inst["R"]) and np.array_equal(it["t"], np.asarray([x * 1000.0 for x in inst["t"]]) / 1000.0)
        assert np.array_equal(np.float32(it["K4"]), im["K4"]) and it["depth_scale"] == im["depth_scale"]   # per image
        assert it["bbox"] == [float(x) for x in w["info"][it["scene"]][it["im"]][it["gt"]]["bbox_visib"]]
    assert {it["K4"] for it in t.items} == {tuple(float(k) for k in np.float32(sr.K_TINY)), sr.K_OTHER}
    i = [_key(it) for it in t.items].index((2, 0, 1))
    rgb, depth, ml = t.read(i)                                   # depth_scale 0.5 applied; the instance's own mask
    assert rgb.shape == (sr.H, sr.W, 3) and rgb.dtype == np.uint8
    assert depth.dtype == np.float32 and np.array_equal(depth, sr.image("half")["depth"])
    assert ml.dtype == np.uint8 and np.array_equal(ml.astype(bool), w["masks"][(2, 0, 1)][1])
    assert t.mesh[3][1].shape == (320, 3) and t.model_points[1].shape == (4, 3)
    assert t.symmetries[2].shape == (2, 12) and t.symmetries[3].shape == (1, 12)
    assert t.has_symmetry(2) and not t.has_symmetry(1)
    # min_visib
    assert len(bop_scene.BopTree(root, n_model_pts=4, min_visib=0.0).items) == 6            # border2 comes back; hidden and
    assert len(bop_scene.BopTree(root, n_model_pts=4, min_visib=0.7).items) == 4            # behind never do; rear leaves
    # targets
    with open(w["targets"]) as f:
        tg = json.load(f)
    assert {"scene_id", "im_id", "obj_id", "inst_count"} == set(tg[0])
    sub = os.path.join(root, "some_targets.json")
    with open(sub, "w") as f:
        json.dump([e for e in tg if (e["scene_id"], e["im_id"], e["obj_id"]) in ((1, 3, 2), (2, 0, 3), (1, 7, 2))], f)
    t2 = bop_scene.BopTree(root, targets=sub, n_model_pts=4)
    assert [_key(it) for it in t2.items] == [(1, 3, 1), (2, 0, 1)] and t2.objlist == [2, 3]  # (1, 7, 2) is `behind`
    assert [_key(it) for it in bop_scene.BopTree(root, n_model_pts=4, objlist=[1]).items] == [(1, 7, 2)]
    with pytest.raises(ValueError, match="num_pt_mesh_large"):
        bop_scene.BopTree(root)                                  # the tetrahedron has 4 vertices < 2600


def test_boptree_missing_gt_info(tmp_path):
    root = str(tmp_path)
    bop_tree.write_tree(root, gt_info=False, masks=False)
    with pytest.raises(FileNotFoundError, match="write_gt_info"):
        bop_scene.BopTree(root, n_model_pts=4)


def test_binary_ply_keeps_raising(tmp_path):
    root = str(tmp_path)
    bop_tree.write_tree(root)
    with open(os.path.join(root, "models", "obj_000002.ply"), "w") as f:
        f.write("ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nend_header\n")
    with pytest.raises(ValueError, match="ascii"):
        bop_scene.BopTree(root, n_model_pts=4)


# ------------------------------------------------------------------------------------------ results

def test_results_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    rows = [{"scene_id": int(rng.integers(1, 50)), "im_id": int(rng.integers(0, 2000)), "obj_id": int(rng.integers(1, 16)),
             "score": float(rng.random()), "R": rr.rotation(rng), "t": rng.standard_normal(3) * 1000.0 / 3.0,
             "time": float(rng.random()) if k % 2 else -1.0} for k in range(20)]
    rows[3]["t"] = np.array([1e-310, -0.0, 1.0 / 3.0])           # a denormal, a signed zero
    p = str(tmp_path / "krrn_tiny-test.csv")
    bop_scene.write_results(p, rows)
    with open(p) as f:
        head = f.readline().strip()
        first = f.readline().strip().split(",")
    assert head == "scene_id,im_id,obj_id,score,R,t,time" and len(first) == 7
    assert len(first[4].split()) == 9 and len(first[5].split()) == 3
    back = bop_scene.read_results(p)
    assert len(back) == len(rows)
    for a, b in zip(rows, back):
        assert (a["scene_id"], a["im_id"], a["obj_id"]) == (b["scene_id"], b["im_id"], b["obj_id"])
        for k in ("score", "time"):
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes()
        for k in ("R", "t"):
            assert np.asarray(a[k], np.float64).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k   # bit for bit
    assert back[0]["R"].shape == (3, 3)
    with open(p, "w") as f:
        f.write("scene,im\n")
    with pytest.raises(ValueError, match="first line"):
        bop_scene.read_results(p)


# ------------------------------------------------------------------------------------------ host checks

def _fakes(names):
    """Distinct, far-apart non-null pointers (never dereferenced: the checks fail before any launch)."""
    return {k: ctypes.c_void_p((i + 1) << 36) for i, k in enumerate(names)}


def test_visib_host_side_errors():
    fn = _lib.lib().krrn_bop_visib_u8
    N, D = ctypes.c_void_p(0), ctypes.c_double
    names = ("verts", "faces", "face_range", "R", "t", "K4", "depth", "frame", "ws", "mask", "mask_visib", "info",
             "visib_fract")

    def call(V=10, Ft=4, F=2, H=48, W=64, scale=1.0, delta=0.015, B=2, **over):
        p = _fakes(names)
        p.update(over)
        return fn(p["verts"], V, p["faces"], Ft, p["face_range"], p["R"], p["t"], p["K4"], p["depth"], F, H, W,
                  p["frame"], D(scale), D(delta), B, p["ws"], p["mask"], p["mask_visib"], p["info"], p["visib_fract"], N)

    for k in names:
        if k not in ("mask", "mask_visib"):                      # the two planes are optional
            assert call(**{k: N}) == -1, k
    f = _fakes(names)
    assert call(mask=f["mask_visib"]) == -1                      # two outputs on one buffer
    assert call(mask_visib=ctypes.c_void_p(f["mask"].value + 2 * 48 * 64 - 1)) == -1   # the last byte of `mask`
    assert call(info=f["visib_fract"]) == -1 and call(visib_fract=ctypes.c_void_p(f["info"].value + 44 * 2 - 4)) == -1
    assert call(info=f["R"]) == -1 and call(ws=f["frame"]) == -1 and call(mask=f["depth"]) == -1   # an output on an input
    assert call(visib_fract=ctypes.c_void_p(f["ws"].value + 4 * 2 * bop.VISIB_WS - 4)) == -1       # the last ws int
    assert call(delta=0.0) == -2 and call(delta=-0.015) == -2 and call(delta=float("nan")) == -2
    assert call(scale=0.0) == -2 and call(scale=-1.0) == -2 and call(scale=float("nan")) == -2
    assert call(B=0) == -2 and call(V=0) == -2 and call(H=0) == -2 and call(W=0) == -2 and call(F=0) == -2
    assert call(Ft=-1) == -2
    assert call(B=0, info=N) == -1                               # pointers are checked first
    n = ctypes.c_longlong(0)
    ws = _lib.lib().krrn_bop_visib_ws
    assert ws(3, ctypes.byref(n)) == 0 and n.value == 3 * bop.VISIB_WS
    assert ws(0, ctypes.byref(n)) == -2 and ws(3, N) == -1


def test_abi_lists_the_entry_points():
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert _lib.SIGNATURES["krrn_bop_visib_u8"] == [P, I, P, I, P, P, P, P, P, I, I, I, P, D, D, I, P, P, P, P, P, P]
    assert _lib.SIGNATURES["krrn_bop_visib_ws"] == [I, P]


# ------------------------------------------------------------------------------------------ python layer

def test_python_layer_errors(tree):
    root, _ = tree
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP path only"):
        bop.visibility(z(4, 3), z(2, 3, dtype=torch.int32), z(1, 2, dtype=torch.int32), z(1, 3, 3), z(1, 3), z(1, 4),
                       z(1, 8, 8), z(1, dtype=torch.int32))
    assert len(bop.INFO) == 11 and bop.INFO[0] == "px_count_all" and bop.INFO[7] == "bbox_visib_x"
    with pytest.raises(ValueError, match="layout"):
        PoseDataset("test", 500, False, root, 0.0, 8, layout="ycb")
    with pytest.raises(ValueError, match="meshes"):
        PoseDataset("test", 500, False, root, 0.0, 8, layout="bop", masks="render", n_model_pts=4)
    with pytest.raises(ValueError, match="masks"):
        PoseDataset("test", 500, False, root, 0.0, 8, layout="bop", masks="jpg", n_model_pts=4)
    with pytest.raises(ValueError, match="needs root"):
        PoseDataset("test", 500, False, None, 0.0, 8, layout="bop")
    ds = PoseDataset("test", 500, False, root, 0.0, 8, layout="bop", n_model_pts=4, meshes=True)
    assert len(ds) == 5 and ds.objlist == [1, 2, 3] and ds.sym_obj == [1] and ds.frame_hw == (sr.H, sr.W)
    assert {ds.crop_size(i) for i in range(len(ds))} == {40}
    for rmin, rmax, cmin, cmax in ds.boxes:                      # snapped inside the tree's own frame
        assert 0 <= rmin and rmax <= sr.H and 0 <= cmin and cmax <= sr.W
    mm = sr.meshes()[2][0].astype(np.float64)
    assert abs(ds.diameter[1] - np.linalg.norm(mm[:, None] - mm[None], axis=-1).max()) < 1e-9   # the tree's json, metres
    assert PoseDataset("test", 500, False, root, 0.0, 8, layout="bop", n_model_pts=4, min_visib=0.0).__len__() == 6
    assert get_square_bbox([100, 100, 50, 50]) == get_square_bbox([100, 100, 50, 50], 480, 640)


def test_write_gt_info_refuses_to_overwrite(tree):
    root, _ = tree
    with pytest.raises(FileExistsError, match="overwrite=True"):
        bop_scene.write_gt_info(root, "test", "cpu")
