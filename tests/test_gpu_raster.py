"""GT-map rendering on the GPU (krrn_raster_maps_f32 / krrn_gt_maps_finish_f32 through raster.render_maps,
raster.finish_maps, PoseDataset(gt_maps=True) and evaluate.test_epoch) against its numpy f64 restatement
(tests/raster_ref.py) on the shared scene family. The discrete maps (face, region, coverage) are compared
exactly, which the restatement's margins license (raster_ref.check_conditions; `grid` by exact arithmetic);
depth / coord / normal within the f32 output format's 1e-6 (tests/test_gpu_umeyama.py's TOL: values below
2 round within 1.2e-7, the f64 differences are far below that).

Scenes (S, faces, what it pins): tetra (40, 4: partial tiles, ray-cast answers), sphere (80, 1280: five face
chunks, analytic depth), layers (40, 4: occlusion), grid (40, 34: exact ties, inclusive edges, duplicates),
behind (40, 80: z <= 1e-3 vertices), border (40, 320: rmin = 0, cut by window and image edge), degenerate
(40, 87: zero-area / collinear / out-of-range faces), mixed (B = 5, S = 40: four meshes, one empty range)."""
import numpy as np
import pytest
import torch

import raster_ref as rr
from pose_estimation_amd import _lib, raster
from pose_estimation_amd.runtime import P, ptr

pytestmark = pytest.mark.gpu

TOL = 1e-6
H, W = rr.H, rr.W
RAW = ("face", "depth", "coord", "normal", "region")
SENTINEL = 7


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Launch:
    """Device operands of one krrn_raster_maps_f32 call, outputs prefilled (NaN / -7 / 7) so that a pixel
    the kernel skipped shows."""

    def __init__(self, dev, verts, faces, face_range, R, t, K4, rc, S, region_pts, cover=True):
        g = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dt)).to(dev)  # noqa: E731
        self.B, self.S, self.NR = len(face_range), S, np.asarray(region_pts).shape[-2]
        B = self.B
        self.verts, self.faces = g(verts, np.float32).reshape(-1, 3), g(faces, np.int32).reshape(-1, 3)
        self.fr, self.R, self.t = g(face_range, np.int32), g(np.reshape(R, (B, 9)), np.float64), g(t, np.float64)
        self.K4, self.rc, self.rp = g(K4, np.float32), g(rc, np.int32), g(region_pts, np.float32).reshape(B, -1, 3)
        self.out = {"face": torch.full((B, S, S), -7, dtype=torch.int32, device=dev),
                    "depth": torch.full((B, S, S), float("nan"), device=dev),
                    "coord": torch.full((B, 3, S, S), float("nan"), device=dev),
                    "normal": torch.full((B, 3, S, S), float("nan"), device=dev),
                    "region": torch.full((B, S, S), -7, dtype=torch.int32, device=dev)}
        self.cover = torch.full((B, H, W), SENTINEL, dtype=torch.uint8, device=dev) if cover else None
        self.dev = dev

    def run(self):
        o = self.out
        _lib.call("krrn_raster_maps_f32", ptr(self.verts), self.verts.shape[0], ptr(self.faces), self.faces.shape[0],
                  ptr(self.fr), ptr(self.R), ptr(self.t), ptr(self.K4), ptr(self.rc), self.S, ptr(self.rp), self.NR,
                  self.B, ptr(o["face"]), ptr(o["depth"]), ptr(o["coord"]), ptr(o["normal"]), ptr(o["region"]),
                  ptr(self.cover), H, W, P(torch.cuda.current_stream(self.dev).cuda_stream))
        return self

    def numpy(self):
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy() for k, v in self.out.items()}
        if self.cover is not None:
            res["cover_frame"] = self.cover.cpu().numpy()
        return res


def _scene_launch(dev, sc, faces=None, cover=True):
    f = sc["faces"] if faces is None else faces
    return Launch(dev, sc["verts"], f, [[0, len(f)]], sc["R"][None], sc["t"][None], sc["K4"][None],
                  [[sc["rmin"], sc["cmin"]]], sc["S"], sc["region_pts"][None], cover=cover)


def _compare(got, b, ref, rmin, cmin, tag, exact=False):
    S = ref["face"].shape[0]
    assert np.array_equal(got["face"][b], ref["face"]), (tag, np.argwhere(got["face"][b] != ref["face"])[:5])
    assert np.array_equal(got["region"][b], ref["region"]), (tag, np.argwhere(got["region"][b] != ref["region"])[:5])
    err = {k: float(np.abs(got[k][b].astype(np.float64) - ref[k]).max()) for k in ("depth", "coord", "normal")}
    print(f"{tag}: covered {int(ref['cover'].sum())} of {S * S}  " + "  ".join(f"|{k} - ref| {v:.2e}" for k, v in err.items()))
    for k, v in err.items():
        assert v <= TOL, (tag, k, v)           # NaN (a pixel never written) fails here too
        if exact:
            assert np.array_equal(got[k][b], ref[k].astype(np.float32)), (tag, k)
    if "cover_frame" in got:
        cf = got["cover_frame"][b]
        assert np.array_equal(cf[rmin:rmin + S, cmin:cmin + S], ref["cover"].astype(np.uint8)), tag
        outside = np.ones((H, W), bool)
        outside[rmin:rmin + S, cmin:cmin + S] = False
        assert (cf[outside] == SENTINEL).all(), tag


@pytest.mark.parametrize("name", rr.SCENES)
def test_scene_parity(dev, name):
    sc, ref = rr.scene(name), rr.reference(name)
    if name in rr.GENERIC:
        rr.check_conditions(ref)
    got = _scene_launch(dev, sc).run().numpy()
    _compare(got, 0, ref, sc["rmin"], sc["cmin"], name, exact=name == "grid")
    if name == "behind":
        for k in ("depth", "coord", "normal"):
            assert np.isfinite(got[k]).all(), k
    if name == "degenerate":   # the mesh without the faces that must be skipped: the same bits
        sound = _scene_launch(dev, sc, faces=sc["faces"][:sc["n_sound"]]).run().numpy()
        for k in RAW + ("cover_frame",):
            assert np.array_equal(_bits(got[k]), _bits(sound[k])), k
    if name == "sphere":
        lo, hi, inner = rr.sphere_depth_bounds(sc)
        z = got["depth"][0].astype(np.float64)
        assert (got["face"][0][inner] >= 0).all()
        assert (z[inner] >= lo[inner] - TOL).all() and (z[inner] <= hi[inner] + TOL).all()


@pytest.mark.parametrize("name", rr.SCENES)
def test_reprojection_of_gpu_output(dev, name):
    """K (R coord + t) of every covered pixel lands within 1e-4 px of its own sample point (f32 coord: an ulp
    of 7.5e-9 m at 0.1 m times fx / z ~ 715 is 5e-6 px), at its own depth."""
    sc = rr.scene(name)
    got = _scene_launch(dev, sc, cover=False).run().numpy()
    ys, xs = np.nonzero(got["face"][0] >= 0)
    assert len(ys)
    cam = got["coord"][0][:, ys, xs].T.astype(np.float64) @ sc["R"].T + sc["t"]
    fx, fy, cx, cy = (float(k) for k in sc["K4"])
    du = fx * cam[:, 0] / cam[:, 2] + cx - (sc["cmin"] + xs)
    dv = fy * cam[:, 1] / cam[:, 2] + cy - (sc["rmin"] + ys)
    dz = cam[:, 2] - got["depth"][0][ys, xs]
    print(f"{name}: |du| {np.abs(du).max():.2e} px  |dv| {np.abs(dv).max():.2e} px  |dz| {np.abs(dz).max():.2e} m")
    assert np.abs(du).max() <= 1e-4 and np.abs(dv).max() <= 1e-4 and np.abs(dz).max() <= TOL


def _mixed_launch(dev, rows=None, cover=True):
    bt, _ = rr.mixed_batch()
    r = list(range(rr.MIXED_B)) if rows is None else rows
    return Launch(dev, bt["verts"], bt["faces"], bt["face_range"][r], bt["R"][r], bt["t"][r], bt["K4"][r], bt["rc"][r],
                  bt["S"], bt["region_pts"][r], cover=cover)


def test_mixed_batch_parity_and_invariance(dev):
    """Five crops over one concatenated mesh (one with an empty face range): each equals its own reference,
    and each rendered alone is bit-identical to itself inside the batch."""
    _, crops = rr.mixed_batch()
    got = _mixed_launch(dev).run().numpy()
    for b, c in enumerate(crops):
        ref = rr.mixed_reference(b)
        rr.check_conditions(ref)
        _compare(got, b, ref, c["rmin"], c["cmin"], f"mixed[{b}]")
    assert (got["face"][3] == -1).all() and not got["depth"][3].any() and not got["region"][3].any()
    assert not got["coord"][3].any() and not got["normal"][3].any()
    for b in range(rr.MIXED_B):
        one = _mixed_launch(dev, rows=[b]).run().numpy()
        for k in RAW + ("cover_frame",):
            assert np.array_equal(_bits(one[k][0]), _bits(got[k][b])), (b, k)
    rev = _mixed_launch(dev, rows=[4, 3, 2, 1, 0]).run().numpy()     # nor on the crop's place in the batch
    for b in range(rr.MIXED_B):
        for k in RAW:
            assert np.array_equal(_bits(rev[k][4 - b]), _bits(got[k][b])), (b, k)


def test_render_maps_api(dev):
    """raster.render_maps (host-side conversion and allocation) gives the kernel's maps, with and without the
    coverage frame; its argument checks raise before any launch."""
    bt, crops = rr.mixed_batch()
    got = _mixed_launch(dev).run().numpy()
    t = torch.from_numpy
    boxes = [(c["rmin"], c["rmin"] + 40, c["cmin"], c["cmin"] + 40) for c in crops]
    args = (t(bt["verts"]).to(dev), t(bt["faces"]).to(dev), t(bt["face_range"]), t(bt["R"]).reshape(-1, 3, 3), t(bt["t"]),
            t(bt["K4"]), boxes, t(bt["region_pts"]).to(dev))
    for hw in ((H, W), None):
        maps = raster.render_maps(*args, frame_hw=hw)
        torch.cuda.synchronize()
        for k in RAW:
            assert maps[k].shape[0] == rr.MIXED_B and np.array_equal(_bits(maps[k].cpu().numpy()), _bits(got[k])), k
        if hw:
            cf = maps["cover_frame"].cpu().numpy()
            assert np.array_equal(cf == 1, got["cover_frame"] == 1) and cf.max() == 1
        else:
            assert "cover_frame" not in maps
    with pytest.raises(ValueError, match="face_range"):
        raster.render_maps(*args[:2], t(bt["face_range"]) + torch.tensor([[0, 10 ** 6]], dtype=torch.int32), *args[3:])
    with pytest.raises(ValueError, match="leaves the"):
        raster.render_maps(*args[:6], [(460, 500, 0, 40)] * rr.MIXED_B, args[7], frame_hw=(H, W))
    with pytest.raises(ValueError, match="one crop size"):
        raster.render_maps(*args[:6], boxes[:4] + [(0, 80, 0, 80)], args[7])
    from oracle.fps_oracle import farthest_point_sampling
    v = rr.scene("sphere")["verts"]
    pts = raster.region_points(t(v).to(dev), 64)
    assert np.array_equal(pts.cpu().numpy(), v[farthest_point_sampling(v, 64)])


def _finish_inputs(dev, seed=3):
    rng = np.random.default_rng(seed)
    B, S = rr.MIXED_B, 40
    L = _mixed_launch(dev, cover=False).run()
    raw = L.numpy()
    pm = ((raw["face"] >= 0) & (rng.random((B, S, S)) < 0.8)).astype(np.uint8)   # label * depth * cover
    cls = np.array([0, 12, 3, 5, 1], np.int64)
    ext = rng.uniform(0.05, 0.2, (B, 3))
    lfb = -ext / 2 + rng.uniform(-0.01, 0.01, (B, 3))
    return L, raw, pm, cls, ext, lfb


FIN = ("xyz", "normal", "region", "mask", "multi_cls_mask", "mask_obj")


def test_finish_parity(dev):
    L, raw, pm, cls, ext, lfb = _finish_inputs(dev)
    B, S = rr.MIXED_B, 40
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    fin = raster.finish_maps(L.out, t(pm).view(B, 1, S, S), t(cls).view(B, 1), t(ext), t(lfb))
    torch.cuda.synchronize()
    assert fin["normal"] is L.out["normal"]                        # masked in place
    shapes = {"xyz": (B, 3, S, S), "normal": (B, 3, S, S), "region": (B, S, S), "mask": (B, 1, S, S),
              "multi_cls_mask": (B, S, S), "mask_obj": (B, 1, S, S)}
    for k in FIN:
        assert tuple(fin[k].shape) == shapes[k], k
    assert fin["region"].dtype == fin["multi_cls_mask"].dtype == torch.int64
    for b in range(B):
        ref = rr.finish(raw["coord"][b].reshape(3, -1), raw["normal"][b].reshape(3, -1), raw["region"][b].reshape(-1),
                        raw["face"][b].reshape(-1), pm[b].reshape(-1), cls[b], ext[b], lfb[b])
        for k in ("region", "multi_cls_mask", "mask", "mask_obj"):
            assert np.array_equal(fin[k][b].cpu().numpy().reshape(-1), ref[k]), (b, k)
        for k in ("xyz", "normal"):
            e = np.abs(fin[k][b].cpu().numpy().reshape(3, -1).astype(np.float64) - ref[k]).max()
            assert e <= TOL, (b, k, e)
    on = pm.astype(bool)
    assert (fin["multi_cls_mask"].cpu().numpy()[on] == (cls[:, None, None] + 1).repeat(S, 1).repeat(S, 2)[on]).all()
    assert not fin["xyz"].cpu().numpy()[np.repeat(~on[:, None], 3, 1)].any()


def test_graph_replay(dev):
    """The render and finish launches captured on a side stream and replayed twice: both replays bit-equal
    to the eager calls."""
    L, raw, pm, cls, ext, lfb = _finish_inputs(dev)
    B, S = rr.MIXED_B, 40
    L.cover = torch.full((B, H, W), SENTINEL, dtype=torch.uint8, device=dev)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    pmt, clst, extt, lfbt = t(pm), t(cls), t(ext), t(lfb)
    fin = {"xyz": torch.empty((B, 3, S, S), device=dev), "region": torch.empty((B, S, S), dtype=torch.int64, device=dev),
           "mask": torch.empty((B, S * S), device=dev), "multi_cls_mask": torch.empty((B, S, S), dtype=torch.int64, device=dev),
           "mask_obj": torch.empty((B, S * S), device=dev)}
    outs = list(L.out.values()) + [L.cover] + list(fin.values())

    def step():
        L.run()
        o = L.out
        _lib.call("krrn_gt_maps_finish_f32", ptr(o["coord"]), ptr(o["region"]), ptr(o["face"]), ptr(pmt), ptr(clst),
                  ptr(extt), ptr(lfbt), B, S * S, ptr(fin["xyz"]), ptr(o["normal"]), ptr(fin["region"]), ptr(fin["mask"]),
                  ptr(fin["multi_cls_mask"]), ptr(fin["mask_obj"]), P(torch.cuda.current_stream(dev).cuda_stream))

    def snap():
        torch.cuda.synchronize()
        return [o.clone() for o in outs]

    def clear():
        for o in outs:
            o.zero_()

    clear()
    step()
    eager = snap()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            step()
    torch.cuda.current_stream().wait_stream(s)
    clear()
    graph.replay()
    first = snap()
    clear()
    graph.replay()
    second = snap()
    for e, a, b in zip(eager, first, second):
        assert torch.equal(e, a) and torch.equal(e, b)
    assert (eager[0] >= 0).any()


def test_empty_ranges_and_no_cover(dev):
    """face_count = 0 for every crop and no cover_frame (H, W unused) is a legal call: all background."""
    bt, _ = rr.mixed_batch()
    L = _mixed_launch(dev, cover=False)
    L.fr.zero_()
    got = L.run().numpy()
    assert (got["face"] == -1).all() and not got["depth"].any() and not got["region"].any()
    assert not got["coord"].any() and not got["normal"].any()


# ------------------------------------------------------------------------------------------- dataset, epoch

TODAY = {"img_croped", "choose", "cloud", "x_map_choosed", "y_map_choosed", "point_mask", "mask_count", "cls_id",
         "intrinsic", "extent", "lfborder", "bbox", "target_r", "target_t", "model_points", "target"}
N_PT, N_MODEL = 500, 150


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """All 13 LineMOD objects (cls_type='all'): the first two with three frames (crop sizes 40 / 80 / 40), the
    rest with one frame of size 40."""
    import mesh_tree
    from pose_estimation_amd.config import LM_OBJLIST
    root = str(tmp_path_factory.mktemp("mesh_tree"))
    w = mesh_tree.write_tree(root, objs=LM_OBJLIST, per_obj=(3, 3) + (1,) * (len(LM_OBJLIST) - 2))
    return root, w


def _dataset(root, gt_maps):
    from pose_estimation_amd.dataset import PoseDataset
    kw = {"gt_maps": True} if gt_maps else {}
    return PoseDataset("test", N_PT, False, root, 0.0, 8, cls_type="all", n_model_pts=N_MODEL, **kw)


def test_dataset_gt_maps(dev, tree):
    from oracle.fps_oracle import farthest_point_sampling
    from pose_estimation_amd.config import models_info
    root, w = tree
    ds = _dataset(root, True)
    sizes = [ds.crop_size(i) for i in range(len(ds))]
    assert len(ds) == 17 and sorted(set(sizes)) == [40, 80] and sizes[:6] == [40, 80, 40, 40, 80, 40]
    info = models_info()
    for S in (40, 80):
        idx = [i for i in range(len(ds)) if sizes[i] == S]
        B = len(idx)
        data = ds.batch(idx, dev)
        torch.cuda.synchronize()
        shapes = {"xyz": (B, 3, S, S), "normal": (B, 3, S, S), "region": (B, S, S), "mask": (B, 1, S, S),
                  "multi_cls_mask": (B, S, S), "mask_obj": (B, 1, S, S), "region_point": (B, 65, 3),
                  "coordinate_choosed": (B, N_PT, 3), "depth_render": (B, S, S)}
        assert set(data) == TODAY | set(shapes)
        for k, shp in shapes.items():
            assert tuple(data[k].shape) == shp, (k, tuple(data[k].shape))
            assert data[k].dtype == (torch.int64 if k in ("region", "multi_cls_mask") else torch.float32), k
        d = {k: v.cpu().numpy() for k, v in data.items()}
        assert (d["mask_count"] > 0).all()
        for b, i in enumerate(idx):
            it = ds.tree.items[i]
            obj, fr = int(it["obj"]), w[(int(it["obj"]), int(it["im"]))]
            rmin, rmax, cmin, cmax = ds.boxes[i]
            win = (slice(rmin, rmax), slice(cmin, cmax))
            # mask = label * depth * cover (batchdataset.py:667-670), from the files the tree writer made
            exp = (fr["mask"][win] == 255) & (fr["depth_mm"][win] != 0) & fr["cover"][win]
            assert np.array_equal(d["mask"][b, 0] == 1, exp) and exp.sum() == d["mask_count"][b]
            assert np.array_equal(d["point_mask"][b, 0] != 0, exp)
            assert np.array_equal(d["mask_obj"][b, 0] == 1, fr["cover"][win])
            assert (d["mask"][b, 0].reshape(-1)[d["choose"][b, 0]] == 1).all()
            cls = ds.objlist.index(obj)
            assert np.array_equal(d["multi_cls_mask"][b], exp * (cls + 1))
            # the maps against the restatement under the pose the loader read from gt.yml
            v, f = w["mesh"][obj]
            lf, ext = np.array(info[obj]["min"]) / 1000.0, np.array(info[obj]["size"]) / 1000.0
            rp = v[farthest_point_sampling(v, 64)]
            ref = rr.render(v, f, it["R"], it["t"], rr.LM_K4, rmin, cmin, S, rp, margins=False)
            assert np.array_equal(ref["cover"], fr["cover"][win])
            assert np.abs(d["depth_render"][b] - ref["depth"]).max() <= TOL
            fin = rr.finish(ref["coord"].reshape(3, -1).astype(np.float32), ref["normal"].reshape(3, -1), ref["region"].reshape(-1),
                            ref["face"].reshape(-1), exp.reshape(-1), cls, ext, lf)
            assert np.array_equal(d["region"][b].reshape(-1), fin["region"])
            # 1e-6 on coord is 1e-6 / extent on xyz: the extents here are 0.04 .. 0.26 m
            assert np.abs(d["xyz"][b].reshape(3, -1) - fin["xyz"]).max() <= TOL / ext.min()
            assert np.abs(d["normal"][b].reshape(3, -1) - fin["normal"]).max() <= TOL
            assert not d["region_point"][b, 0].any()
            assert np.array_equal(d["region_point"][b, 1:], ((rp.astype(np.float64) - lf) / ext).astype(np.float32))
            cc = ref["coord"].reshape(3, -1)[:, d["choose"][b, 0]].T
            assert np.abs(d["coordinate_choosed"][b] - cc).max() <= TOL
    plain = _dataset(root, False)
    data = plain.batch([i for i in range(len(plain)) if sizes[i] == 80], dev)
    assert set(data) == TODAY


def test_eval_epoch_map_losses(dev, tree):
    """test_epoch with a criterion over a stock-layout tree: with gt_maps the map-loss columns fill (finite, over
    a positive number of valid pixels); without, they stay empty as before. On the parent commit this fails
    with TypeError on the gt_maps keyword."""
    from pose_estimation_amd import KRRN, make_config
    from pose_estimation_amd.evaluate import test_epoch as run_epoch
    from pose_estimation_amd.loss import KRRNLoss, map_losses
    from pose_estimation_amd.synthetic import init_weights
    root, _ = tree
    ds = _dataset(root, True)
    m = KRRN(cfg=make_config(num_cls=len(ds.objlist), backbone="w18"))
    init_weights(m, 0)
    m = m.to(dev).eval()
    crit = KRRNLoss(sym_list=ds.sym_obj)
    res = run_epoch(m, ds, bs=4, device=dev, criterion=crit)
    assert res["test_count"] == len(ds) == 17
    for k in ("dis_xyz", "dis_normal", "dis_mask"):
        vals = np.array([res[k][o] for o in ds.objlist])
        print(k, vals)
        assert np.isfinite(vals).all() and (vals > 0).all(), k
    # all four terms and their valid-pixel counts, per crop, for one batch
    idx = [i for i in range(len(ds)) if ds.crop_size(i) == 80]
    data = ds.batch(idx, dev)
    with torch.no_grad():
        pred = m(data["img_croped"], data["cloud"], data["choose"], data["cls_id"], opt_pose=True)
        lc = map_losses(pred, data, per_crop=True).cpu().numpy()
    print(lc)
    assert lc.shape == (len(idx), 8) and np.isfinite(lc).all() and (lc[:, :4] > 0).all() and (lc[:, 4:] > 0).all()
    assert np.array_equal(lc[:, 4], data["mask_count"].cpu().numpy())   # xyz's valid pixels are the mask's
    plain = run_epoch(m, _dataset(root, False), bs=4, device=dev, criterion=crit)
    assert plain["test_count"] == 17
    for k in ("dis_xyz", "dis_normal", "dis_mask"):
        assert all(v == 0.0 for v in plain[k].values()), k
