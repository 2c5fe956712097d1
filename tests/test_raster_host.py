"""GT-map rendering without a GPU: the numpy restatement (tests/raster_ref.py) on the shared scene
family (its decision margins, the known answers of `tetra`, `layers`, `grid` and `sphere`, the
reprojection identity), the PLY face reader, the host-side argument checks of krrn_raster_maps_f32 and
krrn_gt_maps_finish_f32 (they run before any HIP call) and PoseDataset(gt_maps=True)'s errors."""
import ctypes

import numpy as np
import pytest

import raster_ref as rr
from pose_estimation_amd import _lib
from pose_estimation_amd.dataset import PoseDataset, ply_faces, ply_vtx


@pytest.mark.parametrize("name", rr.GENERIC)
def test_scene_conditions(name):
    """Every generic scene decides coverage, depth order, region and normal direction with room to spare."""
    res = rr.reference(name)
    print(name, int(res["cover"].sum()), {k: float(v.min()) for k, v in res["margins"].items()})
    rr.check_conditions(res)
    assert res["cover"].any()


def test_mixed_batch_conditions():
    batch, crops = rr.mixed_batch()
    assert batch["face_range"][3, 1] == 0 and len({tuple(r) for r in batch["face_range"].tolist()}) == rr.MIXED_B
    for b in range(rr.MIXED_B):
        res = rr.mixed_reference(b)
        rr.check_conditions(res)
        assert res["cover"].any() == (b != 3)
    assert batch["face_range"][2, 0] == batch["face_range"][3, 0]   # crops 2 and 3 share a mesh; 3 draws none of it


@pytest.mark.parametrize("name", ["tetra", "layers"])
def test_known_answers_against_ray_casting(name):
    """Face and depth per pixel equal a 3-D ray / triangle intersection that shares no code with the
    rasteriser's 2-D edge functions."""
    sc, res = rr.scene(name), rr.reference(name)
    face, depth = rr.raycast(sc["verts"], sc["faces"], sc["R"], sc["t"], sc["K4"], sc["rmin"], sc["cmin"], sc["S"])
    assert np.array_equal(face, res["face"])
    assert np.abs(depth - res["depth"]).max() < 1e-12
    if name == "tetra":    # the base (face 3) is hidden behind the three sides
        assert set(np.unique(res["face"])) == {-1, 0, 1, 2}
    if name == "layers":   # the near quad (faces 2, 3) hides the far one wherever it projects
        near = np.isin(res["face"], (2, 3))
        assert near.any() and np.isin(res["face"], (0, 1)).any()
        assert res["depth"][near].max() < 0.95 < res["depth"][np.isin(res["face"], (0, 1))].min()


def test_grid_known_answers():
    """Integer geometry: vertex (i, j) projects to pixel (64 + 8 i, 64 + 8 j) exactly, every depth is 1, so
    the expected maps follow from integer arithmetic: closed triangles (edge pixels included, no holes), the
    lowest face index on shared edges and over the duplicates."""
    sc, res = rr.scene("grid"), rr.reference("grid")
    S, r0, c0 = sc["S"], sc["rmin"], sc["cmin"]
    P = np.rint(sc["verts"].astype(np.float64) * 512).astype(np.int64)[:, :2] + 64   # vertex pixels
    exp = np.full((S, S), -1, np.int64)
    for y in range(S):
        for x in range(S):
            p = np.array([c0 + x, r0 + y])
            for f, (a, b, c) in enumerate(sc["faces"]):
                e = [int((P[j, 0] - P[i, 0]) * (p[1] - P[i, 1]) - (P[j, 1] - P[i, 1]) * (p[0] - P[i, 0]))
                     for i, j in ((a, b), (b, c), (c, a))]
                if all(v >= 0 for v in e) or all(v <= 0 for v in e):
                    exp[y, x] = f
                    break
    assert np.array_equal(res["face"], exp)
    cov = exp >= 0
    ys, xs = np.nonzero(cov)
    assert cov.sum() == 33 * 33 and exp.max() < len(sc["faces"]) - 2          # no holes; no duplicate wins
    assert (ys.min() + r0, ys.max() + r0, xs.min() + c0, xs.max() + c0) == (64, 96, 64, 96)
    diag = cov & ((np.arange(S)[:, None] + r0) == (np.arange(S)[None] + c0))   # the cells' shared edges
    assert diag.sum() == 33 and (exp[diag] % 2 == 0).all()                     # go to the lower (even) face
    assert np.array_equal(res["depth"], cov.astype(np.float64))
    assert np.array_equal(res["coord"][0][cov], (xs + c0 - 64) / 512.0)
    assert np.array_equal(res["coord"][1][cov], (ys + r0 - 64) / 512.0)
    assert not res["coord"][2].any()
    assert np.array_equal(res["normal"][2], -cov.astype(np.float64)) and not res["normal"][:2].any()
    rp = np.rint(sc["region_pts"].astype(np.float64) * 512).astype(np.int64)[:, :2] + 64
    d2 = (xs[:, None] + c0 - rp[None, :, 0]) ** 2 + (ys[:, None] + r0 - rp[None, :, 1]) ** 2
    assert np.array_equal(res["region"][cov], 1 + np.argmin(d2, 1))


def test_sphere_depth_within_chord_error():
    """The mesh lies between its inscribed sphere and the sphere through its vertices, so every ray that
    meets the inner sphere hits the mesh between its two analytic sphere hits."""
    sc, res = rr.scene("sphere"), rr.reference("sphere")
    lo, hi, inner = rr.sphere_depth_bounds(sc)
    z = res["depth"]
    assert inner.sum() > 3000 and res["cover"][inner].all()
    assert (z[inner] >= lo[inner] - 1e-7).all() and (z[inner] <= hi[inner] + 1e-7).all()
    print("chord error", float((hi - lo)[inner].max()), "m; depth above the outer sphere", float((z - lo)[inner].max()))


@pytest.mark.parametrize("name", rr.SCENES)
def test_reprojection_identity(name):
    """Every covered pixel's model coordinate projects back onto its own sample point, at its own depth."""
    sc, res = rr.scene(name), rr.reference(name)
    ys, xs = np.nonzero(res["cover"])
    cam = res["coord"][:, ys, xs].T @ sc["R"].T + sc["t"]
    fx, fy, cx, cy = (float(k) for k in sc["K4"])
    du = fx * cam[:, 0] / cam[:, 2] + cx - (sc["cmin"] + xs)
    dv = fy * cam[:, 1] / cam[:, 2] + cy - (sc["rmin"] + ys)
    dz = cam[:, 2] - res["depth"][ys, xs]
    print(name, np.abs(du).max(), np.abs(dv).max(), np.abs(dz).max())
    assert np.abs(du).max() < 1e-9 and np.abs(dv).max() < 1e-9 and np.abs(dz).max() < 1e-12
    assert np.abs(np.linalg.norm(res["normal"][:, ys, xs], axis=0) - 1.0).max() < 1e-12
    assert ((res["normal"][:, ys, xs].T * cam).sum(1) < 0).all()   # towards the camera


def test_skipped_faces():
    """`behind`: faces with a vertex at z <= 1e-3 never appear, and nothing is NaN. `degenerate`: the appended
    zero-area, collinear and out-of-range faces change nothing."""
    sc, res = rr.scene("behind"), rr.reference("behind")
    cz = (sc["verts"].astype(np.float64) @ sc["R"].T + sc["t"])[:, 2]
    bad = (cz[sc["faces"]] <= rr.NEAR).any(1)
    assert bad.sum() > 10 and (~bad).sum() > 10
    assert not np.isin(res["face"], np.nonzero(bad)[0]).any()
    for k in ("depth", "coord", "normal"):
        assert np.isfinite(res[k]).all()
    sc, res = rr.scene("degenerate"), rr.reference("degenerate")
    sound = rr.render(sc["verts"], sc["faces"][:sc["n_sound"]], sc["R"], sc["t"], sc["K4"], sc["rmin"], sc["cmin"],
                      sc["S"], sc["region_pts"], margins=False)
    assert len(sc["faces"]) == sc["n_sound"] + 7
    for k in ("face", "depth", "coord", "normal", "region"):
        assert np.array_equal(res[k], sound[k]), k


def test_border_scene_straddles_window_and_frame():
    sc, res = rr.scene("border"), rr.reference("border")
    assert sc["rmin"] == 0 and res["cover"][0].any() and res["cover"][:, 0].any()   # cut by row 0 and the left edge
    v = (sc["verts"].astype(np.float64) @ sc["R"].T + sc["t"])
    assert (float(sc["K4"][1]) * v[:, 1] / v[:, 2] + float(sc["K4"][3])).min() < 0  # part of it is above the image


def test_ply_faces_round_trip(tmp_path):
    import linemod_tree
    import mesh_tree
    w = mesh_tree.write_tree(str(tmp_path / "a"), objs=(6,), per_obj=(1,))
    v, f = w["mesh"][6]
    path = str(tmp_path / "a" / "models" / "obj_06.ply")
    got = ply_faces(path)                                   # trailing per-face properties are ignored
    assert got.dtype == np.int32 and np.array_equal(got, f) and len(f) == 320
    assert np.array_equal(ply_vtx(path) / 1000.0, v)
    linemod_tree.write_tree(str(tmp_path / "b"), objs=(6,), per_obj=1, sizes=(80,))
    assert ply_faces(str(tmp_path / "b" / "models" / "obj_06.ply")).shape == (0, 3)
    quad = tmp_path / "quad.ply"
    quad.write_text("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                    "element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n4 0 0 0 0\n")
    with pytest.raises(ValueError, match="not a triangle"):
        ply_faces(str(quad))


def test_gt_maps_needs_a_mesh(tmp_path):
    import linemod_tree
    with pytest.raises(ValueError, match="root=None"):
        PoseDataset("test", 500, False, None, 0.0, 8, cls_type="cat", gt_maps=True)
    linemod_tree.write_tree(str(tmp_path), objs=(6,), per_obj=1, sizes=(80,))
    with pytest.raises(ValueError, match="obj_06.ply has no faces"):
        PoseDataset("test", 500, False, str(tmp_path), 0.0, 8, cls_type="cat", gt_maps=True)
    ds = PoseDataset("test", 500, False, str(tmp_path), 0.0, 8, cls_type="cat")   # the default needs no faces
    assert ds.gt_maps is False and ds.tree.mesh == {}


def _fakes(names):
    """Distinct, far-apart non-null pointers (never dereferenced: the checks fail before any launch)."""
    return {k: ctypes.c_void_p((i + 1) << 36) for i, k in enumerate(names)}


def test_raster_host_side_errors():
    fn = _lib.lib().krrn_raster_maps_f32
    N = ctypes.c_void_p(0)
    names = ("verts", "faces", "face_range", "R", "t", "K4", "rc", "region_pts", "face", "depth", "coord", "normal",
             "region", "cover")

    def call(S=40, NR=64, B=2, V=10, F=4, H=480, W=640, **over):
        p = _fakes(names)
        p.update(over)
        return fn(p["verts"], V, p["faces"], F, p["face_range"], p["R"], p["t"], p["K4"], p["rc"], S, p["region_pts"],
                  NR, B, p["face"], p["depth"], p["coord"], p["normal"], p["region"], p["cover"], H, W, N)

    for k in names[:-1]:                                    # every required pointer; cover_frame is optional
        assert call(**{k: N}) == -1, k
    f = _fakes(names)
    assert call(depth=f["face"]) == -1                      # two outputs on one buffer
    assert call(coord=f["verts"]) == -1                     # an output on an input
    assert call(normal=ctypes.c_void_p(f["coord"].value + 16)) == -1   # overlapping ranges
    assert call(cover=f["rc"]) == -1
    assert call(S=0) == -2 and call(S=481) == -2
    assert call(NR=0) == -2 and call(NR=257) == -2
    assert call(B=0) == -2 and call(V=0) == -2 and call(F=-1) == -2
    assert call(S=481, verts=N) == -1                       # pointers are checked first
    assert call(S=480, H=479, W=640) == -2 and call(S=480, H=480, W=479) == -2   # no window fits the frame
    # without cover_frame H and W are unused, and face_count = 0 everywhere is a legal call: those launch, so
    # they are GPU tests (test_gpu_raster.py)


def test_finish_host_side_errors():
    fn = _lib.lib().krrn_gt_maps_finish_f32
    N = ctypes.c_void_p(0)
    names = ("coord", "region_raw", "face", "point_mask", "cls", "extent", "lfborder", "xyz", "normal", "region",
             "mask", "multi_cls_mask", "mask_obj")

    def call(B=2, HW=1600, **over):
        p = _fakes(names)
        p.update(over)
        return fn(p["coord"], p["region_raw"], p["face"], p["point_mask"], p["cls"], p["extent"], p["lfborder"], B, HW,
                  p["xyz"], p["normal"], p["region"], p["mask"], p["multi_cls_mask"], p["mask_obj"], N)

    for k in names:
        if k not in ("face", "mask_obj"):
            assert call(**{k: N}) == -1, k
    assert call(face=N) == -1                               # mask_obj needs the face map
    f = _fakes(names)
    assert call(xyz=f["coord"]) == -1 and call(mask=f["multi_cls_mask"]) == -1
    assert call(B=0) == -2 and call(HW=0) == -2 and call(HW=480 * 480 + 1) == -2
    assert call(B=0, coord=N) == -1


def test_cpu_tensors_raise():
    import torch
    from pose_estimation_amd import raster
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP path only"):
        raster.render_maps(z(4, 3), z(2, 3, dtype=torch.int32), z(1, 2, dtype=torch.int32), z(1, 3, 3), z(1, 3),
                           z(1, 4), [(0, 40, 0, 40)], z(1, 64, 3))
    assert (raster.N_REGIONS, raster.MAX_S, raster.MAX_REGIONS) == (64, 480, 256)
