"""The surface sampler's definition and refusals, without a GPU: the numpy restatement (tests/surface_ref.py) on a box
whose weights, areas and sides are known exactly, the cumulative weights across tile edges, the entry point's host-side
checks (they run before any HIP call, so fake pointers do), and the Python layer's refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bop_tree
import surface_ref as sf
from pose_estimation_amd import _lib, bop_scene, models
from pose_estimation_amd.dataset import PoseDataset

SIZE = np.float32([1, 2, 3])
# corner x * 4 + y * 2 + z of a 1 x 2 x 3 box; the 2 x 3 sides first, then 1 x 3, then 1 x 2, wound outwards; then a
# zero-area face, a face with an index past the vertices and one with a negative index
BOX_V = np.array([[x, y, z] for x in (0, 1) for y in (0, 2) for z in (0, 3)], np.float32)
BOX_F = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 4, 5], [0, 5, 1], [2, 7, 6], [2, 3, 7],
                  [0, 2, 6], [0, 6, 4], [1, 7, 3], [1, 5, 7], [0, 0, 1], [0, 1, 8], [0, -1, 2]], np.int32)
BOX_W = [6, 6, 6, 6, 3, 3, 3, 3, 2, 2, 2, 2, 0, 0, 0]
BOX_AXIS = [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]            # the axis each side is normal to
BOX_SIGN = [-1, -1, 1, 1, -1, -1, 1, 1, -1, -1, 1, 1]      # and the outward direction along it


def test_restated_box_case():
    n = 4096
    w, N = sf.face_weights(BOX_V, BOX_F)
    assert w.tolist() == BOX_W
    s = sf.sample_one(BOX_V, BOX_F, n, seed=7, stream=3, row=5)
    assert s["status"] == 0 and s["cum"][-1] == 44.0 and s["area"] == 22.0
    assert s["cum"].tolist() == np.cumsum(BOX_W).tolist()
    face, p, q = s["face"], s["points"], s["normals"]
    assert p.dtype == np.float32 and q.dtype == np.float32 and face.dtype == np.int32
    assert face.min() >= 0 and face.max() <= 11                # never a face of weight 0
    axis, sign = np.array(BOX_AXIS)[face], np.array(BOX_SIGN)[face]
    plane = np.where(sign > 0, SIZE[axis], np.float32(0))
    assert np.array_equal(p[np.arange(n), axis], plane)       # exactly on its side
    assert (p >= 0).all() and (p <= SIZE).all()                # and inside the box
    want = np.zeros((n, 3), np.float32)
    want[np.arange(n), axis] = sign
    assert np.array_equal(q, want)                             # N / |N| of an axis-aligned side is exact
    count = np.bincount(face, minlength=15)
    prob = np.array(BOX_W) / 44.0
    sigma = np.sqrt(n * prob * (1 - prob))
    dev = np.abs(count[:12] - n * prob[:12]) / sigma[:12]
    print("largest deviation of a face's count: %.2f sigma" % dev.max())
    assert dev.max() < 5.0 and not count[12:].any()
    # the two triangles of a side are hit evenly too: the barycentric map covers the triangle, not a corner of it
    c = p[face == 0]
    assert 0.2 < (c[:, 2] > 1.5).mean() < 0.8 and 0.05 < (c[:, 1] > 1.0).mean() < 0.6


def test_restated_draws_differ_by_row_seed_and_stream():
    base = sf.sample_one(BOX_V, BOX_F, 64, seed=7, stream=3, row=5)
    for kw in (dict(seed=8, stream=3, row=5), dict(seed=7, stream=4, row=5), dict(seed=7, stream=3, row=6)):
        other = sf.sample_one(BOX_V, BOX_F, 64, **kw)
        assert not np.array_equal(other["points"], base["points"]), kw
    again = sf.sample_one(BOX_V, BOX_F, 64, seed=7, stream=3, row=5)
    assert np.array_equal(again["points"], base["points"]) and np.array_equal(again["face"], base["face"])
    first = sf.sample_one(BOX_V, BOX_F, 16, seed=7, stream=3, row=5)         # sample i does not depend on n
    assert np.array_equal(first["points"], base["points"][:16])


def test_restated_cum_is_non_decreasing_across_tile_edges():
    rng = np.random.default_rng(0)
    F = 3 * sf.TILE + 17
    v = rng.normal(size=(400, 3)).astype(np.float32)
    f = rng.integers(0, 400, size=(F, 3))
    f[sf.TILE - 1] = f[sf.TILE] = f[2 * sf.TILE] = [3, 3, 3]                 # weight 0 on both sides of an edge
    w, _ = sf.face_weights(v, f)
    cum = sf.cumulative(w)
    assert (np.diff(cum) >= 0).all() and (w >= 0).all()
    assert cum[sf.TILE] == cum[sf.TILE - 1] == cum[sf.TILE - 2] and cum[2 * sf.TILE] == cum[2 * sf.TILE - 1]
    assert cum[sf.TILE - 1] == np.cumsum(w[:sf.TILE])[-1]                    # tile 0 is a plain running sum
    # 785 sums of non-negative terms, each rounded within 2^-53 of its value: 1e-12 relative covers the reordering
    assert abs(cum[-1] - w.sum()) <= 1e-12 * w.sum()


def test_restated_object_without_area():
    for faces in (np.zeros((0, 3), np.int32), BOX_F[12:]):
        s = sf.sample_one(BOX_V, faces, 5, seed=1, stream=0, row=0)
        assert s["status"] == 1 and s["area"] == 0.0 and not s["points"].any() and not s["normals"].any()
        assert (s["face"] == -1).all()
    nan = BOX_V.copy()
    nan[0, 1] = np.nan
    w, _ = sf.face_weights(nan, BOX_F)
    assert [x for k, x in enumerate(w.tolist()) if 0 in BOX_F[k]] == [0.0] * 9 and w[2] == 6.0
    s = sf.sample(BOX_V, BOX_F, [[0, 12], [-1, 3], [2, -1], [10, 6], [12, 3]], [0, 1, 2, 3, 4], 4, 1, 0, max_f=12)
    assert s["status"].tolist() == [0, 1, 1, 1, 1] and s["area"].tolist() == [22.0, 0, 0, 0, 0]


def test_entry_point_refuses_on_the_host():
    fn = _lib.lib().krrn_surface_sample_f64
    N = ctypes.c_void_p(0)
    p = [ctypes.c_void_p(0x10000 * (k + 1)) for k in range(9)]

    # verts, Vtot, faces, Ftot, face_range, row_id, O, max_f, n, seed, stream_id, cum, pts, nrm, face, status, stream
    def call(null=None, **kw):
        k = dict(Vtot=8, Ftot=12, O=2, max_f=12, n=16)
        k.update(kw)
        a = [p[0], k["Vtot"], p[1], k["Ftot"], p[2], p[3], k["O"], k["max_f"], k["n"], 7, 3, p[4], p[5], p[6], p[7],
             p[8], N]
        if null is not None:
            a[null] = N
        return fn(*a)
    for null in (0, 2, 4, 5, 11, 12, 13, 14, 15):
        assert call(null=null) == -1, null
    for bad in (dict(O=0), dict(O=65536), dict(O=-1), dict(Vtot=0), dict(Ftot=-1), dict(max_f=0), dict(n=0),
                dict(n=(1 << 28) + 1), dict(n=-5)):
        assert call(**bad) == -2, bad
    assert call(null=0, O=0) == -1                                          # a null pointer before a bad shape


def test_python_layer_refuses():
    v, f = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    r = torch.tensor([[0, 2]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP path only"):
        models.sample_surface(v, f, r, 16)
    with pytest.raises(ValueError, match="16384"):
        models.sample_surface(v, f, r, 4097, oversample=4)                  # before the tensors are looked at
    with pytest.raises(ValueError, match="16384"):
        models.sample_surface(v, f, r, 2, oversample=8193)
    with pytest.raises(ValueError, match="meshes=True"):
        PoseDataset("test", 100, False, None, model_points="surface")
    with pytest.raises(ValueError, match="model_points"):
        PoseDataset("test", 100, False, None, model_points="faces")
    assert models.SURFACE_TILE == sf.TILE and models.FPS_MAX == 16384


def test_write_models_eval_refuses_an_existing_file(tmp_path):
    root = str(tmp_path)
    bop_tree.write_models(root)
    os.makedirs(os.path.join(root, "models_eval"))
    path = os.path.join(root, "models_eval", "obj_000002.ply")
    with open(path, "w") as fh:
        fh.write("mine\n")
    with pytest.raises(FileExistsError, match="overwrite=True"):
        bop_scene.write_models_eval(root, "cuda:0", n=64)
    assert open(path).read() == "mine\n" and os.listdir(os.path.join(root, "models_eval")) == ["obj_000002.ply"]
