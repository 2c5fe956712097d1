"""The model-info kernels' definitions and refusals, without a GPU: the numpy restatement (tests/models_ref.py) against
brute force, the entry points' host-side checks (they run before any HIP call, so fake pointers do), and the Python
layer's refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bop_tree
import models_ref as mr
from pose_estimation_amd import _lib, bop_scene, models


def test_restated_diameter_is_the_brute_force_norm():
    """rel 1e-12: three non-negative products, two sums and a root of at most 2^-53 each, with no cancellation."""
    v = np.random.default_rng(0).normal(size=(50, 3)).astype(np.float32)
    d2, box = mr.extent_one(v)
    x = v.astype(np.float64)
    brute = max(np.linalg.norm(x[i] - x[j]) for i in range(50) for j in range(50))
    assert abs(np.sqrt(d2) - brute) <= 1e-12 * brute
    assert (box[:3] == x.min(0)).all() and (box[3:] == x.max(0)).all()


def test_restated_extent_edges():
    assert mr.extent_one(np.zeros((0, 3), np.float32))[0] == 0.0
    assert mr.extent_one(np.ones((1, 3), np.float32))[0] == 0.0
    assert mr.extent_one(np.ones((7, 3), np.float32))[0] == 0.0
    d2, box = mr.extent_one(np.array([[0, 0, 0], [np.nan, 1, 1], [3, 4, 12]], np.float32))
    assert d2 == 169.0 and list(box) == [0, 0, 0, 3, 4, 12]
    d2, box = mr.extent(np.zeros((4, 3), np.float32), [[-1, 2], [2, 3], [0, 4]], max_v=3)
    assert list(d2) == [0.0] * 3 and np.isposinf(box[:, :3]).all() and np.isneginf(box[:, 3:]).all()


def _triangles(rng, n):
    tri = rng.normal(size=(n, 3, 3))
    tri[0, 1] = tri[0, 2] = tri[0, 0]                          # collapsed to a point
    tri[1, 2] = tri[1, 0] + 0.3 * (tri[1, 1] - tri[1, 0])      # collinear, c between a and b
    tri[2, 2] = tri[2, 0] + 2.5 * (tri[2, 1] - tri[2, 0])      # collinear, c beyond b
    return tri


def test_restated_closest_point_never_exceeds_dense_sampling():
    """The closest point is a point of the triangle at least as near as every sampled one. Slack: the sampled
    distances and the restatement each carry a few dozen roundings of 2^-53 relative to the operands' squares (all
    of order 1 to 10 here), so 1e-12 absolute covers them a thousand times over. The other direction bounds the
    restatement from below: some sample lies within one grid step (the longest edge / n) of the true closest point."""
    rng = np.random.default_rng(1)
    n = 60
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = i + j <= n
    u, v = i[keep] / n, j[keep] / n
    for tri in _triangles(rng, 40):
        a, b, c = tri
        pts = rng.normal(size=(25, 3)) * 1.5
        pts[:3] = a, b, (a + b + c) / 3.0                       # on a corner and inside the face
        d = mr.tri_dist2(pts, a, b, c)
        assert np.isfinite(d).all()
        samples = a + u[:, None] * (b - a) + v[:, None] * (c - a)
        dense = ((pts[:, None, :] - samples[None]) ** 2).sum(-1).min(1)
        assert (d <= dense + 1e-12).all()
        step = max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b)) / n
        assert (np.sqrt(dense) <= np.sqrt(d) + step + 1e-9).all()


def test_restated_residual_edges():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 9]])                       # the second face names a vertex that does not exist
    eye = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    assert mr.residual_one(v, f, (0, 3), (0, 2), eye) == 0.0
    assert mr.residual_one(v, f, (0, 4), (0, 2), eye) == np.inf            # the NaN vertex
    assert mr.residual_one(v, f, (0, 3), (1, 1), eye) == np.inf            # only the skipped face
    assert mr.residual_one(v, f, (0, 3), (0, 0), eye) == np.inf            # no faces
    assert mr.residual_one(v, f, (0, 0), (0, 2), eye) == 0.0               # no vertices
    up = eye.copy()
    up[11] = 2.0
    assert mr.residual_one(v, f, (0, 3), (0, 2), up) == 4.0
    r = mr.residual(v, f, [[0, 3]], [[0, 2]], np.stack([eye, up, eye]), [[0, 2]])
    assert list(r[:2]) == [0.0, 4.0] and np.isnan(r[2])                    # nobody owns the third


def test_entry_points_refuse_on_the_host():
    lib = _lib.lib()
    N = ctypes.c_void_p(0)
    p = [ctypes.c_void_p(0x10000 * (k + 1)) for k in range(8)]             # 64 KiB apart: no span below reaches the next
    ext = lib.krrn_model_extent_f64  # verts, Vtot, vert_range, O, max_v, d2, box, stream
    for null in (0, 2, 5, 6):
        a = [p[0], 10, p[1], 2, 10, p[2], p[3], N]
        a[null] = N
        assert ext(*a) == -1, null
    for bad in (dict(Vtot=0), dict(O=0), dict(O=65536), dict(max_v=0)):
        k = {"Vtot": 10, "O": 2, "max_v": 10, **bad}
        assert ext(p[0], k["Vtot"], p[1], k["O"], k["max_v"], p[2], p[3], N) == -2, bad
    assert ext(N, 0, p[1], 2, 10, p[2], p[3], N) == -1                      # a null pointer before a bad shape
    assert ext(p[0], 10, p[1], 2, 10, p[2], p[2], N) == -1                  # d2 and box overlap
    assert ext(p[0], 10, p[1], 2, 10, p[0], p[3], N) == -1                  # d2 over verts
    assert ext(p[0], 10, p[1], 2, 10, p[2], ctypes.c_void_p(p[1].value + 8), N) == -1   # box over vert_range's end

    # verts, Vtot, faces, Ftot, vert_range, face_range, syms, NStot, sym_range, O, max_v, max_f, res2, stream
    res = lib.krrn_symmetry_residual_f64

    def call(null=None, res2=None, **kw):
        k = dict(Vtot=10, Ftot=5, NStot=3, O=2, max_v=10, max_f=5)
        k.update(kw)
        a = [p[0], k["Vtot"], p[1], k["Ftot"], p[2], p[3], p[4], k["NStot"], p[5], k["O"], k["max_v"], k["max_f"],
             p[6] if res2 is None else res2, N]
        if null is not None:
            a[null] = N
        return res(*a)
    for null in (0, 2, 4, 5, 6, 8, 12):
        assert call(null=null) == -1, null
    for bad in (dict(O=0), dict(Vtot=0), dict(NStot=0), dict(max_v=0), dict(max_f=0), dict(Ftot=-1),
                dict(NStot=1 << 23, max_v=257)):
        assert call(**bad) == -2, bad
    assert call(null=0, O=0) == -1
    for over in (0, 1, 2, 3, 4, 5):                                         # res2 over each input
        assert call(res2=p[over]) == -1, over


def test_wrappers_raise_on_cpu_tensors():
    v, f = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    r = torch.tensor([[0, 4]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP path only"):
        models.extent(v, r)
    with pytest.raises(RuntimeError, match="HIP path only"):
        models.symmetry_residual(v, f, r, torch.tensor([[0, 2]]), torch.zeros((1, 12), dtype=torch.float64),
                                 torch.tensor([[0, 1]]))
    assert all(isinstance(c, int) and c >= 64 for c in (models.EXTENT_R, models.EXTENT_C, models.RESIDUAL_R,
                                                         models.RESIDUAL_C))


def test_write_models_info_refuses_an_existing_file(tmp_path):
    root = str(tmp_path)
    bop_tree.write_models(root)
    path = os.path.join(root, "models", "models_info.json")
    before = open(path).read()
    with pytest.raises(FileExistsError, match="overwrite=True"):
        bop_scene.write_models_info(root, "cuda:0")
    assert open(path).read() == before
