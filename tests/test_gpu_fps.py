"""krrn_fps_f32 at the edges of its layout: each of the 1024 threads holds 16 register slots, slot k
of thread t being point t + 1024 k, so n = 1024 fills slot 0 exactly, 1025 and 2049 put a single
point in the next slot; n = 1 leaves 1023 threads with nothing; coincident points make every
distance 0, where only the tie rule (lowest index) decides. Indices equal oracle.fps_oracle exactly."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.fps_oracle import farthest_point_sampling as fps_ref


def _points(n, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "coincident":
        return np.tile(np.array([[0.03, -0.01, 0.07]], np.float32), (n, 1))
    if kind == "lattice":  # 3 x 3 x 3 sites, each held by several points: all distances 0 after 27 picks
        g = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
        return (g[rng.integers(0, len(g), n)] * 0.01).astype(np.float32)
    return (rng.random((n, 3)) * np.array([0.1, 0.08, 0.05])).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("n,ns,kind", [(1, 3, "rand"), (1024, 6, "rand"), (1025, 6, "rand"), (2049, 5, "rand"),
                                       (300, 300, "coincident"), (300, 300, "lattice")])
def test_fps_slot_edges_and_ties(dev, n, ns, kind):
    from pose_estimation_amd.fps import farthest_point_sampling
    pts = _points(n, kind, seed=n + ns)
    if kind == "rand" and n > 1024:  # the lone point of the last slot is an extreme one: it must be picked
        pts[n - 1] = [0.5, 0.5, 0.5]
    ref = fps_ref(pts, ns)
    if n == 1 or kind == "coincident":
        assert not ref.any()
    if kind == "lattice":
        assert len(set(ref[:27].tolist())) == 27 and not ref[27:].any()  # then only the tie rule is left
    if kind == "rand" and n > 1024:
        assert ref[1] == n - 1
    got = farthest_point_sampling(torch.from_numpy(pts).to(dev), ns).cpu().numpy()
    assert np.array_equal(got, ref), np.nonzero(got != ref)[0][:5]


@pytest.mark.gpu
def test_fps_five_unrelated_sets(dev):
    from pose_estimation_amd.fps import farthest_point_sampling
    batch = np.stack([_points(1500, "rand", seed=40 + b) for b in range(5)])
    got = farthest_point_sampling(torch.from_numpy(batch).to(dev), 20).cpu().numpy()
    refs = np.stack([fps_ref(batch[b], 20) for b in range(5)])
    assert len({tuple(r) for r in refs.tolist()}) == 5  # the sets' answers differ: a set mix-up shows
    assert np.array_equal(got, refs)


def test_fps_rejects_more_points_than_slots():
    """n = 16385 > 1024 x 16: KRRN_ESHAPE before any launch (no GPU needed: the pointers are never
    read)."""
    from pose_estimation_amd import _lib
    fn = _lib.lib().krrn_fps_f32
    pts = np.zeros((16385, 3), np.float32)
    out = np.zeros(4, np.int32)
    assert fn(pts.ctypes.data_as(ctypes.c_void_p), 1, 16385, 4, out.ctypes.data_as(ctypes.c_void_p), None) == -2
    assert fn(pts.ctypes.data_as(ctypes.c_void_p), 1, 0, 4, out.ctypes.data_as(ctypes.c_void_p), None) == -2
