"""krrn_rle_encode_u8 / krrn_rle_encode_ws without a GPU: every host-side argument check of the entry points
(made before any HIP call, so the pointers are never dereferenced), their ABI signatures, and the refusals of
rle.encode_gpu that come before a device is touched."""
import ctypes

import numpy as np
import pytest
import torch

from pose_estimation_amd import _lib, rle

EARG, ESHAPE = -1, -2
N = ctypes.c_void_p(0)
NAMES = ("mask", "ws", "counts", "n_runs", "info")


def _call(n=2, H=48, W=64, max_runs=16, **over):
    p = {k: ctypes.c_void_p((i + 1) << 36) for i, k in enumerate(NAMES)}   # never dereferenced
    p.update(over)
    return _lib.lib().krrn_rle_encode_u8(p["mask"], n, H, W, max_runs, p["ws"], p["counts"], p["n_runs"], p["info"], N)


def test_abi_lists_the_entry_points():
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["krrn_rle_encode_u8"] == [P, I, I, I, I, P, P, P, P, P]
    assert _lib.SIGNATURES["krrn_rle_encode_ws"] == [I, I, P]


@pytest.mark.parametrize("name", NAMES)
def test_null_pointer_is_earg(name):
    assert _call(**{name: N}) == EARG
    assert _call(n=0, **{name: N}) == EARG and _call(H=0, **{name: N}) == EARG   # pointers are checked first


@pytest.mark.parametrize("bad", [dict(n=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-1), dict(H=65536, W=32768),
                                 dict(H=46341, W=46341), dict(max_runs=0), dict(max_runs=-5)])
def test_bad_shape_is_eshape(bad):
    assert _call(**bad) == ESHAPE
    assert _call(**dict(dict(n=0), **bad)) == ESHAPE     # shapes are checked before the n == 0 return


def test_no_mask_returns_ok_without_a_launch():
    assert _call(n=0) == 0
    assert _call(n=0, H=32768, W=65535) == 0             # H * W = 2^31 - 32768 fits
    assert _call(n=0, max_runs=1) == 0


def test_workspace_size():
    fn = _lib.lib().krrn_rle_encode_ws
    out = ctypes.c_longlong(-1)
    assert fn(3, 640, N) == EARG
    assert fn(-1, 640, ctypes.byref(out)) == ESHAPE and fn(3, 0, ctypes.byref(out)) == ESHAPE and out.value == -1
    assert fn(0, 640, ctypes.byref(out)) == 0 and out.value == 0
    assert fn(3, 640, ctypes.byref(out)) == 0 and out.value > 0 and out.value % (3 * 640) == 0
    per = out.value // (3 * 640)
    assert fn(70000, 65535, ctypes.byref(out)) == 0 and out.value == per * 70000 * 65535    # past 2^31: no wrap


def test_encode_gpu_refuses_before_touching_a_device():
    plane = torch.zeros((2, 8, 6), dtype=torch.uint8)
    for fn in (rle.encode_gpu, rle.encode_planes):
        with pytest.raises(RuntimeError, match="HIP path only"):
            fn(plane)                                    # a CPU tensor: no host fallback
        with pytest.raises(RuntimeError, match="HIP path only"):
            fn(plane[0] != 0)                            # bool [H, W]
        with pytest.raises(ValueError, match="contiguous"):
            fn(plane[:, ::2])
        with pytest.raises(ValueError, match="contiguous"):
            fn(plane.transpose(1, 2))
        with pytest.raises(ValueError, match="u8 or bool"):
            fn(plane.to(torch.int32))
        with pytest.raises(ValueError, match="u8 or bool"):
            fn(plane[0, 0])
        with pytest.raises(ValueError, match="u8 or bool"):
            fn(np.zeros((4, 6), np.uint8))
        with pytest.raises(ValueError, match="max_runs"):
            fn(plane, max_runs=0)
