"""The resized input kernels (krrn_crop_inputs_resize_u8, krrn_choose_points_resize) called directly, every output
between sentinel guards: bit-identical to the native-size entry points when every side equals T, and equal bit for
bit to tests/resize_ref.py's restatement on batches that mix sides, up and down, at the frame's corners."""
import numpy as np
import pytest
import torch

from pose_estimation_amd import _lib
from pose_estimation_amd._lib import P, stream_ptr
from pose_estimation_amd.dataset import get_square_bbox, synthetic_frames
from pose_estimation_amd.synthetic import LM_K
from tests import draws_ref as D
from tests import resize_ref as R
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu

K4 = [LM_K[0, 0], LM_K[1, 1], LM_K[0, 2], LM_K[1, 2]]
EARG, ESHAPE = -1, -2
H, W = 480, 640


def _dev(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _k4(B):
    return np.array([[K4[0] * (1 + 0.01 * b), K4[1] * (1 - 0.02 * b), K4[2] + 3 * b, K4[3] - 5 * b]
                     for b in range(B)], np.float32)


def _inputs(dev, fr, frame, rc, side, k4, seed):
    return {"rgb": _dev(dev, fr["rgb"]), "depth": _dev(dev, fr["depth"]), "ml": _dev(dev, fr["mask_label"]),
            "frame": _dev(dev, np.asarray(frame, np.int32)), "rc": _dev(dev, np.asarray(rc, np.int32)),
            "side": _dev(dev, np.asarray(side, np.int32)), "k4": _dev(dev, k4),
            "seed": torch.tensor([seed], dtype=torch.int64, device=dev)}


def _outputs(dev, B, T, N):
    return {"img": Guarded(dev, (B, 3, T, T), torch.float32), "mask": Guarded(dev, (B, T * T), torch.uint8),
            "choose": Guarded(dev, (B, N), torch.int64), "cloud": Guarded(dev, (B, N, 3), torch.float32),
            "xmap": Guarded(dev, (B, N), torch.float32), "ymap": Guarded(dev, (B, N), torch.float32),
            "count": Guarded(dev, (B,), torch.int32)}


def _crop_args(ins, out, F, B, T):
    return [P(ins["rgb"].data_ptr()), P(ins["depth"].data_ptr()), P(ins["ml"].data_ptr()), P(0), F, H, W,
            P(ins["frame"].data_ptr()), P(ins["rc"].data_ptr()), P(ins["side"].data_ptr()), B, T, P(out["img"].ptr),
            P(out["mask"].ptr)]


def _choose_args(ins, out, B, T, N, depth_scale, stream_id):
    return [P(out["mask"].ptr), B, T, N, P(ins["depth"].data_ptr()), H, W, P(ins["frame"].data_ptr()),
            P(ins["rc"].data_ptr()), P(ins["side"].data_ptr()), P(ins["k4"].data_ptr()), float(depth_scale),
            P(ins["seed"].data_ptr()), stream_id, P(out["choose"].ptr), P(out["cloud"].ptr), P(out["xmap"].ptr),
            P(out["ymap"].ptr), P(out["count"].ptr)]


def _run(dev, fr, frame, rc, side, T, N, k4, depth_scale, seed, stream_id):
    """Both launches on the current stream; every output read back through its guards."""
    B, F = len(frame), len(fr["depth"])
    ins, out = _inputs(dev, fr, frame, rc, side, k4, seed), _outputs(dev, B, T, N)
    lib = _lib.lib()
    assert lib.krrn_crop_inputs_resize_u8(*_crop_args(ins, out, F, B, T), stream_ptr(dev)) == 0
    assert lib.krrn_choose_points_resize(*_choose_args(ins, out, B, T, N, depth_scale, stream_id), stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    return {k: v.get() for k, v in out.items()}


@pytest.mark.parametrize("T,N", [(40, 300), (120, 1000)])
def test_identity_with_the_native_entry_points(dev, T, N):
    """Every side == T: all seven outputs equal krrn_crop_inputs_u8 + krrn_choose_points on the same frames, seed and
    stream id (weights 0, nearest pixel = the pixel itself, centre = its integer coordinate)."""
    B = 3
    fr = synthetic_frames(B, seed=T, sizes=[T])
    boxes = [get_square_bbox([float(v) for v in bb]) for bb in fr["bbox"]]
    assert all(b[1] - b[0] == T and b[3] - b[2] == T for b in boxes)
    frame, rc, k4 = [2, 0, 1], [(boxes[f][0], boxes[f][2]) for f in (2, 0, 1)], _k4(B)
    got = _run(dev, fr, frame, rc, [T] * B, T, N, k4, 2.0, seed=1234, stream_id=3)
    ins = _inputs(dev, fr, frame, rc, [T] * B, k4, 1234)
    ref = _outputs(dev, B, T, N)
    lib = _lib.lib()
    a = _crop_args(ins, ref, B, B, T)
    assert lib.krrn_crop_inputs_u8(*a[:9], B, T, a[12], a[13], stream_ptr(dev)) == 0
    c = _choose_args(ins, ref, B, T, N, 2.0, 3)
    assert lib.krrn_choose_points(*c[:9], *c[10:], stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert got["count"].min() > 0 and (got["count"] > N).any() and (T != 40 or (got["count"] < N).any())
    for k, v in ref.items():
        r = v.get()
        same = np.array_equal(got[k].view(np.uint32), r.view(np.uint32)) if r.dtype == np.float32 else np.array_equal(got[k], r)
        assert same, k


# ---- batches that mix sides, against the restatement ----

def _mixed_frames(seed):
    """Three synthetic frames whose label mask is replaced by noise of density 0.9 (frame 0: crops there hold more
    pixels than N), 0.3 (frame 1: fewer) and, on frame 2, nothing inside its top-left 240 x 240 (an empty crop)."""
    fr = dict(synthetic_frames(3, seed=seed, sizes=[120]))
    rng = np.random.default_rng(seed)
    ml = np.stack([(rng.random((H, W)) < d) * 255 for d in (0.9, 0.3, 0.9)]).astype(np.uint8)
    ml[2, :240, :240] = 0
    fr["mask_label"] = ml
    return fr


BATCHES = {
    # T, N, then per crop (frame, r0, c0, side): the first window at the frame's top-left corner, the last-but-one at
    # its bottom-right, the last the empty one; frames repeated and out of order
    "down": (40, 1000, [(1, 0, 0, 40), (0, 100, 37, 80), (0, 211, 333, 120), (1, 50, 420, 200), (0, H - 200, W - 200, 200),
                        (1, H - 40, W - 40, 40), (2, 3, 7, 120)]),
    "updown": (80, 3000, [(0, 0, 0, 40), (1, 17, 301, 120), (0, 301, 17, 120), (1, H - 40, W - 40, 40),
                          (0, H - 120, W - 120, 120), (2, 100, 60, 40)]),
}
_CACHE = {}


def _batch(dev, name):
    if name not in _CACHE:
        T, N, crops = BATCHES[name]
        fr = _mixed_frames(seed=T)
        B = len(crops)
        k4 = _k4(B)
        got = _run(dev, fr, [c[0] for c in crops], [(c[1], c[2]) for c in crops], [c[3] for c in crops], T, N, k4, 2.0,
                   seed=77, stream_id=9)
        ref = [R.crop(fr["rgb"][f], fr["depth"][f], fr["mask_label"][f], r0, c0, S, T, N, k4[b], 2.0, seed=77,
                      stream_id=9, index=b) for b, (f, r0, c0, S) in enumerate(crops)]
        _CACHE[name] = (got, ref)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(BATCHES))
def test_mixed_sides_match_the_restatement(dev, name):
    """"down": sides 40, 80, 120, 200 at T = 40 (1x, 2x, 3x, 5x down). "updown": sides 40 and 120 at T = 80 (2x up with
    the clamped left tap -1 and right tap S - 1, 1.5x down with fractional weights). Per-crop K4, depth_scale 2, one
    crop that wraps, one that subsets, one that is empty."""
    T, N, crops = BATCHES[name]
    got, ref = _batch(dev, name)
    counts = [r["count"] for r in ref]
    assert counts[-1] == 0 and any(0 < c < N for c in counts) and any(c > N for c in counts), counts
    assert len({c[3] for c in crops}) >= 2
    for b, r in enumerate(ref):
        assert int(got["count"][b]) == r["count"], b
        assert np.array_equal(got["img"][b].view(np.uint32), r["img"].view(np.uint32)), b
        assert np.array_equal(got["mask"][b], r["mask"]), b
        assert np.array_equal(got["choose"][b], r["choose"]), b
        assert np.array_equal(got["cloud"][b].view(np.uint32), r["cloud"].view(np.uint32)), b
        assert np.array_equal(got["xmap"][b], r["xmap"]) and np.array_equal(got["ymap"][b], r["ymap"]), b
    # the empty crop: zeros everywhere
    assert not got["choose"][-1].any() and not got["cloud"][-1].any() and not got["xmap"][-1].any()
    # an enlarged crop's maps are fractional, and every map stays inside its source window
    for b, (f, r0, c0, S) in enumerate(crops[:-1]):
        assert (got["xmap"][b] >= c0 - 0.5).all() and (got["xmap"][b] <= c0 + S - 0.5).all()
        assert (got["ymap"][b] >= r0 - 0.5).all() and (got["ymap"][b] <= r0 + S - 0.5).all()
        if (R.centre(S, T) % 1 != 0).all():  # 2x down, 2x up, 1.5x down (3x and 5x down land on pixel centres)
            assert (got["xmap"][b] != np.round(got["xmap"][b])).all() and (got["ymap"][b] % 1 != 0).all()


def test_choose_keys_mix_the_crop_index(dev):
    """The subset of crop b is the restatement's for index b over the resized mask, not index 0's."""
    T, N, crops = BATCHES["down"]
    got, ref = _batch(dev, "down")
    seen = 0
    for b in range(1, len(crops)):
        if ref[b]["count"] <= N:
            continue
        seen += 1
        assert np.array_equal(got["choose"][b], D.choose(ref[b]["mask"], N, seed=77, stream_id=9, crop=b))
        assert not np.array_equal(got["choose"][b], D.choose(ref[b]["mask"], N, seed=77, stream_id=9, crop=0))
    assert seen >= 1


def test_host_refusals(dev):
    """Null pointers KRRN_EARG (obj_mask may be NULL); T = 0 and 4097, B = 0 and 65536, N = 0, depth_scale = 0 and
    stream ids outside 0 .. 65534 KRRN_ESHAPE; nothing is launched, every output keeps its sentinel."""
    T, N, B = 40, 50, 2
    fr = synthetic_frames(1, seed=1, sizes=[40])
    ins = _inputs(dev, fr, [0, 0], [(0, 0), (10, 10)], [40, 80], _k4(B), 5)
    out = _outputs(dev, B, T, N)
    lib = _lib.lib()
    st = stream_ptr(dev)
    good_c, good_p = _crop_args(ins, out, 1, B, T), _choose_args(ins, out, B, T, N, 1.0, 0)
    for i in (0, 1, 2, 7, 8, 9, 12, 13):
        a = list(good_c)
        a[i] = P(0)
        assert lib.krrn_crop_inputs_resize_u8(*a, st) == EARG, i
    for i, v in [(11, 0), (11, 4097), (10, 0), (10, 65536), (4, 0)]:
        a = list(good_c)
        a[i] = v
        assert lib.krrn_crop_inputs_resize_u8(*a, st) == ESHAPE, (i, v)
    for i in (0, 4, 7, 8, 9, 10, 12, 14, 15, 16, 17, 18):
        a = list(good_p)
        a[i] = P(0)
        assert lib.krrn_choose_points_resize(*a, st) == EARG, i
    for i, v in [(2, 0), (2, 4097), (1, 0), (1, 65536), (3, 0), (11, 0.0), (13, 65535), (13, -1), (13, 65536)]:
        a = list(good_p)
        a[i] = v
        assert lib.krrn_choose_points_resize(*a, st) == ESHAPE, (i, v)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out.values())
