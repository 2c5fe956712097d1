"""krrn_mask_paste_f32 and what sits on it, without a GPU: the entry point's ABI signature and every host-side
argument check (made before any HIP call, so the pointers are never dereferenced), the refusals of rle.paste_masks that
come before a device is touched, tests/paste_ref.py against a per-pixel Python loop on hand cases,
bop_scene.net_mask_rows, and evaluate.test_epoch's seg_source argument errors."""
import ctypes
import math

import numpy as np
import pytest
import torch

import paste_ref as pr
from pose_estimation_amd import _lib, bop_scene, rle

EARG, ESHAPE = -1, -2
N = ctypes.c_void_p(0)
NAMES = ("logits", "chan", "rc", "mask", "info")
I32_MAX = 0x7fffffff


def _call(ld_b=None, C1=2, S=40, B=3, H=48, W=64, **over):
    p = {k: ctypes.c_void_p((i + 1) << 36) for i, k in enumerate(NAMES)}   # never dereferenced
    p.update(over)
    ld_b = C1 * S * S if ld_b is None else ld_b
    return _lib.lib().krrn_mask_paste_f32(p["logits"], ld_b, C1, S, p["chan"], p["rc"], B, H, W, p["mask"], p["info"], N)


def test_abi_lists_the_entry_point():
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.SIGNATURES["krrn_mask_paste_f32"] == [P, L, I, I, P, P, I, I, I, P, P, P]


@pytest.mark.parametrize("name", NAMES)
def test_null_pointer_is_earg(name):
    assert _call(**{name: N}) == EARG
    assert _call(B=0, **{name: N}) == EARG and _call(H=0, **{name: N}) == EARG   # pointers are checked first


@pytest.mark.parametrize("bad", [dict(B=-1), dict(C1=0), dict(C1=-2), dict(S=0), dict(S=-1), dict(H=0), dict(H=-3),
                                 dict(W=0), dict(W=-1), dict(H=65536, W=32768), dict(H=46341, W=46341),
                                 dict(C1=2, S=32768), dict(C1=1, S=46341), dict(C1=I32_MAX, S=I32_MAX),
                                 dict(ld_b=2 * 40 * 40 - 1), dict(ld_b=0), dict(ld_b=-(1 << 40))])
def test_bad_shape_is_eshape(bad):
    assert _call(**bad) == ESHAPE
    assert _call(**dict(dict(B=0), **bad)) == ESHAPE     # shapes are checked before the B == 0 return


def test_overlap_is_earg():
    base = 1 << 36                                       # logits: 3 crops of 2 x 40 x 40 floats from here
    crop = 2 * 40 * 40 * 4
    assert _call(mask=ctypes.c_void_p(base)) == EARG
    assert _call(mask=ctypes.c_void_p(base + 3 * crop - 1)) == EARG          # the logits' last byte
    assert _call(mask=ctypes.c_void_p(base - 1)) == EARG                     # the mask's planes reach into the logits
    assert _call(info=ctypes.c_void_p(base + 100)) == EARG
    assert _call(info=ctypes.c_void_p((4 << 36) + 5)) == EARG                # info inside mask: two outputs
    assert _call(mask=ctypes.c_void_p((2 << 36) + 3)) == EARG                # mask over chan
    assert _call(info=ctypes.c_void_p((3 << 36) + 8)) == EARG                # info over rc
    # a batch stride wider than the crop: the extent is (B - 1) ld_b + C1 S S floats
    wide = 3 * crop // 4
    assert _call(ld_b=wide, mask=ctypes.c_void_p(base + (2 * wide + crop // 4) * 4 - 1)) == EARG
    assert _call(ld_b=1 << 62, B=2, mask=ctypes.c_void_p(5 << 36)) == EARG   # an extent past the address space: no wrap


def test_no_crop_returns_ok_without_a_launch():
    # B == 0 launches nothing, so placeholder addresses are safe; every extent is empty, so nothing overlaps either
    assert _call(B=0) == 0
    assert _call(B=0, H=32768, W=65535) == 0             # H * W = 2^31 - 32768 fits
    assert _call(B=0, C1=1, S=46340) == 0                # C1 S S = 2^31 - 88047 fits
    assert _call(B=0, ld_b=1 << 40) == 0
    assert _call(B=0, mask=ctypes.c_void_p(1 << 36)) == 0


def test_paste_masks_refuses_before_touching_a_device():
    l = torch.zeros((3, 2, 8, 8), dtype=torch.float32)
    chan, rc = [1, 1, 1], [[0, 0]] * 3
    with pytest.raises(RuntimeError, match="HIP path only"):
        rle.paste_masks(l, chan, rc, 20, 30)             # a CPU tensor: no host fallback
    with pytest.raises(RuntimeError, match="HIP path only"):
        rle.paste_masks(torch.zeros((3, 5, 8, 8))[:, 0:2], chan, rc, 20, 30)   # a channel slice is a legal view
    for bad in (l.double(), l.half(), l.to(torch.int32), l[0], l[:, :, :, 0], l.reshape(3, 2, 4, 16), np.zeros((3, 2, 8, 8), np.float32)):
        with pytest.raises(ValueError, match="f32 .B, C1, S, S."):
            rle.paste_masks(bad, chan, rc, 20, 30)
    wide = torch.zeros((3, 2, 8, 16))
    for bad in (l.transpose(2, 3), l.transpose(0, 1), wide[:, :, :, ::2], wide[:, :, :, 0:8],
                torch.zeros((3, 2, 16, 8))[:, :, ::2], torch.zeros((2, 3, 8, 8)).transpose(0, 1)[:, :, :, :],
                l[0:1].expand(3, 2, 8, 8)):
        assert tuple(bad.shape) in ((3, 2, 8, 8), (2, 3, 8, 8))
        with pytest.raises(ValueError, match="strides"):
            rle.paste_masks(bad, [1] * bad.shape[0], [[0, 0]] * bad.shape[0], 20, 30)
    for H, W in ((0, 30), (20, -1), (65536, 32768)):
        with pytest.raises(ValueError, match="frame"):
            rle.paste_masks(l, chan, rc, H, W)
    for out in (torch.zeros((3, 20, 31), dtype=torch.uint8), torch.zeros((2, 20, 30), dtype=torch.uint8),
                torch.zeros((3, 20, 30), dtype=torch.int32), torch.zeros((3, 20, 60), dtype=torch.uint8)[:, :, ::2],
                torch.zeros((3, 600), dtype=torch.uint8), np.zeros((3, 20, 30), np.uint8)):
        with pytest.raises(ValueError, match="out must be"):
            rle.paste_masks(l, chan, rc, 20, 30, out=out)


def _loop(logits, chan, rc, H, W):
    """Independent of paste_ref: one frame pixel at a time, the walk written with math.isnan."""
    l = np.asarray(logits, np.float32)
    B, C1, S, _ = l.shape
    mask = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                i, j = y - int(rc[b][0]), x - int(rc[b][1])
                if not (0 <= i < S and 0 <= j < S):
                    continue
                v = [float(l[b, c, i, j]) for c in range(C1)]
                best = 0
                for c in range(1, C1):
                    if not math.isnan(v[c]) and not math.isnan(v[best]) and v[c] > v[best]:
                        best = c
                ch = int(chan[b])
                mask[b, y, x] = (best == ch) if 1 <= ch < C1 else (best != 0 if ch == 0 else False)
    info = []
    for m in mask:
        ys, xs = np.nonzero(m)
        info.append([len(ys), xs.min(), ys.min(), xs.max() - xs.min(), ys.max() - ys.min()] if len(ys) else [0] * 5)
    return mask, np.asarray(info, np.int32).reshape(B, 5)


def test_paste_ref_against_a_pixel_loop():
    nan, inf = float("nan"), float("inf")
    # 1 x 1 windows, C1 = 3: [l0, l1, l2] -> best
    for v, best in (([0.0, 1.0, 2.0], 2), ([0.0, 1.0, 1.0], 1), ([1.0, 1.0, 0.0], 0), ([-0.0, 0.0, -1.0], 0),
                    ([0.0, -0.0, 0.0], 0), ([nan, 5.0, 6.0], 0), ([0.0, nan, -1.0], 0), ([0.0, nan, 1.0], 2),
                    ([nan, nan, nan], 0), ([-inf, -inf, -inf], 0), ([-inf, inf, inf], 1), ([inf, inf, 0.0], 0),
                    ([-1.0, nan, -0.5], 2)):
        l = np.asarray(v, np.float32).reshape(3, 1, 1)
        assert int(pr.decide(l)[0, 0]) == best, v
        assert [int(pr.window(l, ch)[0, 0]) for ch in (-1, 0, 1, 2, 3)] == [0, int(best != 0), int(best == 1), int(best == 2), 0], v
    assert int(pr.window(np.ones((1, 1, 1), np.float32), 0)[0, 0]) == 0     # C1 = 1: no foreground channel
    rng = np.random.default_rng(3)
    l = rng.standard_normal((6, 3, 5, 5)).astype(np.float32)
    l[0, :, 1, 1] = nan
    l[1, 0, 2, :] = nan
    l[2, 2] = l[2, 1]                                    # ties between the foreground channels
    l[3, 1] = l[3, 0]                                    # ties with background
    chan = [1, 0, 1, 2, 3, -1]
    rc = [[0, 0], [4, 6], [-2, -3], [5, 7], [1, 1], [2, 2]]   # inside, flush bottom right, cut top left, cut bottom right
    want = _loop(l, chan, rc, 9, 11)
    got = pr.paste(l, chan, rc, 9, 11)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[0][:4].any(1).any(1).all() and not got[0][4:].any()
    assert not pr.window(l[2], 2).any() and not pr.window(l[3], 1).any()   # a tie goes to the lower channel
    far = pr.paste(l[:2], [1, 1], [[-2 ** 31, 2 ** 31 - 1], [2 ** 31 - 1, -2 ** 31]], 9, 11)
    assert not far[0].any() and not far[1].any()
    one = np.zeros((1, 2, 4, 4), np.float32)
    one[0, 1, 2, 3] = 1.0                                # a single set pixel: w = h = 0
    assert pr.paste(one, [1], [[3, 1]], 9, 11)[1].tolist() == [[1, 4, 5, 0, 0]]


def _rows(n):
    return [{"scene_id": 1 + k // 2, "im_id": 10 * k, "obj_id": 3 - k % 3, "score": 0.25 * k, "R": np.eye(3),
             "t": np.arange(3.0), "time": -1.0 if k % 2 else 0.5 * k} for k in range(n)]


def test_net_mask_rows(tmp_path):
    H, W = 6, 7
    planes = np.zeros((4, H, W), np.uint8)
    planes[0, 1:3, 2:6] = 1
    planes[2, 5, 6] = 1                                  # one pixel; planes 1 and 3 stay empty
    runs = [rle.encode(p) for p in planes]
    info = np.stack([pr.rf.info(p) for p in planes])
    rows = _rows(4)
    det, st = bop_scene.net_mask_rows(rows, runs, info, H, W)
    assert st == {"empty": 2} and len(det) == 2
    assert [(d["scene_id"], d["image_id"], d["category_id"]) for d in det] == [(1, 0, 3), (2, 20, 1)]   # the rows' order
    assert det[0] == {"scene_id": 1, "image_id": 0, "category_id": 3, "score": 0.0, "bbox": [2.0, 1.0, 3.0, 1.0],
                      "segmentation": {"counts": runs[0], "size": [H, W]}, "time": 0.0}
    assert det[1]["bbox"] == [6.0, 5.0, 0.0, 0.0] and det[1]["score"] == 0.5 and det[1]["time"] == 1.0
    assert all(type(v) is float for d in det for v in d["bbox"] + [d["score"], d["time"]])
    assert bop_scene._check_rows(det, "det") == det      # the normal form already
    path = str(tmp_path / "seg.json")
    bop_scene.write_detections(path, det)
    assert bop_scene.read_detections(path) == det
    # info as device-style int32 rows or plain lists, runs as numpy arrays: the same rows
    again, _ = bop_scene.net_mask_rows(rows, [np.asarray(r, np.int32) for r in runs], info.tolist(), H, W)
    assert again == det
    assert bop_scene.net_mask_rows([], [], [], H, W) == ([], {"empty": 0})
    with pytest.raises(ValueError, match="one of each"):
        bop_scene.net_mask_rows(rows, runs[:3], info, H, W)


def test_epoch_argument_errors(tmp_path):
    """Raised before the model or a batch is touched: the model is a dummy."""
    import bop_tree
    from pose_estimation_amd.dataset import PoseDataset
    from pose_estimation_amd.evaluate import test_epoch as run_epoch
    root = str(tmp_path / "tree")
    bop_tree.write_tree(root)
    dummy = torch.nn.Linear(1, 1)
    ds = PoseDataset("test", 500, False, root, 0.0, 8, n_model_pts=4, layout="bop")
    seg = str(tmp_path / "seg.json")
    with pytest.raises(ValueError, match="seg_source must be 'render' or 'net'"):
        run_epoch(dummy, ds, bs=3, device="cpu", seg_json=seg, seg_source="bogus")
    with pytest.raises(ValueError, match="seg_source must be 'render' or 'net'"):
        run_epoch(dummy, ds, bs=3, device="cpu", seg_source=None)
    with pytest.raises(ValueError, match="seg_source='net'.*needs seg_json"):
        run_epoch(dummy, ds, bs=3, device="cpu", seg_source="net")
    lm = PoseDataset("test", 500, False, None, 0.0, 8, cls_type="all", num_frames=2)
    with pytest.raises(ValueError, match="seg_source='net'.*layout='bop'"):
        run_epoch(dummy, lm, bs=2, device="cpu", seg_json=seg, seg_source="net")
    with pytest.raises(ValueError, match="seg_source='net' runs on one rank"):
        run_epoch(dummy, ds, bs=3, device="cpu", seg_json=seg, seg_source="net", world=2, rank=0)
    with pytest.raises(ValueError, match="seg_json.*layout='bop'.*meshes=True"):          # the default is today's check
        run_epoch(dummy, ds, bs=3, device="cpu", seg_json=seg, seg_source="render")
    import os
    assert not os.path.exists(seg)
