"""The resized input path on the host: its numpy restatement (tests/resize_ref.py) against the native-size oracle
and against the definition's own properties, the resize intrinsic, and PoseDataset(resize=T)'s one bucket and its
refusals. No GPU: nothing here launches a kernel."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import inputs_oracle as io
from pose_estimation_amd import _lib, evaluate
from pose_estimation_amd.dataset import (BucketBatcher, PoseDataset, build_inputs, get_square_bbox, resize_intrinsic,
                                         synthetic_frames)
from pose_estimation_amd.synthetic import LM_K
from tests import resize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4 = [LM_K[0, 0], LM_K[1, 1], LM_K[0, 2], LM_K[1, 2]]
GRID = [(S, T) for S in (40, 80, 120, 200, 480) for T in (40, 80, 120)]


@pytest.mark.parametrize("S,N", [(40, 500), (80, 1000)])
def test_restatement_is_the_native_oracle_when_sizes_agree(S, N):
    """S == T: image, mask, maps and cloud equal oracle.inputs_oracle's bit for bit (a subset and a wrap case)."""
    fr = synthetic_frames(2, seed=S, sizes=[S])
    for f in range(2):
        rmin, rmax, cmin, _ = get_square_bbox([float(v) for v in fr["bbox"][f]])
        assert rmax - rmin == S
        got = R.crop(fr["rgb"][f], fr["depth"][f], fr["mask_label"][f], rmin, cmin, S, S, N, K4, 2.0, seed=5,
                     stream_id=1, index=f)
        img, m = io.crop_inputs(fr["rgb"][f], fr["depth"][f], fr["mask_label"][f], rmin, cmin, S)
        assert np.array_equal(got["img"].view(np.uint32), img.view(np.uint32))
        assert np.array_equal(got["mask"], m.reshape(-1).astype(np.uint8)) and got["count"] == int(m.sum()) > 0
        cloud, xm, ym = io.points(got["choose"], fr["depth"][f], rmin, cmin, S, K4, 2.0)
        assert np.array_equal(got["cloud"].view(np.uint32), cloud.view(np.uint32))
        assert np.array_equal(got["xmap"], xm) and np.array_equal(got["ymap"], ym)


@pytest.mark.parametrize("S,T", GRID)
def test_index_ranges(S, T):
    x0, xa, xb, w = R.taps(S, T)
    n = R.nearest(S, T)
    assert xa.min() >= 0 and xb.max() <= S - 1 and (xa <= xb).all()
    assert n.min() >= 0 and n.max() <= S - 1 and (np.diff(n) >= 0).all()
    assert x0.min() >= -1 and x0.max() <= S - 1
    assert (w >= 0).all() and (w < 1).all()
    # the left tap falls off the window exactly when the crop is enlarged
    assert bool((x0 == -1).any()) == (S < T)
    # the first and the last centre are symmetric about the window's centre (S - 1) / 2: exactly in integers ...
    nx0, nxl = S - T, (2 * T - 1) * S - T
    assert nx0 + nxl == (S - 1) * 2 * T
    # ... and to rounding in the f64 the maps are made of
    c = R.centre(S, T)
    assert abs((c[0] + c[-1]) - (S - 1)) <= 4 * np.finfo(np.float64).eps * S
    if S == T:
        assert np.array_equal(x0, np.arange(T)) and (w == 0).all() and np.array_equal(n, np.arange(T))
        assert np.array_equal(c, np.arange(T, dtype=np.float64))


def test_downscale_by_two_gives_the_midpoints():
    """A window whose value is linear in row and column, halved: every output is the mean of its 2 x 2 source
    pixels, i.e. the plane's value at (2i + 0.5, 2j + 0.5), exactly (the sums are small integers over 4)."""
    S, T = 80, 40
    r, c = np.mgrid[0:S, 0:S]
    win = np.stack([r + c, 2 * r + 10, 255 - 3 * c], 2).astype(np.uint8)
    assert win.max() <= 255 and (np.stack([r + c, 2 * r + 10, 255 - 3 * c], 2) >= 0).all()
    p = R.bilinear(win, T)
    i, j = np.mgrid[0:T, 0:T]
    ri, cj = 2 * i + 0.5, 2 * j + 0.5
    want = np.stack([ri + cj, 2 * ri + 10, 255 - 3 * cj], 2)
    assert np.array_equal(p, want)
    x0, _, _, w = R.taps(S, T)
    assert np.array_equal(x0, 2 * np.arange(T)) and (w == 0.5).all()


@pytest.mark.parametrize("S,T", [(40, 120), (80, 120), (160, 80), (240, 120)])
def test_resize_intrinsic_projects_resized_pixel_indices(S, T):
    rng = np.random.default_rng(S + T)
    B = 6
    k4 = np.array([[K4[0] * (1 + 0.01 * b), K4[1] * (1 - 0.01 * b), K4[2] + b, K4[3] - b] for b in range(B)])
    boxes = []
    for b in range(B):
        r0, c0 = int(rng.integers(0, 480 - S + 1)), int(rng.integers(0, 640 - S + 1))
        boxes.append((r0, r0 + S, c0, c0 + S))
    s, intr = resize_intrinsic(torch.from_numpy(k4), boxes, T)
    assert s.dtype == np.float64 and intr.dtype == np.float64 and intr.shape == (B, 4)
    assert np.array_equal(s, np.full(B, S / T))
    for b in range(B):
        r0, _, c0, _ = boxes[b]
        # camera points that project inside the window
        u = c0 + rng.uniform(0, S, 50)
        v = r0 + rng.uniform(0, S, 50)
        Z = rng.uniform(0.5, 1.5, 50)
        X, Y = (u - k4[b, 2]) * Z / k4[b, 0], (v - k4[b, 3]) * Z / k4[b, 1]
        uf, vf = k4[b, 0] * X / Z + k4[b, 2], k4[b, 1] * Y / Z + k4[b, 3]
        ur, vr = intr[b, 0] * X / Z + intr[b, 2], intr[b, 1] * Y / Z + intr[b, 3]
        assert np.abs(ur - ((uf - c0 + 0.5) / s[b] - 0.5)).max() < 1e-12
        assert np.abs(vr - ((vf - r0 + 0.5) / s[b] - 0.5)).max() < 1e-12
    # the resized pixels' centres (the maps PnP reads) invert it: index j sits at frame column c0 + centre(j)
    ctr = R.centre(S, T)
    assert np.abs((c0 + ctr - c0 + 0.5) / s[-1] - 0.5 - np.arange(T)).max() < 1e-12


def test_one_bucket():
    kw = dict(mode="test", num_point=100, cls_type="all", num_frames=9, sizes=[80, 120, 160], n_model_pts=32)
    ds = PoseDataset(resize=120, **kw)
    assert ds.resize == 120 and [ds.crop_size(i) for i in range(len(ds))] == [120] * 9
    assert list(BucketBatcher(ds, bs=4).buckets()) == [120]
    assert [len(idx) for _, idx in BucketBatcher(ds, bs=4)] == [4, 4, 1]
    # the source windows keep their own sides
    assert sorted({b[1] - b[0] for b in ds.boxes}) == [80, 120, 160]
    plain = PoseDataset(**kw)
    assert plain.resize is None and list(BucketBatcher(plain, bs=4).buckets()) == [80, 120, 160]
    assert plain.boxes == ds.boxes


def test_refusals():
    with pytest.raises(ValueError, match="resize with gt_maps=True is not built"):
        PoseDataset(num_frames=2, resize=80, gt_maps=True)
    for bad in (0, 20, 39, 100, -40, 80.5):
        with pytest.raises(ValueError, match="multiple of 40"):
            PoseDataset(num_frames=2, resize=bad)
    ds = PoseDataset(num_frames=2, sizes=[80], n_model_pts=32, resize=80)
    with pytest.raises(ValueError, match="resize is not built"):
        evaluate.test_epoch(None, ds, device="cpu", seg_json="unused.json", seg_source="net")


def test_build_inputs_checks_the_windows_on_the_host():
    """The device reads each crop's side, so build_inputs(resize=) refuses a bad window before any launch (host
    tensors here: a launch would fail differently)."""
    fr = {"rgb": torch.zeros((1, 48, 64, 3), dtype=torch.uint8), "depth": torch.zeros((1, 48, 64)),
          "mask_label": torch.zeros((1, 48, 64), dtype=torch.uint8)}
    k4, seed = torch.tensor([K4], dtype=torch.float32), torch.zeros(1, dtype=torch.int64)
    for box, frame in [((0, 49, 0, 49), 0), ((-1, 39, 0, 40), 0), ((10, 50, 0, 40), 0), ((0, 40, 30, 70), 0),
                       ((0, 40, 0, 39), 0), ((5, 5, 5, 5), 0), ((0, 40, 0, 40), 1)]:
        with pytest.raises(ValueError, match="window|outside"):
            build_inputs(fr, [frame], [box], 10, k4, seed, resize=40)
    with pytest.raises(ValueError, match="positive"):
        build_inputs(fr, [0], [(0, 40, 0, 40)], 10, k4, seed, resize=0)


def test_entry_points_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "krrn_hip.h")).read()
    lib = _lib.lib()
    for name, nargs in [("krrn_crop_inputs_resize_u8", 15), ("krrn_choose_points_resize", 20)]:
        m = re.search(rf"^int {name}\((.*?)\);", src, re.M | re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs
        assert len(_lib.SIGNATURES[name]) == nargs and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs
