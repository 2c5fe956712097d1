"""The zoom-in pass on the host: the window rule's numpy restatement (tests/zoom_ref.py) against the rule's own
properties and against dataset.resize_intrinsic, the refusals of test_epoch(zoom=) and batch(zoom=True), and the new
entry points' presence. No GPU: nothing here launches a kernel."""
import os
import re

import numpy as np
import pytest
import torch

from pose_estimation_amd import _lib, evaluate, zoom
from pose_estimation_amd.dataset import (PoseDataset, build_inputs_windows, get_square_bbox, resize_intrinsic,
                                         synthetic_frames)
from pose_estimation_amd.synthetic import LM_K
from tests import zoom_ref as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4 = np.array([LM_K[0, 0], LM_K[1, 1], LM_K[0, 2], LM_K[1, 2]], np.float32)
H, W, T = 480, 640, 80
_FR = {}


def _frames():
    if not _FR:
        fr = synthetic_frames(64, n_model_pts=256)
        boxes = [get_square_bbox([float(v) for v in bb]) for bb in fr["bbox"]]
        _FR.update(fr=fr, boxes=boxes, rc=np.array([[b[0], b[2]] for b in boxes], np.int32),
                   side=np.array([b[1] - b[0] for b in boxes], np.int32))
    return _FR


def _windows(R, t, pad=zoom.ZOOM_PAD, ms=zoom.ZOOM_MIN_SIDE):
    f = _frames()
    n = len(R)
    return Z.windows(f["fr"]["model_points"][:n], R.reshape(n, 9), t, np.tile(K4, (n, 1)), H, W, T, pad, ms, f["rc"][:n],
                     f["side"][:n])


def _check_properties(out, ms):
    """Inside the frame, the side within its bounds, and wherever nothing was clamped the window holds the points'
    box: c0 = floor(centre - S / 2 + 1) <= centre - S / 2 + 1 and S >= pad * extent, so c0 <= umin as soon as
    (pad - 1) / 2 * extent >= 1, i.e. extent >= 10 pixels at pad 1.2, which an unclamped side >= min_side = 40
    implies along the larger extent (the smaller one has more room); the right edge c0 + S - 1 > centre + S / 2 - 1
    alike."""
    for r in out["rows"]:
        if r["status"] != 0:
            continue
        (r0, c0), S = r["rc"], r["side"]
        assert ms <= S <= min(H, W)
        assert 0 <= r0 and r0 + S <= H and 0 <= c0 and c0 + S <= W
        if not r["clamped"]:
            umin, umax, vmin, vmax = r["box"]
            assert c0 <= umin and umax <= c0 + S - 1 and r0 <= vmin and vmax <= r0 + S - 1, r


def test_ground_truth_poses_on_the_synthetic_frames():
    """The default pad and min_side on synthetic_frames(64)'s own poses: every crop gets a new window inside the
    frame."""
    f = _frames()
    out = _windows(f["fr"]["target_r"].astype(np.float64), f["fr"]["target_t"].astype(np.float64))
    assert (out["status"] == 0).all()
    _check_properties(out, zoom.ZOOM_MIN_SIDE)
    assert len(set(f["side"].tolist())) >= 3 and f["side"].min() >= 80
    assert 40 < out["side"].min() and out["side"].max() < 480
    assert any(not r["clamped"] for r in out["rows"])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_poses_keep_the_rule_s_properties(seed):
    """The ground-truth poses perturbed: rotated by up to ~30 degrees, moved by up to 40 cm sideways and 50 % in
    depth, so that projections leave the frame, cross its edges, outgrow it and shrink below min_side."""
    f = _frames()
    rng = np.random.default_rng(seed)
    n = 64
    R = f["fr"]["target_r"].astype(np.float64).copy()
    t = f["fr"]["target_t"].astype(np.float64).copy()
    for b in range(n):
        w = rng.normal(0, 0.3, 3)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R[b] = (np.eye(3) + Kx + Kx @ Kx / 2) @ R[b]  # near a rotation: the rule does not need an exact one
    t[:, :2] += rng.uniform(-0.4, 0.4, (n, 2))
    t[:, 2] *= rng.uniform(0.15, 6.0, n)
    t[::16, 2] = -t[::16, 2]  # behind the camera
    out = _windows(R, t)
    st = out["status"]
    assert (st == 0).any() and (st == 1).any() and (st == 2).any()
    _check_properties(out, zoom.ZOOM_MIN_SIDE)
    sides = out["side"][st == 0]
    assert sides.min() == zoom.ZOOM_MIN_SIDE or sides.max() == min(H, W) or any(r["clamped"] for r in out["rows"])
    keep = st != 0
    assert np.array_equal(out["rc"][keep], f["rc"][:n][keep]) and np.array_equal(out["side"][keep], f["side"][:n][keep])


def test_scale_and_intrinsic_are_resize_intrinsic_s():
    """Whatever the window, kept ones included: scale and intr equal dataset.resize_intrinsic of the same boxes, cast
    to f32, bit for bit; with per-crop K4 rows."""
    f = _frames()
    n = 64
    k4 = np.stack([K4 * np.float32(1 + 0.01 * b) + np.float32(b) for b in range(n)]).astype(np.float32)
    rng = np.random.default_rng(5)
    t = f["fr"]["target_t"].astype(np.float64) + rng.uniform(-0.3, 0.3, (n, 3))
    out = Z.windows(f["fr"]["model_points"], f["fr"]["target_r"].astype(np.float64).reshape(n, 9), t, k4, H, W, T,
                    zoom.ZOOM_PAD, zoom.ZOOM_MIN_SIDE, f["rc"], f["side"])
    boxes = [(int(b[0]), int(b[1]), int(b[2]), int(b[3])) for b in out["bbox"]]
    assert all(b[1] - b[0] == s and b[3] - b[2] == s for b, s in zip(boxes, out["side"]))
    s, intr = resize_intrinsic(torch.from_numpy(k4), boxes, T)
    assert np.array_equal(out["scale"].view(np.uint32), s.astype(np.float32).view(np.uint32))
    assert np.array_equal(out["intr"].view(np.uint32), intr.astype(np.float32).view(np.uint32))
    assert len({b[1] - b[0] for b in boxes}) > 5


def test_garbage_poses_never_overflow_the_int_conversion():
    """A point a hair in front of the camera projects ~1e300 pixels away: the side and the shifts are clamped in f64,
    so the window is the whole short side, inside the frame."""
    pts = np.array([[[-1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0]]], np.float32)
    out = Z.windows(pts, np.eye(3).reshape(1, 9), np.array([[0.0, 0.0, 1e-300]]), K4[None], H, W, T, 1.2, 40,
                    np.array([[1, 2]], np.int32), np.array([50], np.int32))
    assert out["status"][0] == 0 and out["side"][0] == min(H, W) and tuple(out["rc"][0]) == (0, 0)
    out = Z.windows(pts, np.eye(3).reshape(1, 9), np.array([[1e300, 0.0, 1e-300]]), K4[None], H, W, T, 1.2, 40,
                    np.array([[1, 2]], np.int32), np.array([50], np.int32))
    assert out["status"][0] == 1 and tuple(out["rc"][0]) == (1, 2) and out["side"][0] == 50  # u overflows to inf


def test_refusals():
    plain = PoseDataset(num_frames=2, sizes=[80], n_model_pts=32)
    sized = PoseDataset(num_frames=2, sizes=[80], n_model_pts=32, resize=80)
    for bad in (-1, 1.0, 0.5, "1", None, True):
        with pytest.raises(ValueError, match="integer >= 0"):
            evaluate.test_epoch(None, sized, device="cpu", zoom=bad)
        with pytest.raises(ValueError, match="integer >= 0"):
            evaluate.eval_records(None, sized, {80: [0, 1]}, 2, "cpu", zoom=bad)
    with pytest.raises(ValueError, match="zoom needs a dataset built with resize"):
        evaluate.test_epoch(None, plain, device="cpu", zoom=1)
    with pytest.raises(ValueError, match="zoom needs a dataset built with resize"):
        evaluate.eval_records(None, plain, {80: [0, 1]}, 2, "cpu", zoom=2)
    with pytest.raises(ValueError, match="zoom needs a dataset built with resize"):
        plain.batch([0, 1], "cpu", zoom=True)
    with pytest.raises(ValueError, match="zoom needs a dataset built with resize"):
        plain.zoom_batch({}, None, None)
    with pytest.raises(ValueError, match="one rank"):
        evaluate.test_epoch(None, sized, device="cpu", zoom=1, world=2, rank=0)
    with pytest.raises(ValueError, match="zoom with net_masks"):
        evaluate.eval_records(None, sized, {80: [0, 1]}, 2, "cpu", zoom=1, net_masks=True)
    with pytest.raises(ValueError, match="zoom=True"):
        sized.zoom_batch({"img_croped": None}, None, None)


def test_entry_points_take_gpu_tensors_only():
    fr = {"rgb": torch.zeros((1, 48, 64, 3), dtype=torch.uint8), "depth": torch.zeros((1, 48, 64)),
          "mask_label": torch.zeros((1, 48, 64), dtype=torch.uint8)}
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    with pytest.raises(RuntimeError, match="HIP path only"):
        build_inputs_windows(fr, i32([0]), i32([[0, 0]]), i32([40]), 10, torch.from_numpy(K4[None]),
                             torch.zeros(1, dtype=torch.int64), 0, 1.0, None, 40)
    with pytest.raises(RuntimeError, match="HIP path only"):
        zoom.pose_windows(torch.zeros((1, 5, 3)), torch.eye(3)[None], torch.zeros((1, 3)), torch.from_numpy(K4[None]),
                          (48, 64), i32([[0, 0]]), i32([40]), 40)
    assert zoom.ZOOM_PAD == 1.2 and zoom.ZOOM_MIN_SIDE == 40


def test_entry_point_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "krrn_hip.h")).read()
    m = re.search(r"^int krrn_pose_windows_f64\((.*?)\);", src, re.M | re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 20
    assert len(_lib.SIGNATURES["krrn_pose_windows_f64"]) == 20
    assert len(_lib.lib().krrn_pose_windows_f64.argtypes) == 20
    mk = open(os.path.join(ROOT, "pose_estimation_amd", "csrc", "Makefile")).read()
    assert re.search(r"^FLAGS_pose_window := -ffp-contract=off$", mk, re.M)
