"""PoseDataset.zoom_batch: the crops cut again about a pose equal, bit for bit, what build_inputs(resize=T) makes of
the same windows given on the host and what tests/resize_ref.py's restatement makes of them; the keys it does not
replace are the first batch's own tensors; a crop whose pose is bad keeps its window; and batch() without zoom is what
it was."""
import numpy as np
import pytest
import torch

from pose_estimation_amd.dataset import ZOOM_KEYS, PoseDataset, build_inputs
from tests import resize_ref as R
from tests import zoom_ref as Z

pytestmark = pytest.mark.gpu

T, N = 80, 500
IDX = [0, 1, 2, 3, 4, 5]


def _ds():
    return PoseDataset("test", N, False, None, 0.0, 8, cls_type="all", num_frames=6, sizes=[80, 120, 160],
                       n_model_pts=128, resize=T)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


_CACHE = {}


def _zoomed(dev):
    """One zoom_batch with the ground-truth poses, except crop 2 whose pose lies behind the camera."""
    if not _CACHE:
        ds = _ds()
        data = ds.batch(IDX, dev, zoom=True)
        t = data["target_t"].clone()
        t[2, 2] = -t[2, 2]
        out = ds.zoom_batch(data, data["target_r"], t)
        torch.cuda.synchronize()
        _CACHE.update(ds=ds, data=data, out=out, t=t, sid=ds._draw_for(dev)[1])  # _calls stands where zoom_batch left it
    return _CACHE


def test_zoom_keys_of_the_first_batch(dev):
    c = _zoomed(dev)
    ds, data = c["ds"], c["data"]
    boxes = [ds.boxes[i] for i in IDX]
    assert _np(data["zoom_rc"]).tolist() == [[b[0], b[2]] for b in boxes] and data["zoom_rc"].dtype == torch.int32
    assert _np(data["zoom_side"]).tolist() == [b[1] - b[0] for b in boxes] and data["zoom_side"].dtype == torch.int32
    assert _np(data["zoom_frame"]).tolist() == IDX and data["zoom_frame"].dtype == torch.int32
    fr = ds.frames(dev)
    assert data["zoom_rgb"] is fr["rgb"] and data["zoom_depth"] is fr["depth"] and data["zoom_mask"] is fr["mask_label"]
    assert float(data["zoom_depth_scale"]) == 1.0 and "zoom_status" not in data


def test_windows_are_the_restatement_s_and_a_bad_pose_keeps_its_window(dev):
    c = _zoomed(dev)
    ds, data, out = c["ds"], c["data"], c["out"]
    ref = Z.windows(_np(data["model_points"]), _np(data["target_r"]).astype(np.float64).reshape(-1, 9),
                    _np(c["t"]).astype(np.float64), _np(data["intrinsic"]), 480, 640, T, 1.2, 40, _np(data["zoom_rc"]),
                    _np(data["zoom_side"]))
    assert ref["status"].tolist() == [0, 0, 1, 0, 0, 0]
    assert np.array_equal(_np(out["zoom_status"]), ref["status"]) and out["zoom_status"].dtype == torch.int32
    assert np.array_equal(_np(out["zoom_rc"]), ref["rc"]) and np.array_equal(_np(out["zoom_side"]), ref["side"])
    for k, r in (("bbox", "bbox"), ("resize_scale", "scale"), ("resize_intrinsic", "intr")):
        assert np.array_equal(_bits(_np(out[k])), _bits(ref[r])), k
    # the bad-pose row keeps its first window, the others moved
    assert _np(out["zoom_rc"])[2].tolist() == _np(data["zoom_rc"])[2].tolist()
    assert int(out["zoom_side"][2]) == int(data["zoom_side"][2])
    assert np.array_equal(_np(out["bbox"])[2], _np(data["bbox"])[2])
    moved = (_np(out["zoom_rc"]) != _np(data["zoom_rc"])).any(1) | (_np(out["zoom_side"]) != _np(data["zoom_side"]))
    assert moved.tolist() == [True, True, False, True, True, True]


def test_replaced_keys_equal_build_inputs_on_the_same_windows(dev):
    """build_inputs(resize=T) with the boxes read back from zoom_rc / zoom_side, the same seed and stream id."""
    c = _zoomed(dev)
    ds, data, out = c["ds"], c["data"], c["out"]
    rc, sd = _np(out["zoom_rc"]), _np(out["zoom_side"])
    boxes = [(int(r0), int(r0 + s), int(c0), int(c0 + s)) for (r0, c0), s in zip(rc, sd)]
    seed, sid = ds._seed_for(dev), c["sid"]
    assert sid == 2
    want = build_inputs(ds.frames(dev), IDX, boxes, N, data["intrinsic"],
                        seed, stream_id=sid, resize=T)
    want["bbox"] = torch.tensor([list(map(float, b)) for b in boxes])
    torch.cuda.synchronize()
    for k in ZOOM_KEYS:
        if k in ("zoom_rc", "zoom_side", "zoom_status"):
            continue
        a, b = _np(out[k]), _np(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), k
    assert set(ZOOM_KEYS) - {"zoom_status"} <= set(data) and set(out) == set(data) | {"zoom_status"}


def test_replaced_keys_equal_the_resize_restatement(dev):
    c = _zoomed(dev)
    ds, data, out = c["ds"], c["data"], c["out"]
    rc, sd = _np(out["zoom_rc"]), _np(out["zoom_side"])
    fr = ds.frames_np
    seed = int(ds._seed_for(dev).item())
    k4 = _np(data["intrinsic"])
    for b, f in enumerate(IDX):
        r = R.crop(fr["rgb"][f], fr["depth"][f], fr["mask_label"][f], int(rc[b, 0]), int(rc[b, 1]), int(sd[b]), T, N,
                   k4[b], 1.0, seed=seed, stream_id=2, index=b)
        assert r["count"] > 0 and int(out["mask_count"][b]) == r["count"], b
        assert np.array_equal(_bits(_np(out["img_croped"][b])), _bits(r["img"])), b
        assert np.array_equal(_np(out["point_mask"][b]).reshape(-1), r["mask"]), b
        assert np.array_equal(_np(out["choose"][b]).reshape(-1), r["choose"]), b
        assert np.array_equal(_bits(_np(out["cloud"][b])), _bits(r["cloud"])), b
        assert np.array_equal(_np(out["x_map_choosed"][b]).reshape(-1), r["xmap"]), b
        assert np.array_equal(_np(out["y_map_choosed"][b]).reshape(-1), r["ymap"]), b


def test_untouched_keys_are_the_same_tensors(dev):
    c = _zoomed(dev)
    data, out = c["data"], c["out"]
    for k in data:
        if k in ZOOM_KEYS:
            assert out[k] is not data[k], k
        else:
            assert out[k] is data[k], k
    # a second zoom of the zoomed batch works on the windows in use
    again = c["ds"].zoom_batch(out, data["target_r"], data["target_t"])
    torch.cuda.synchronize()
    assert _np(again["zoom_status"]).tolist() == [0] * 6
    assert np.array_equal(_np(again["zoom_rc"])[[0, 1, 3, 4, 5]], _np(out["zoom_rc"])[[0, 1, 3, 4, 5]])


def test_batch_without_zoom_is_unchanged(dev):
    """Against a second dataset built with the same seed: batch() returns the same keys and values with and without
    zoom=True apart from the zoom_* keys, and the resize keys are still the host function's."""
    a, b = _ds().batch(IDX, dev), _ds().batch(IDX, dev, zoom=True)
    torch.cuda.synchronize()
    assert list(a) == [k for k in b if not k.startswith("zoom_")]
    assert sorted(set(b) - set(a)) == ["zoom_depth", "zoom_depth_scale", "zoom_frame", "zoom_mask", "zoom_rc", "zoom_rgb",
                                       "zoom_side"]
    for k in a:
        x, y = _np(a[k]), _np(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), k
    assert list(a) == ["img_croped", "choose", "cloud", "x_map_choosed", "y_map_choosed", "point_mask", "mask_count",
                       "resize_scale", "resize_intrinsic", "cls_id", "intrinsic", "extent", "lfborder", "bbox", "target_r",
                       "target_t", "model_points", "target"]
    with pytest.raises(ValueError, match="zoom needs a dataset built with resize"):
        PoseDataset("test", N, False, None, 0.0, 8, num_frames=2, sizes=[80], n_model_pts=32).batch([0, 1], dev, zoom=True)
