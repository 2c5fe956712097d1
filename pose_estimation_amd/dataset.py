"""LineMOD-style eval loader with the per-sample work on the GPU (SURVEY.md §8b loader API,
§8f rows f2 and f3).

The reference's PoseDataset (dataset/linemod/batchdataset.py:34) reads one frame per item and
builds the crop in numpy (`_load_data`, :603-771): square-box snap, crop, ImageNet
normalisation, mask, random `choose`, back-projected cloud. Here the box snap stays on the host
(scalar integer logic, `get_square_bbox` below restates :890-961) and the per-pixel work runs for
a whole bucket of equal-size crops at once in two HIP launches (krrn_crop_inputs_u8,
krrn_choose_points). The frames live on the GPU. `resize=T` (the reference's Data.RESIZE path, _load_resize_data
:339-601, by this project's own definition) resamples every crop to T x T instead, in the same two
steps (krrn_crop_inputs_resize_u8, krrn_choose_points_resize), so crops of any side share one batch.

`root` = a LineMOD tree in the reference's layout (Linemod_preprocessed): per object
`data/XX/{test,train}.txt` (image ids), `data/XX/gt.yml` (cam_R_m2c, cam_t_m2c in mm, obj_bb;
for benchvise the entry with obj_id 2, batchdataset.py:152-153, 229-240), `data/XX/rgb/NNNN.png`,
`data/XX/depth/NNNN.png` (uint16 mm), `data/XX/mask/NNNN.png` (mask_label = channel 0 == 255;
mode 'eval': `segnet_results/XX_label/NNNN_label.png` == 255, :197-244), and
`models/obj_XX.ply` (ascii PLY vertices / 1000, ply_vtx :841-852; 2600 random model points at
test time, :700-704). Only the crop sizes (from gt.yml's boxes) are read up front; each batch
reads and decodes its frames (a thread pool) and stages them to the GPU. Not read: the per-frame
GT-map pickles (xyz / normal / region, :202-212) and fps_64.pkl (:105), which come from an offline
renderer that neither the reference's tree nor a stock Linemod_preprocessed holds. They feed the
logged loss terms and the `mask_obj` factor of the point mask. By default the mask is therefore
mask_label * mask_depth (documented deviation) and the loss keys are absent; with `gt_maps=True` the
maps are rendered on the GPU from the PLY's faces, the GT pose and K (raster.py), the mask is the
reference's label * obj * depth, and every batch carries xyz, normal, region, mask, multi_cls_mask,
mask_obj, region_point, coordinate_choosed and depth_render. `meshes=True` only loads the meshes
(faces, all vertices, symmetry sets) for the BOP pose errors (bop.py): `batch(idx, device, bop=True)`, and for
pose verification (verify.py, pose.select_pose): `batch(idx, device, verify=True)`.

`layout="bop"` reads `root` as a tree in BOP's own layout instead (bop_scene.py: several instances per image, a
camera matrix and a depth scale per image, models_info.json; LM-O and its kin) and feeds the same kernels:
see PoseDataset.

`root=None` (the default; no LineMOD data ships with the reference and there is no network)
serves seeded synthetic 640x480 RGB-D frames built like the real ones (an object mask inside a
YOLO-like detection box whose snapped sizes follow the LineMOD test histogram, a depth plane
with an object bump, LineMOD intrinsics and models_info extents, a GT pose and model points).

    ds = PoseDataset("test", 1000, False, None, 0.0, 8, cls_type="all")
    ds = PoseDataset("test", 1000, False, "/data/Linemod_preprocessed", 0.0, 8, cls_type="cat")
    for S, idx in BucketBatcher(ds, bs=64):      # f3: equal-S batches (trainer.py:521-551)
        data = ds.batch(idx, device)             # the eval keys of :730-771, on the GPU
"""
from __future__ import annotations

import os
import random
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import bop as _bop
from . import rle as _rle
from .bop import symmetry_set
from .bop_scene import BopTree
from .config import CONFIG, LM_OBJLIST, OBJ_DICT, SYM_OBJ, models_info
from .models import FPS_MAX, sample_surface
from .raster import N_REGIONS, finish_maps, region_points, render_maps
from .runtime import h2d, ptr, stream_ptr
from .synthetic import LM_K, rand_rotation
from .zoom import pose_windows

# batchdataset.py:823
BORDER_LIST = [-1] + list(range(40, 640, 40)) + [640]
# measured LineMOD test crop sizes (get_square_bbox over bbox_yolov3_all.json)
LM_CROP_HIST = {40: 3, 80: 3025, 120: 4889, 160: 3659, 200: 1402, 240: 403, 280: 41, 320: 3}
# krrn_choose_points takes stream ids 0 .. 65534 (include/krrn_hip.h)
CHOOSE_STREAMS = 65535
# the keys PoseDataset.zoom_batch replaces (it adds zoom_status); every other key is the first batch's own tensor
ZOOM_KEYS = ("img_croped", "choose", "cloud", "x_map_choosed", "y_map_choosed", "point_mask", "mask_count", "bbox",
             "resize_scale", "resize_intrinsic", "zoom_rc", "zoom_side", "zoom_status")


def get_square_bbox(bbox, height_px: int = 480, width_px: int = 640) -> Tuple[int, int, int, int]:
    """batchdataset.py:890-961: [x, y, w, h] -> (rmin, rmax, cmin, cmax), a square whose side is
    snapped up to the 40-px border grid and shifted inside the frame."""
    bbx = [bbox[1], bbox[1] + bbox[3], bbox[0], bbox[0] + bbox[2]]
    if bbx[0] < 0:
        bbx[0] = 0
    if bbx[1] >= height_px:
        bbx[1] = height_px - 1
    if bbx[2] < 0:
        bbx[2] = 0
    if bbx[3] >= width_px:
        bbx[3] = width_px - 1
    rmin, rmax, cmin, cmax = bbx
    rmax += 1
    cmax += 1
    r_b = rmax - rmin
    c_b = cmax - cmin
    if r_b <= c_b:
        r_b = c_b
    else:
        c_b = r_b
    for tt in range(len(BORDER_LIST) - 1):
        if BORDER_LIST[tt] < r_b < BORDER_LIST[tt + 1]:
            r_b = BORDER_LIST[tt + 1]
            break
    for tt in range(len(BORDER_LIST) - 1):
        if BORDER_LIST[tt] < c_b < BORDER_LIST[tt + 1]:
            c_b = BORDER_LIST[tt + 1]
            break
    center = [int((rmin + rmax) / 2), int((cmin + cmax) / 2)]
    rmin = center[0] - int(r_b / 2)
    rmax = center[0] + int(r_b / 2)
    cmin = center[1] - int(c_b / 2)
    cmax = center[1] + int(c_b / 2)
    if rmin < 0:
        delt = -rmin
        rmin = 0
        rmax += delt
    if cmin < 0:
        delt = -cmin
        cmin = 0
        cmax += delt
    if rmax > height_px:
        delt = rmax - height_px
        rmax = height_px
        rmin -= delt
        if rmin < 0:
            rmax = rmax - rmin
            rmin = 0
            if rmax >= height_px:
                rmax = height_px - 1
    if cmax > width_px:
        delt = cmax - width_px
        cmax = width_px
        cmin -= delt
        if cmin < 0:
            cmax = cmax - cmin
            cmin = 0
            if cmax >= width_px:
                cmax = width_px - 1
    m = (rmax - rmin) - (cmax - cmin)
    if m > 0:
        rmax = rmax - np.floor(m / 2)
        rmin = rmin + np.floor(m / 2)
    elif m < 0:
        cmax = cmax + np.floor(m / 2)
        cmin = cmin - np.floor(m / 2)
    return int(rmin), int(rmax), int(cmin), int(cmax)


def synthetic_frames(F: int, seed: int = 0, objlist: Sequence[int] = (6,), H: int = 480, W: int = 640,
                     n_model_pts: int = 2600, sizes: Optional[Sequence[int]] = None) -> Dict[str, np.ndarray]:
    """Seeded full RGB-D frames with one object each (see module doc). Crop sizes are drawn from
    LM_CROP_HIST unless `sizes` fixes them (one per frame, cycled)."""
    rng = np.random.default_rng(seed)
    info = models_info()
    fx, fy, cx, cy = LM_K[0, 0], LM_K[1, 1], LM_K[0, 2], LM_K[1, 2]
    hs = np.array(list(LM_CROP_HIST.keys()))
    hp = np.array(list(LM_CROP_HIST.values()), dtype=np.float64)
    hp /= hp.sum()
    out = {k: [] for k in ("rgb", "depth", "mask_label", "bbox", "obj_id", "target_r", "target_t", "model_points")}
    yy, xx = np.mgrid[0:H, 0:W]
    for f in range(F):
        oid = objlist[f % len(objlist)]
        S = int(sizes[f % len(sizes)]) if sizes is not None else int(rng.choice(hs, p=hp))
        # a detection box whose snapped square is S (w, h in (S - 39, S - 1])
        w = S - 1 - rng.uniform(0.0, 30.0)
        h = S - 1 - rng.uniform(0.0, 30.0)
        x = rng.uniform(0, W - w - 1)
        y = rng.uniform(0, H - h - 1)
        ccy, ccx = y + h / 2, x + w / 2
        a, c = 0.45 * h, 0.45 * w
        m = (((yy - ccy) / a) ** 2 + ((xx - ccx) / c) ** 2) <= 1.0
        z0 = rng.uniform(0.7, 1.1)
        bump = 0.05 * np.sqrt(np.clip(1.0 - ((yy - ccy) / a) ** 2 - ((xx - ccx) / c) ** 2, 0, None))
        depth = (z0 - bump * m).astype(np.float32)
        depth[rng.random((H, W)) < 0.02] = 0.0  # sensor holes (mask_depth, :663)
        mi = info[oid]
        lf = np.array(mi["min"]) / 1000.0
        ext = np.array(mi["size"]) / 1000.0
        R = rand_rotation(rng)
        t = np.array([(ccx - cx) * z0 / fx, (ccy - cy) * z0 / fy, z0])
        out["rgb"].append(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
        out["depth"].append(depth)
        out["mask_label"].append((m * 255).astype(np.uint8))
        out["bbox"].append(np.array([x, y, w, h], np.float32))
        out["obj_id"].append(oid)
        out["target_r"].append(R.astype(np.float32))
        out["target_t"].append(t.astype(np.float32))
        out["model_points"].append((lf + rng.random((n_model_pts, 3)) * ext).astype(np.float32))
    return {k: np.stack(v) for k, v in out.items()}


def _stage_windows(frame_idx: Sequence[int], boxes: Sequence[Tuple[int, int, int, int]], dev):
    """(fi int32 [B], rc int32 [B, 2] = (r0, c0), side int32 [B]) of the boxes' windows, on `dev`: what the input
    kernels read. One upload; the three are contiguous views of it."""
    fi, B = list(frame_idx), len(boxes)
    rc = [v for b in boxes for v in (b[0], b[2])]
    w = h2d(torch.tensor(fi + rc + [b[1] - b[0] for b in boxes], dtype=torch.int32), dev)
    return w[:len(fi)], w[len(fi):len(fi) + 2 * B].view(B, 2), w[len(fi) + 2 * B:]


def _launch_inputs(frames, fi, rc, side, out_side: int, num_point: int, K4, seed, stream_id, depth_scale,
                   obj_mask) -> Dict[str, torch.Tensor]:
    """The two launches of the input path for windows staged on the device (fi, rc, side: _stage_windows), at output
    side `out_side`. side=None: every window's side is out_side (krrn_crop_inputs_u8, krrn_choose_points); else the
    kernels read side[b] (krrn_crop_inputs_resize_u8, krrn_choose_points_resize)."""
    rgb, depth, ml = frames["rgb"], frames["depth"], frames["mask_label"]
    dev = rgb.device
    F, H, W = depth.shape
    B, T, N = int(fi.shape[0]), out_side, num_point
    crop, pick, sd = (("krrn_crop_inputs_u8", "krrn_choose_points", ()) if side is None else
                      ("krrn_crop_inputs_resize_u8", "krrn_choose_points_resize", (ptr(side),)))
    img = torch.empty((B, 3, T, T), dtype=torch.float32, device=dev)
    mask = torch.empty((B, T * T), dtype=torch.uint8, device=dev)
    st = stream_ptr(dev)
    _lib.call(crop, ptr(rgb), ptr(depth), ptr(ml), ptr(obj_mask), F, H, W, ptr(fi), ptr(rc), *sd, B, T, ptr(img),
              ptr(mask), st)
    choose = torch.empty((B, 1, N), dtype=torch.int64, device=dev)
    cloud = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    xm = torch.empty((B, N, 1), dtype=torch.float32, device=dev)
    ym = torch.empty((B, N, 1), dtype=torch.float32, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    K4 = h2d(K4, dev, torch.float32)
    _lib.call(pick, ptr(mask), B, T, N, ptr(depth), H, W, ptr(fi), ptr(rc), *sd, ptr(K4), float(depth_scale),
              ptr(seed), int(stream_id), ptr(choose), ptr(cloud), ptr(xm), ptr(ym), ptr(cnt), st)
    return {"img_croped": img, "choose": choose, "cloud": cloud, "x_map_choosed": xm, "y_map_choosed": ym,
            "point_mask": mask.view(B, 1, T, T), "mask_count": cnt}


def build_inputs(frames: Dict[str, torch.Tensor], frame_idx: Sequence[int], boxes: Sequence[Tuple[int, int, int, int]],
                 num_point: int, K4: torch.Tensor, seed: torch.Tensor, stream_id: int = 0,
                 depth_scale: float = 1.0, obj_mask: Optional[torch.Tensor] = None,
                 resize: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The per-pixel half of _load_data for crops of one size on the GPU: img_croped, choose,
    cloud, x/y_map_choosed, plus the point mask and its pixel count per crop.
    resize=T (default None: the above, unchanged) takes boxes of mixed sides and resamples every crop to T x T
    (krrn_crop_inputs_resize_u8, krrn_choose_points_resize): the same keys at side T, x/y_map_choosed
    the resized pixels' centres in full-frame coordinates, plus resize_scale f32 [B] = S_b / T and resize_intrinsic
    f32 [B, 4] = (fx / s, fy / s, (cx - c0 + 0.5) / s - 0.5, (cy - r0 + 0.5) / s - 0.5), the pinhole under which the
    crop's resized pixel indices project (the reference's key; nothing here reads it)."""
    if resize is not None:
        return _build_inputs_resize(frames, frame_idx, boxes, num_point, K4, seed, stream_id, depth_scale, obj_mask,
                                    int(resize))[0]
    sizes = {rmax - rmin for rmin, rmax, _, _ in boxes} | {cmax - cmin for _, _, cmin, cmax in boxes}
    if len(sizes) != 1:
        raise ValueError(f"one crop size per batch (bucket by get_square_bbox first), got {sorted(sizes)}")
    fi, rc, _ = _stage_windows(frame_idx, boxes, frames["rgb"].device)
    return _launch_inputs(frames, fi, rc, None, sizes.pop(), num_point, K4, seed, stream_id, depth_scale, obj_mask)


def _build_inputs_resize(frames, frame_idx, boxes, num_point, K4, seed, stream_id, depth_scale, obj_mask, T: int):
    """build_inputs(resize=T): the device reads each crop's side, so the windows are checked here, from the boxes.
    Returns (build_inputs' dict, the staged windows (fi, rc, side)); the latter is for PoseDataset.batch(zoom=True)."""
    dev = frames["rgb"].device
    F, H, W = frames["depth"].shape
    B = len(frame_idx)
    if T < 1:
        raise ValueError(f"resize must be a positive size, got {T}")
    if len(boxes) != B or tuple(K4.shape) != (B, 4):
        raise ValueError(f"one box and one K4 row per crop: {B} crops, {len(boxes)} boxes, K4 {tuple(K4.shape)}")
    for f, (rmin, rmax, cmin, cmax) in zip(frame_idx, boxes):
        S = rmax - rmin
        if cmax - cmin != S or not 1 <= S <= min(H, W):
            raise ValueError(f"a resized crop's window is a square of side 1..{min(H, W)}, got box "
                             f"{(rmin, rmax, cmin, cmax)}")
        if rmin < 0 or cmin < 0 or rmax > H or cmax > W or not 0 <= int(f) < F:
            raise ValueError(f"box {(rmin, rmax, cmin, cmax)} of frame {f} lies outside the {F} frames of {H} x {W}")
    win = _stage_windows(frame_idx, boxes, dev)
    scale, intr = resize_intrinsic(K4, boxes, T)
    out = build_inputs_windows(frames, *win, num_point, K4, seed, stream_id, depth_scale, obj_mask, T)
    out["resize_scale"] = h2d(torch.from_numpy(scale.astype(np.float32)), dev)
    out["resize_intrinsic"] = h2d(torch.from_numpy(intr.astype(np.float32)), dev)
    return out, win


def build_inputs_windows(frames: Dict[str, torch.Tensor], fi: torch.Tensor, rc: torch.Tensor, side: torch.Tensor,
                         num_point: int, K4: torch.Tensor, seed: torch.Tensor, stream_id: int, depth_scale: float,
                         obj_mask: Optional[torch.Tensor], T: int) -> Dict[str, torch.Tensor]:
    """The two launches of the resized input path (krrn_crop_inputs_resize_u8, krrn_choose_points_resize) for windows
    that live on the device: fi int32 [B] each crop's frame, rc int32 [B, 2] = (r0, c0) and side int32 [B], GPU tensors
    that the kernels read themselves, so windows computed on the GPU (zoom.pose_windows) feed them without a
    read-back. No host-side window check: the kernels treat a window the frame does not hold as an empty crop (zeros,
    an empty mask, count 0). Returns build_inputs(resize=T)'s keys at side T except resize_scale / resize_intrinsic,
    which belong to whoever made the windows."""
    rgb, depth, ml = frames["rgb"], frames["depth"], frames["mask_label"]
    if not (rgb.is_cuda and depth.is_cuda and ml.is_cuda and fi.is_cuda and rc.is_cuda and side.is_cuda
            and seed.is_cuda and (obj_mask is None or obj_mask.is_cuda)):
        raise RuntimeError("build_inputs_windows runs on the HIP path only (the frames, fi / rc / side and the seed "
                           "must be GPU tensors)")
    B = int(fi.shape[0])
    T = int(T)
    if T < 1:
        raise ValueError(f"resize must be a positive size, got {T}")
    if tuple(rc.shape) != (B, 2) or tuple(side.shape) != (B,) or tuple(K4.shape) != (B, 4):
        raise ValueError(f"one window and one K4 row per crop: {B} crops, rc {tuple(rc.shape)}, side "
                         f"{tuple(side.shape)}, K4 {tuple(K4.shape)}")
    fi, rc, side = (h2d(x, rgb.device, torch.int32) for x in (fi, rc, side))
    return _launch_inputs(frames, fi, rc, side, T, num_point, K4, seed, stream_id, depth_scale, obj_mask)


def resize_intrinsic(K4, boxes: Sequence[Tuple[int, int, int, int]], T: int) -> Tuple[np.ndarray, np.ndarray]:
    """(resize_scale [B], resize_intrinsic [B, 4]) of windows `boxes` resampled to side T, in f64 on the host:
    s = S_b / T, and resized pixel index u' = (u - c0 + 0.5) / s - 0.5 of frame pixel u, so fx' = fx / s,
    cx' = (cx - c0 + 0.5) / s - 0.5 (rows alike)."""
    k = torch.as_tensor(K4).detach().cpu().double().numpy().reshape(-1, 4)
    s = np.array([(b[1] - b[0]) / float(T) for b in boxes], np.float64)
    r0 = np.array([b[0] for b in boxes], np.float64)
    c0 = np.array([b[2] for b in boxes], np.float64)
    intr = np.stack([k[:, 0] / s, k[:, 1] / s, (k[:, 2] - c0 + 0.5) / s - 0.5, (k[:, 3] - r0 + 0.5) / s - 0.5], 1)
    return s, intr


def ply_vtx(path: str) -> np.ndarray:
    """Vertices of an ascii PLY (batchdataset.py:841-852: the element count on the 4th line, x y z
    the first three fields of each vertex line), f32 [n, 3] in the file's units."""
    with open(path) as f:
        if f.readline().strip() != "ply":
            raise ValueError(f"{path}: not a PLY file")
        n = None
        fmt = None
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            tok = line.split()
            if tok[:1] == ["format"]:
                fmt = tok[1]
            if tok[:2] == ["element", "vertex"]:
                n = int(tok[2])
            if line.strip() == "end_header":
                break
        if fmt != "ascii" or n is None:
            raise ValueError(f"{path}: only ascii PLY vertex lists are read (format {fmt})")
        return np.array([np.float32(f.readline().split()[:3]) for _ in range(n)], dtype=np.float32)


def ply_faces(path: str) -> np.ndarray:
    """Triangles of an ascii PLY, int32 [n, 3]: the `element face` block's `3 i j k` lines (whatever
    follows the three indices on a line, e.g. per-face colours, is ignored). A PLY with `element face 0`
    gives [0, 3]; a face that is not a triangle raises."""
    with open(path) as f:
        if f.readline().strip() != "ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elems = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            tok = line.split()
            if tok[:1] == ["format"]:
                fmt = tok[1]
            if tok[:1] == ["element"]:
                elems.append((tok[1], int(tok[2])))
            if line.strip() == "end_header":
                break
        if fmt != "ascii":
            raise ValueError(f"{path}: only ascii PLY is read (format {fmt})")
        for name, n in elems:  # the elements' lines follow the header in the order declared
            if name != "face":
                for _ in range(n):
                    f.readline()
                continue
            out = np.zeros((n, 3), dtype=np.int32)
            for i in range(n):
                tok = f.readline().split()
                if len(tok) < 4 or int(tok[0]) != 3:
                    raise ValueError(f"{path}: face {i} is not a triangle ('{' '.join(tok)}')")
                out[i] = [int(tok[1]), int(tok[2]), int(tok[3])]
            return out
    return np.zeros((0, 3), dtype=np.int32)


def _read_lines(p: str) -> List[str]:
    with open(p) as f:
        return [ln.strip() for ln in f if ln.strip()]


class _LinemodTree:
    """Index of a LineMOD tree (module doc): one entry per (object, image id) of the split, its GT
    pose and detection box from gt.yml; frames are read on demand."""

    def __init__(self, root: str, mode: str, objlist: Sequence[int], n_model_pts: int, seed: int,
                 meshes: bool = False, model_points: str = "vertices"):
        import yaml
        self.root, self.mode = root, mode
        self.items: List[Dict[str, object]] = []
        self.model_points: Dict[int, np.ndarray] = {}
        # meshes: per object the full vertex set (metres) and the triangles, for GT-map rendering and the BOP
        # errors; apart from the n_model_pts subsample below, which ADD(-S) uses
        self.mesh: Dict[int, Tuple[np.ndarray, np.ndarray]] = {}
        # per object its symmetry transformations [NS, 12] (bop.symmetry_set), from the optional keys
        # symmetries_discrete / symmetries_continuous of the tree's models/models_info.yml (BOP's convention);
        # a stock Linemod_preprocessed tree has none: the identity only
        self.symmetries: Dict[int, np.ndarray] = {}
        tree_info = {}
        ipath = os.path.join(root, "models", "models_info.yml")
        if meshes and os.path.exists(ipath):
            with open(ipath) as f:
                tree_info = {int(k): v for k, v in (yaml.safe_load(f) or {}).items()}
        rng = np.random.default_rng(seed)
        split = "train.txt" if mode == "train" else "test.txt"
        for obj in objlist:
            croot = os.path.join(root, "data", f"{obj:02d}")
            with open(os.path.join(croot, "gt.yml")) as f:
                meta = yaml.safe_load(f)
            for im in _read_lines(os.path.join(croot, split)):
                entries = meta[int(im)]
                e = entries[0]
                if obj == 2:  # benchvise frames list several objects (batchdataset.py:230-234)
                    e = next((m for m in entries if int(m["obj_id"]) == 2), e)
                self.items.append({"obj": obj, "im": int(im), "R": np.resize(np.array(e["cam_R_m2c"], np.float64), (3, 3)),
                                   "t": np.array(e["cam_t_m2c"], np.float64) / 1000.0,
                                   "bbox": [float(v) for v in e["obj_bb"]]})
            pts = ply_vtx(os.path.join(root, "models", f"obj_{obj:02d}.ply")) / 1000.0
            if meshes:
                tri = ply_faces(os.path.join(root, "models", f"obj_{obj:02d}.ply"))
                if len(tri) == 0:
                    raise ValueError(f"gt_maps=True / meshes=True render from the mesh, but obj_{obj:02d}.ply has no "
                                     "faces (element face 0)")
                if tri.min() < 0 or tri.max() >= len(pts):
                    raise ValueError(f"obj_{obj:02d}.ply: a face index lies outside its {len(pts)} vertices")
                self.mesh[obj] = (pts.astype(np.float32), tri)
                oi = tree_info.get(obj, {})
                self.symmetries[obj] = symmetry_set(oi.get("symmetries_discrete"), oi.get("symmetries_continuous"))
            if model_points == "surface":  # PoseDataset samples them on the mesh before its first batch
                continue
            if len(pts) < n_model_pts:
                # the reference's random.sample(range(len(pts)), len(pts) - num_pt_mesh_large) raises here
                # too (batchdataset.py:700-704): every crop's ADD(-S) runs over exactly n_model_pts points
                raise ValueError(f"obj_{obj:02d}.ply has {len(pts)} vertices < num_pt_mesh_large = {n_model_pts}")
            if len(pts) > n_model_pts:  # random deletion down to num_pt_mesh_large (:700-704)
                keep = np.sort(rng.choice(len(pts), n_model_pts, replace=False))
                pts = pts[keep]
            self.model_points[obj] = pts.astype(np.float32)

    def read(self, i: int):
        it = self.items[i]
        croot = os.path.join(self.root, "data", f"{int(it['obj']):02d}")
        im = int(it["im"])
        from PIL import Image
        with Image.open(os.path.join(croot, "rgb", f"{im:04d}.png")) as ri:
            rgb = np.array(ri)[:, :, :3]
        with Image.open(os.path.join(croot, "depth", f"{im:04d}.png")) as di:
            # depth / cam_scale (f64) then float32, as _load_data's depth_choosed (:714-716)
            depth = (np.asarray(di).astype(np.float64) / 1000.0).astype(np.float32)
        if self.mode == "eval":
            lp = os.path.join(self.root, "segnet_results", f"{int(it['obj']):02d}_label", f"{im:04d}_label.png")
        else:
            lp = os.path.join(croot, "mask", f"{im:04d}.png")
        with Image.open(lp) as li:
            label = np.array(li)
        ml = (label[:, :, 0] if label.ndim == 3 else label) == 255
        return rgb, depth, ml.astype(np.uint8)


class PoseDataset(torch.utils.data.Dataset):
    """The reference's constructor signature (batchdataset.py:34); `root` = a LineMOD tree, or
    None for synthetic frames (module doc). Eval only: add_noise / noise_trans / num_kps are
    accepted and unused. gt_maps=True also serves the per-pixel ground truth, rendered from the tree's
    meshes (needs a tree whose PLYs have faces; ValueError otherwise); the default changes nothing.
    meshes=True loads the meshes (vertices, faces, symmetry sets) without rendering GT maps, which is what
    batch(..., bop=True) and bop.bop_errors need; gt_maps=True implies it. The symmetry sets come from the
    optional keys symmetries_discrete / symmetries_continuous of the tree's models/models_info.yml; a stock
    Linemod_preprocessed tree has none, so every object, eggbox and glue included, then gets the identity
    only and MSSD / MSPD are the plain maximum distances.

    layout="bop" reads `root` as a tree in BOP's own layout (bop_scene.BopTree: one item per GT instance of
    `split`, filtered by the `targets` list and BOP-19's `min_visib` rule; several instances per image, a camera
    matrix and a depth scale per image). Then each crop's K4 is its image's, `objlist` is the tree's (cls_type
    None / "all": the sorted object ids that remain; a name: that object), extent, lfborder, diameter and the
    region points' normalisation come from the tree's models/models_info.json (BOP's models are not in
    Linemod_preprocessed's coordinates), sym_obj holds the classes whose entry there has a symmetry key, and the
    crop boxes are snapped inside the tree's own frame size. masks="png" (default) takes mask_label from the
    tree's mask_visib PNGs; masks="render" (needs meshes=True) takes it from bop.visibility of the GT pose
    against the observed depth, for trees that ship none. layout="linemod" (default) changes nothing.

    detections (a BOP detection file's path or rows; needs layout="bop", refused with masks="render") and
    det_min_score: every kept GT instance is paired with its best detection (bop_scene.BopTree), the crop is snapped
    from the detection's bbox, no mask PNG is read, and batch() decodes the batch's run-length encoded masks into
    mask_label with one rle.decode on the input stream; everything downstream reads that mask_label unchanged. A
    batch then also carries det_score f32 [B] and det_info int32 [B, 5] (rle.decode's info); the GT keys remain the
    paired instance's. Targets without a detection are in tree.missed and yield no item.
    det_per_target="inst_count" (default "best": the above) makes one item of each of a target's `inst_count` best
    detections instead, so that an image may hold an object several times (bop_scene.BopTree). An item's GT keys are
    then a provisional association by box IoU: they feed the per-crop ADD records and the map losses only, and no
    BOP recall reads them (evaluate.test_epoch(..., bop=True) asks for match=True on such a dataset).

    resize=T (default None: nothing changes; a multiple of 40, at least 40) resamples every crop to T x T on the GPU
    (build_inputs(resize=T)): crop_size(i) is T for every crop, so BucketBatcher, bucket_shard, the
    pipeline and test_epoch see one bucket, one plan and full batches whatever the boxes' sides. batch() then also
    carries resize_scale and resize_intrinsic; `bbox` stays the source window in frame coordinates, x/y_map_choosed
    are the resized pixels' centres in the frame, and the cloud is made of the frame's own depth pixels, so PnP,
    verification, refinement and the result files read what they always read. Works on every layout, with or without
    detections; refused (ValueError) with gt_maps=True: the GT maps are not resampled. Only such a dataset can cut
    its crops again about an estimated pose (batch(..., zoom=True), zoom_batch; evaluate.test_epoch(..., zoom=n)).

    model_points="surface" (default "vertices": nothing changes; needs meshes=True or gt_maps=True, ValueError
    otherwise; both layouts): the n_model_pts model points of every object are drawn uniformly on its mesh's surface
    instead of being a random subset of its vertices (models.sample_surface with generator row = the object id and
    `seed`, thinned by FPS from surface_oversample times as many candidates). A model with fewer vertices than
    n_model_pts then opens, which the default mode refuses, and the points follow the shape, not the tessellation.
    They are sampled on the device of the first batch, before it is built, and kept as the tree's model_points;
    `target`, ADD(-S), ICP and the zoom windows read them as they read the vertex subset."""

    def __init__(self, mode: str = "test", num_point: int = 1000, add_noise: bool = False, root: Optional[str] = None,
                 noise_trans: float = 0.0, num_kps: int = 8, cls_type: Optional[str] = None, cfg=CONFIG,
                 num_frames: int = 256, seed: int = 0, sizes: Optional[Sequence[int]] = None,
                 n_model_pts: int = 2600, io_threads: int = 8, gt_maps: bool = False, meshes: bool = False,
                 layout: str = "linemod", split: str = "test", targets: Optional[str] = None, min_visib: float = 0.1,
                 masks: str = "png", detections=None, det_min_score: float = 0.0, det_per_target: str = "best",
                 resize: Optional[int] = None, model_points: str = "vertices", surface_oversample: int = 4):
        if layout not in ("linemod", "bop"):
            raise ValueError(f"layout must be 'linemod' or 'bop', got {layout!r}")
        if model_points not in ("vertices", "surface"):
            raise ValueError(f"model_points must be 'vertices' or 'surface', got {model_points!r}")
        if masks not in ("png", "render"):
            raise ValueError(f"masks must be 'png' or 'render', got {masks!r}")
        if detections is not None and layout != "bop":
            raise ValueError("detections are BOP detection files: they need layout='bop'")
        if detections is not None and masks == "render":
            raise ValueError("detections bring their own masks: they cannot be combined with masks='render'")
        if resize is not None:
            if gt_maps:
                raise ValueError("resize with gt_maps=True is not built: the GT maps are rendered at the frame's "
                                 "resolution and are not resampled")
            if int(resize) != resize or resize < 40 or resize % 40:
                raise ValueError(f"resize must be a multiple of 40 that is at least 40 (the sizes the model is "
                                 f"exercised at); other sizes are not built, got {resize!r}")
        self.resize = None if resize is None else int(resize)
        self.layout, self.masks = layout, masks
        self.detections = detections is not None
        self.mode, self.num_point, self.cfg, self.root = mode, num_point, cfg, root
        self.gt_maps = bool(gt_maps)
        self.meshes = bool(meshes) or self.gt_maps
        if self.meshes and root is None:
            raise ValueError("gt_maps=True / meshes=True render from the objects' meshes and need a LineMOD tree "
                             "(root=None serves synthetic frames, which have no mesh)")
        self.model_points_mode, self.surface_oversample = model_points, int(surface_oversample)
        self.n_model_pts, self.seed = int(n_model_pts), int(seed)
        if model_points == "surface":
            if not self.meshes:
                raise ValueError("model_points='surface' samples the model points on the objects' meshes: it needs "
                                 "meshes=True (or gt_maps=True)")
            if self.surface_oversample < 1 or (self.surface_oversample > 1
                                               and self.n_model_pts * self.surface_oversample > FPS_MAX):
                raise ValueError(f"n_model_pts * surface_oversample = {self.n_model_pts * self.surface_oversample} "
                                 f"candidates: surface_oversample must be >= 1 and the product at most the FPS "
                                 f"kernel's {FPS_MAX}")
        if masks == "render" and not (layout == "bop" and self.meshes):
            raise ValueError("masks='render' renders mask_label from the objects' meshes: it needs layout='bop' and "
                             "meshes=True (or gt_maps=True)")
        if layout == "bop" and root is None:
            raise ValueError("layout='bop' reads a tree in BOP's layout and needs root")
        if cls_type in (None, "all"):
            self.objlist = list(LM_OBJLIST)
        else:
            self.objlist = [OBJ_DICT[cls_type]]
        self.sym_obj = [i for i in SYM_OBJ if i < len(self.objlist)] if len(self.objlist) > 1 else []
        # per object {"min", "size" (mm, [3]), "diameter" (mm)}: the packaged yaml, or a BOP tree's models_info.json
        self.obj_info = models_info()
        self.io_threads = io_threads
        self.frame_hw = (480, 640)
        if layout == "bop":
            self.tree = BopTree(root, split=split, targets=targets,
                                objlist=None if cls_type in (None, "all") else self.objlist, n_model_pts=n_model_pts,
                                seed=seed, meshes=self.meshes, min_visib=min_visib, detections=detections,
                                det_min_score=det_min_score, det_per_target=det_per_target, model_points=model_points)
            self.objlist = list(self.tree.objlist)
            self.obj_info = {o: {"min": [e["min_x"], e["min_y"], e["min_z"]], "size": [e["size_x"], e["size_y"], e["size_z"]],
                                 "diameter": e["diameter"]} for o, e in ((o, self.tree.info[o]) for o in self.objlist)}
            self.sym_obj = [i for i, o in enumerate(self.objlist) if self.tree.has_symmetry(o)]
            self.frame_hw = self.tree.frame_hw or self.frame_hw
            self.frames_np = None
            self.boxes = [get_square_bbox(it["bbox"], *self.frame_hw) for it in self.tree.items]
        elif root is not None:
            self.tree = _LinemodTree(root, mode, self.objlist, n_model_pts, seed, meshes=self.meshes,
                                     model_points=model_points)
            self.frames_np = None
            self.boxes = [get_square_bbox(it["bbox"]) for it in self.tree.items]
        else:
            self.tree = None
            self.frames_np = synthetic_frames(num_frames, seed, self.objlist, sizes=sizes)
            self.boxes = [get_square_bbox([float(v) for v in bb]) for bb in self.frames_np["bbox"]]
        self.diameter = [self.obj_info[o]["diameter"] / 1000.0 for o in self.objlist]
        self._dev_frames: Dict[str, Dict[str, torch.Tensor]] = {}
        self._dev_mesh: Dict[str, Dict[str, object]] = {}
        self._seed: Dict[str, torch.Tensor] = {}
        self._seed_epoch: Dict[str, int] = {}  # how far each device's seed stands past its base (_draw_for)
        self._calls = 0

    def __len__(self):
        return len(self.boxes)

    def crop_size(self, i: int) -> int:
        """The side of crop i as the network sees it: its snapped box's, or `resize` for every crop."""
        if self.resize is not None:
            return self.resize
        rmin, rmax, _, _ = self.boxes[i]
        return rmax - rmin

    def _seed_for(self, device) -> torch.Tensor:
        key = str(device)
        if key not in self._seed:
            self._seed[key] = torch.tensor([int(np.random.SeedSequence(len(self)).generate_state(1)[0])],
                                           dtype=torch.int64, device=device)
            self._seed_epoch[key] = 0
        return self._seed[key]

    def _draw_for(self, device) -> Tuple[torch.Tensor, int]:
        """(seed tensor, stream_id) of batch number self._calls: krrn_choose_points takes ids 0 .. 65534, so the
        id is calls % 65535 and the device seed is the base seed plus calls // 65535, advanced by one each
        time the id wraps: no (seed, stream_id) pair repeats however long the run, and the first 65534 batches
        draw what they always drew."""
        seed = self._seed_for(device)
        key = str(device)
        epoch, sid = divmod(self._calls, CHOOSE_STREAMS)
        if epoch != self._seed_epoch[key]:
            seed += epoch - self._seed_epoch[key]
            self._seed_epoch[key] = epoch
        return seed, sid

    def frames(self, device) -> Dict[str, torch.Tensor]:
        """Synthetic frames, resident on `device` (all of them: 2.4 MB per 640x480 frame)."""
        key = str(device)
        if key not in self._dev_frames:
            self._dev_frames[key] = {k: torch.from_numpy(self.frames_np[k]).to(device)
                                     for k in ("rgb", "depth", "mask_label")}
        return self._dev_frames[key]

    def _read_frames(self, idx: Sequence[int], device) -> Dict[str, torch.Tensor]:
        """Decode the batch's frames from the tree (thread pool) and stage them on `device`."""
        with ThreadPoolExecutor(max_workers=max(1, min(self.io_threads, len(idx)))) as ex:
            if self.layout == "bop":
                # each distinct image is decoded once and stacked per item: the input kernels index the rgb, depth
                # and mask planes by one frame[b] (the cover_frame convention), so per-item frames are what is fed
                its = [self.tree.items[i] for i in idx]
                keys = list(dict.fromkeys((int(it["scene"]), int(it["im"]), float(it["depth_scale"])) for it in its))
                img = dict(zip(keys, ex.map(lambda k: self.tree.read_image(*k), keys)))
                if self.masks == "render" or self.detections:
                    ml = [None] * len(idx)
                else:
                    ml = list(ex.map(self.tree.read_mask, idx))
                fr = [img[(int(it["scene"]), int(it["im"]), float(it["depth_scale"]))] + (m,) for it, m in zip(its, ml)]
            else:
                fr = list(ex.map(self.tree.read, idx))
        out = {"rgb": h2d(torch.from_numpy(np.stack([f[0] for f in fr])), device),
               "depth": h2d(torch.from_numpy(np.stack([f[1] for f in fr])), device)}
        if fr[0][2] is not None:  # masks="render" / detections: batch() makes mask_label on the device
            out["mask_label"] = h2d(torch.from_numpy(np.stack([f[2] for f in fr])), device)
        return out

    def _meta(self, i: int):
        """(obj id, R [3,3] f64, t [3] f64, model points [P,3] f32) of crop i."""
        if self.tree is not None:
            it = self.tree.items[i]
            obj = int(it["obj"])
            return obj, it["R"], it["t"], self.tree.model_points[obj]
        f = self.frames_np
        return (int(f["obj_id"][i]), f["target_r"][i].astype(np.float64), f["target_t"][i].astype(np.float64),
                f["model_points"][i])

    def _sample_model_points(self, device) -> None:
        """model_points="surface": the n_model_pts points of every object, drawn once on `device` uniformly on its
        mesh (models.sample_surface: generator row = the object id, the dataset's seed, FPS-thinned from
        surface_oversample times as many candidates) and kept as the tree's model_points, where the default mode keeps
        its vertex subset. The draw depends on (seed, object id, mesh) only, so every device gives the same points."""
        mesh = self._mesh_for(device)
        s = sample_surface(mesh["verts"], mesh["faces"], torch.tensor([mesh["range"][o] for o in self.objlist],
                                                                       dtype=torch.int32),
                           self.n_model_pts, seed=self.seed, row_id=torch.tensor(self.objlist, dtype=torch.int32),
                           oversample=self.surface_oversample)
        status, pts = s["status"].cpu().tolist(), s["points"].cpu().numpy()
        for j, obj in enumerate(self.objlist):
            if status[j] != 0:
                raise ValueError(f"model_points='surface': the mesh of object {obj} has no area (only degenerate faces)")
            self.tree.model_points[obj] = pts[j]

    def _mesh_for(self, device) -> Dict[str, object]:
        """The objects' meshes on `device`, concatenated (faces index the concatenated vertices), each
        object's face range (`range`), vertex range (`vrange`) and symmetry range (`srange`) into the
        concatenated symmetry sets (`syms` f64 [NStot, 12]), and with gt_maps its 64 FPS region points
        (metres, from vertex 0: sample_model.py:33-46) and its `region_point` rows (a [0, 0, 0] row, then the
        normalised points, batchdataset.py:723-728). Built once per device."""
        key = str(device)
        if key not in self._dev_mesh:
            info = self.obj_info
            if self.tree is None or not self.tree.mesh:
                raise ValueError("this dataset holds no meshes: build it on a LineMOD tree with meshes=True (or "
                                 "gt_maps=True); root=None serves synthetic frames, which have no mesh")
            vs, fs, ss, frange, vrange, srange, v0, f0, s0 = [], [], [], {}, {}, {}, 0, 0, 0
            for obj in self.objlist:
                v, f = self.tree.mesh[obj]
                sy = self.tree.symmetries[obj]
                vs.append(v)
                fs.append(f + v0)
                ss.append(sy)
                frange[obj], vrange[obj], srange[obj] = (f0, len(f)), (v0, len(v)), (s0, len(sy))
                v0, f0, s0 = v0 + len(v), f0 + len(f), s0 + len(sy)
            region, region_point = {}, {}
            for obj in self.objlist if self.gt_maps else ():
                pts = region_points(h2d(torch.from_numpy(self.tree.mesh[obj][0]), device), N_REGIONS)
                lf, ext = np.array(info[obj]["min"]) / 1000.0, np.array(info[obj]["size"]) / 1000.0
                nrm = (pts.cpu().numpy().astype(np.float64) - lf) / ext
                region[obj] = pts
                region_point[obj] = h2d(torch.from_numpy(np.concatenate([np.zeros((1, 3)), nrm]).astype(np.float32)),
                                        device)
            self._dev_mesh[key] = {"verts": h2d(torch.from_numpy(np.concatenate(vs)), device),
                                   "faces": h2d(torch.from_numpy(np.concatenate(fs).astype(np.int32)), device),
                                   "syms": h2d(torch.from_numpy(np.concatenate(ss)), device),
                                   "range": frange, "vrange": vrange, "srange": srange, "region": region,
                                   "region_point": region_point}
        return self._dev_mesh[key]

    def batch(self, indices: Sequence[int], device, bop: bool = False, verify: bool = False,
              zoom: bool = False) -> Dict[str, torch.Tensor]:
        """The eval keys of batchdataset.py:730-771 for `indices` (one crop size), collated. With gt_maps
        also the per-pixel GT of :755-759 (xyz, normal, region, mask, multi_cls_mask), mask_obj,
        region_point, coordinate_choosed and depth_render: the object's mesh is rendered under the GT pose
        (raster.render_maps), its coverage is the point mask's `mask_obj` factor (:667-670), and
        raster.finish_maps applies the loader's masking. bop=True (needs meshes; ValueError otherwise) adds
        what bop.bop_errors reads: bop_depth [F, H, W] the observed depth frames (metres), bop_frame int32 [B]
        each crop's frame, bop_face_range / bop_vert_range / bop_sym_range int32 [B, 2] its object's ranges in
        the dataset's resident meshes and symmetry sets. The other keys are unchanged. verify=True implies the
        bop=True keys and adds verify_mask u8 [F, H, W], the mask_label frames the crops were cut from (the
        rendered ones with masks="render"), for pose.select_pose; the crop's box is the `bbox` key.
        zoom=True (needs a dataset built with resize; ValueError otherwise) adds what zoom_batch needs to cut the crops
        again: zoom_rgb / zoom_depth / zoom_mask the frames these crops were cut from (the decoded detection masks or
        the rendered masks where the dataset uses those), zoom_frame int32 [B] each crop's frame, zoom_rc int32 [B, 2]
        and zoom_side int32 [B] the windows in use, and zoom_depth_scale (a host scalar tensor). They alias bop_depth,
        bop_frame and verify_mask where those exist. The other keys are unchanged."""
        device = torch.device(device)
        idx = list(indices)
        bop = bop or verify
        if self.model_points_mode == "surface" and not self.tree.model_points:
            self._sample_model_points(device)
        if zoom and self.resize is None:
            raise ValueError("zoom needs a dataset built with resize: a re-cut window has a side of its own, which "
                             "only the resized input path takes")
        if bop and not self.meshes:
            raise ValueError("batch(..., bop=True) needs the objects' meshes: build the dataset on a LineMOD tree "
                             "with meshes=True (or gt_maps=True); root=None serves synthetic frames, which have none")
        if self.tree is not None:
            fr = self._read_frames(idx, device)
            fidx = list(range(len(idx)))
        else:
            fr = self.frames(device)
            fidx = idx
        if self.layout == "bop":
            K4 = torch.tensor([self.tree.items[i]["K4"] for i in idx], dtype=torch.float32)
        else:
            K4 = torch.tensor([[LM_K[0, 0], LM_K[1, 1], LM_K[0, 2], LM_K[1, 2]]] * len(idx), dtype=torch.float32)
        self._calls += 1
        boxes = [self.boxes[i] for i in idx]
        metas = [self._meta(i) for i in idx]
        R64 = torch.from_numpy(np.stack([m[1] for m in metas]))
        t64 = torch.from_numpy(np.stack([m[2] for m in metas]))
        det = None
        if self.detections:  # the detections' masks: one decode of the batch's runs, on this (the input) stream
            runs = [self.tree.items[i]["rle"] for i in idx]
            det = _rle.decode(np.concatenate([np.asarray(r, np.int64) for r in runs]),
                              np.cumsum([0] + [len(r) for r in runs]), *fr["depth"].shape[1:], device)
            fr["mask_label"] = det["mask"]
        if "mask_label" not in fr:  # masks="render": the visible mask of the GT pose against the observed depth
            mesh = self._mesh_for(device)
            fr["mask_label"] = _bop.visibility(
                mesh["verts"], mesh["faces"], torch.tensor([mesh["range"][m[0]] for m in metas], dtype=torch.int32),
                R64, t64, K4, fr["depth"], torch.tensor(fidx, dtype=torch.int32))["mask_visib"]
        maps = None
        if self.gt_maps:
            mesh = self._mesh_for(device)
            maps = render_maps(mesh["verts"], mesh["faces"],
                               torch.tensor([mesh["range"][m[0]] for m in metas], dtype=torch.int32), R64, t64, K4,
                               boxes, torch.stack([mesh["region"][m[0]] for m in metas]),
                               frame_hw=tuple(fr["depth"].shape[1:]))
        seed, sid = self._draw_for(device)
        if self.resize is None:
            out = build_inputs(fr, fidx, boxes, self.num_point, K4, seed, stream_id=sid,
                               obj_mask=maps["cover_frame"] if maps is not None else None)
        else:  # build_inputs(resize=), and the windows it staged for zoom=True below (no maps: resize refuses gt_maps)
            out, win = _build_inputs_resize(fr, fidx, boxes, self.num_point, K4, seed, sid, 1.0, None, self.resize)
        info = self.obj_info
        ext = [np.array(info[m[0]]["size"]) / 1000.0 for m in metas]
        lfb = [np.array(info[m[0]]["min"]) / 1000.0 for m in metas]
        # every object keeps exactly num_pt_mesh_large model points (_LinemodTree / synthetic_frames), so
        # a batch mixing objects stacks them without cutting any crop's ADD(-S) point set
        assert len({len(m[3]) for m in metas}) == 1, [len(m[3]) for m in metas]
        mp = torch.from_numpy(np.stack([m[3] for m in metas]))
        host = {
            "cls_id": torch.tensor([[self.objlist.index(m[0])] for m in metas], dtype=torch.int64),
            "intrinsic": K4,
            "extent": torch.from_numpy(np.stack(ext)),
            "lfborder": torch.from_numpy(np.stack(lfb)),
            "bbox": torch.tensor([[b[0], b[1], b[2], b[3]] for b in (self.boxes[i] for i in idx)], dtype=torch.float32),
            "target_r": R64.float(), "target_t": t64.float(), "model_points": mp,
            # model_points @ target_r.T + target_t in f64, then float32 (batchdataset.py:706, 765)
            "target": (mp.double() @ R64.transpose(1, 2) + t64[:, None]).float(),
        }
        out.update({k: h2d(v, device) for k, v in host.items()})
        if maps is not None:
            B, N, S = len(idx), self.num_point, boxes[0][1] - boxes[0][0]
            out.update(finish_maps(maps, out["point_mask"], out["cls_id"], out["extent"], out["lfborder"]))
            out["region_point"] = torch.stack([mesh["region_point"][m[0]] for m in metas])
            out["depth_render"] = maps["depth"]
            # coordinate_choosed (:688): the rendered model coordinates at `choose`, columns 3..5 of the packed
            # [cloud | xyz | normal] gather
            p9 = torch.empty((B, N, 9), dtype=torch.float32, device=device)
            _lib.call("krrn_points_gather_f32", ptr(out["cloud"]), ptr(maps["coord"]), ptr(out["normal"]),
                      ptr(out["choose"]), B, N, S, S, ptr(p9), stream_ptr(device))
            out["coordinate_choosed"] = p9[:, :, 3:6]
        if bop:
            mesh = self._mesh_for(device)
            rng = lambda k: h2d(torch.tensor([mesh[k][m[0]] for m in metas], dtype=torch.int32), device)  # noqa: E731
            out.update({"bop_depth": fr["depth"], "bop_frame": h2d(torch.tensor(fidx, dtype=torch.int32), device),
                        "bop_face_range": rng("range"), "bop_vert_range": rng("vrange"),
                        "bop_sym_range": rng("srange")})
        if verify:
            out["verify_mask"] = fr["mask_label"]
        if det is not None:
            out["det_score"] = h2d(torch.tensor([self.tree.items[i]["score"] for i in idx], dtype=torch.float32), device)
            out["det_info"] = det["info"]
        if zoom:
            out.update({"zoom_rgb": fr["rgb"], "zoom_depth": fr["depth"], "zoom_mask": fr["mask_label"],
                        "zoom_frame": out["bop_frame"] if bop else win[0], "zoom_rc": win[1], "zoom_side": win[2],
                        "zoom_depth_scale": torch.tensor(1.0, dtype=torch.float64)})  # the build's, above
        return out

    def zoom_batch(self, data: Dict[str, torch.Tensor], R: torch.Tensor, t: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The batch `data` (made with batch(..., zoom=True), or by this method) cut again about the pose estimate
        R [B, 3, 3], t [B, 3] (GPU tensors): zoom.pose_windows turns the poses into windows on the device and
        build_inputs_windows crops them, with a fresh draw (`_calls` advances and `_draw_for` gives the stream id, as in
        batch()). Returns a dict like `data` with img_croped, choose, cloud, x_map_choosed, y_map_choosed, point_mask,
        mask_count, bbox, resize_scale, resize_intrinsic, zoom_rc and zoom_side replaced and zoom_status int32 [B]
        (zoom.pose_windows' status: a crop whose pose gives no window keeps its previous one) added; every other key
        is `data`'s own tensor. Queued on the current stream; no host round trip."""
        if self.resize is None:
            raise ValueError("zoom needs a dataset built with resize")
        if "zoom_rc" not in data:
            raise ValueError("zoom_batch needs a batch made with dataset.batch(indices, device, zoom=True)")
        device = data["zoom_depth"].device
        win = pose_windows(data["model_points"], R, t, data["intrinsic"], tuple(data["zoom_depth"].shape[1:]),
                           data["zoom_rc"], data["zoom_side"], self.resize)
        self._calls += 1
        seed, sid = self._draw_for(device)
        fr = {"rgb": data["zoom_rgb"], "depth": data["zoom_depth"], "mask_label": data["zoom_mask"]}
        out = dict(data)
        out.update(build_inputs_windows(fr, data["zoom_frame"], win["rc"], win["side"], self.num_point,
                                        data["intrinsic"], seed, sid, float(data["zoom_depth_scale"]), None, self.resize))
        out.update({"bbox": win["bbox"], "resize_scale": win["resize_scale"], "resize_intrinsic": win["resize_intrinsic"],
                    "zoom_rc": win["rc"], "zoom_side": win["side"], "zoom_status": win["status"]})
        return out

    def __getitem__(self, i: int) -> Dict[str, torch.Tensor]:
        dev = torch.device("cuda", torch.cuda.current_device())
        return {k: v[0].cpu() for k, v in self.batch([i], dev).items()}


class BucketBatcher:
    """Size-bucketed eval batches: the reference's process_patch_datas
    (tools/trainer.py:521-551) accumulates crops per square size and emits a batch of `bs` from a
    bucket holding more than `bs`; here every bucket is drained in `bs`-sized batches (the last
    one short) so each crop is evaluated exactly once, in dataset order within a bucket.
    Yields (S, [indices])."""

    def __init__(self, dataset: PoseDataset, bs: int, shuffle_buckets: bool = False, seed: int = 0):
        self.ds, self.bs = dataset, bs
        self.shuffle_buckets, self.seed = shuffle_buckets, seed

    def buckets(self) -> "OrderedDict[int, List[int]]":
        b: "OrderedDict[int, List[int]]" = OrderedDict()
        for i in range(len(self.ds)):
            b.setdefault(self.ds.crop_size(i), []).append(i)
        return OrderedDict(sorted(b.items()))

    def __iter__(self) -> Iterator[Tuple[int, List[int]]]:
        batches = []
        for S, idx in self.buckets().items():
            for lo in range(0, len(idx), self.bs):
                batches.append((S, idx[lo:lo + self.bs]))
        if self.shuffle_buckets:
            random.Random(self.seed).shuffle(batches)
        return iter(batches)

    def __len__(self):
        return sum((len(v) + self.bs - 1) // self.bs for v in self.buckets().values())
