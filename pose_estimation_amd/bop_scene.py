"""Datasets in BOP's own layout (Hodan et al., "BOP: Benchmark for 6D Object Pose Estimation", ECCV 2018; the
format of LM-O, YCB-V, T-LESS ... as published): the index of a tree, the GPU counterpart of BOP's
calc_gt_masks / calc_gt_info scripts, and BOP's result CSV.

    tree = BopTree("/data/lmo", split="test", targets="/data/lmo/test_targets_bop19.json", meshes=True)
    write_models_info("/data/mine", device)                      # for a tree that ships no models/models_info.json
    write_gt_info("/data/mine", "test", device, masks=True)      # for a tree that ships no scene_gt_info.json
    write_gt_coco("/data/mine", "test", device)                  # scene_gt_coco.json: COCO ground truth, RLE masks
    write_results("krrn_lmo-test.csv", rows); rows = read_results("krrn_lmo-test.csv")

A tree is read as follows. `models/models_info.json` (millimetres): per object `diameter`, `min_x/y/z`,
`size_x/y/z` and the optional `symmetries_discrete` / `symmetries_continuous`, which are already in the
convention bop.symmetry_set takes. `models/obj_%06d.ply`: read with dataset.ply_vtx / ply_faces, which read ASCII
PLY only; a binary PLY (what some BOP datasets ship) keeps raising their ValueError: convert it first. Per scene
`<split>/%06d/scene_gt.json` (per image a list of {obj_id, cam_R_m2c, cam_t_m2c in mm}), `scene_camera.json`
(per image `cam_K` row-major and `depth_scale`: raw depth x depth_scale = millimetres) and `scene_gt_info.json`
(per instance `visib_fract`, `px_count_visib`, `bbox_visib`, ...); images `rgb/%06d.png` (or .jpg),
`depth/%06d.png` (uint16) and the per-instance `mask_visib/%06d_%06d.png` (image id, GT index).

Detections. BOP distributes detectors' output, and a user's own detector writes, a JSON list of {scene_id, image_id,
category_id, score, bbox = [x, y, w, h], optional segmentation = {"counts": run list or COCO's compressed string,
"size": [H, W]}, optional time} (read_detections / write_detections). BopTree(..., detections=path or rows) pairs
every kept GT instance with the best-scoring detection of its (scene, image, object) and takes the crop box and the
mask from it instead of bbox_visib / mask_visib (the runs are decoded on the GPU per batch: rle.decode);
gt_detections(tree) writes a tree's own ground truth as detections, an upper-bound run.

    rows = read_detections("/data/lmo/detections.json"); write_detections("mine.json", rows)
    tree = BopTree("/data/lmo", targets=..., detections="/data/lmo/detections.json", det_min_score=0.1)

Scoring a result file. eval_results(dataset, rows, device) is the counterpart of the BOP toolkit's
eval_bop19_pose: per (scene, image, object) target the `inst_count` best-scored rows are greedily matched to the
target's kept GT instances (bop.match_poses, on the GPU, once per error function and threshold of correctness)
and recall is matched instances over kept instances, so a target may hold an object several times and a file may
hold several rows per target. BopTree(..., det_per_target="inst_count") makes one item of each of a target's
`inst_count` best detections, which is how such a file comes out of evaluate.test_epoch(..., match=True).

    ds = PoseDataset("test", 1000, False, "/data/tless", layout="bop", targets=..., meshes=True)
    res = eval_results(ds, read_results("krrn_tless-test.csv"), "cuda:0")     # AR_VSD / AR_MSSD / AR_MSPD / AR, ...

Masks of a result file. write_result_masks(path, dataset, rows, device) renders every estimate's visible mask against
the observed depth (bop.visibility under the estimated pose), encodes it on the GPU (rle.encode_planes) and writes
the rows in the detection format above: a segmentation result file, which BopTree(..., detections=path) reads back.
net_mask_rows(rows, runs, info, H, W) makes the same rows from masks that are already run lists: the network's own
segmentation, which evaluate.test_epoch(seg_json=..., seg_source="net") pastes and encodes per batch.

Scoring a detection or segmentation result file. eval_coco(gt, rows, device, iou_type="segm" | "bbox") is the
counterpart of the toolkit's eval_bop22_coco: COCO's average precision of the rows against scene_gt_coco.json, with the
mask IoUs taken from the run lists on the GPU (rle.iou) and the per-image matching there too (coco.match).

    write_gt_coco("/data/mine", "test", device)
    res = eval_coco(("/data/mine", "test"), read_detections("krrn_mine-test_seg.json"), "cuda:0")   # AP, AP50, AR100, ...

Pictures of a result file. vis_results(dataset, rows, out_dir, device) is the counterpart of the toolkit's
vis_est_poses: every image's estimates are rendered into one z-buffer (scene.render), blended over the RGB image in
their objects' colours with outlines, the ground truth's outlines on top, and written as PNGs; diff=True adds the
rendered against the observed depth. evaluate.test_epoch(vis_dir=...) does it for an epoch's own estimates.

    vis_results(ds, read_results("krrn_tless-test.csv"), "vis", "cuda:0", diff=True)   # vis/000001/000000.png, ..._diff.png

Model facts. model_info(root, device) is the counterpart of the toolkit's calc_model_info: every model's diameter (the
maximum over all vertex pairs, models.extent on the GPU) and box; write_models_info writes them as
models/models_info.json, and check_models_info(root, device) sets an existing file beside its PLYs: the diameter and
box differences and, per declared symmetry, how far it moves the mesh off itself (models.symmetry_residual).

    write_models_info("/data/mine", device); rep = check_models_info("/data/tless", device)   # rep[obj]["residual"]

Resampled models. write_models_eval(root, device, n=...) writes models_eval/obj_%06d.ply: n points drawn uniformly on
each model's surface with their normals (models.sample_surface: area-weighted faces, FPS thinning), in the model's own
unit, as ASCII PLY without faces.

    write_models_eval("/data/mine", device, n=4096)

Out of scope: binary PLY, polygon segmentations, keypoints, finding symmetries."""
from __future__ import annotations

import json
import os
from itertools import accumulate
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import bop, rle

INFO_KEYS = ("bbox_obj", "bbox_visib", "px_count_all", "px_count_valid", "px_count_visib", "visib_fract")  # BOP's six


def _load_json(path: str) -> Dict[int, object]:
    with open(path) as f:
        return {int(k): v for k, v in json.load(f).items()}


def scene_ids(root: str, split: str) -> List[int]:
    d = os.path.join(root, split)
    return sorted(int(n) for n in os.listdir(d) if n.isdigit() and os.path.isdir(os.path.join(d, n)))


def _scene_dir(root: str, split: str, scene) -> str:
    return os.path.join(root, split, f"{int(scene):06d}")


def _key(it) -> Tuple[int, int, int]:
    """The (scene, image, object) target of an item or instance."""
    return int(it["scene"]), int(it["im"]), int(it["obj"])


def _image_path(sdir: str, sub: str, im: int) -> str:
    for ext in (".png", ".jpg"):
        p = os.path.join(sdir, sub, f"{im:06d}{ext}")
        if os.path.exists(p):
            return p
    raise FileNotFoundError(os.path.join(sdir, sub, f"{im:06d}.png (or .jpg)"))


def read_depth(sdir: str, im: int, depth_scale: float) -> np.ndarray:
    """depth/%06d.png in metres, f32 [H, W]: (raw as f64 x depth_scale / 1000) rounded to f32 once."""
    from PIL import Image
    with Image.open(os.path.join(sdir, "depth", f"{im:06d}.png")) as di:
        return (np.asarray(di).astype(np.float64) * float(depth_scale) / 1000.0).astype(np.float32)


def load_models(root: str, objs: Sequence[int], faces: bool = True):
    """({obj: its models_info.json entry}, {obj: (verts f32 [V, 3] metres, faces int32 [F, 3])}) of a tree."""
    from .dataset import ply_faces, ply_vtx
    info = _load_json(os.path.join(root, "models", "models_info.json"))
    mesh = {}
    for obj in objs:
        p = os.path.join(root, "models", f"obj_{obj:06d}.ply")
        pts = (ply_vtx(p) / 1000.0).astype(np.float32)
        tri = ply_faces(p) if faces else np.zeros((0, 3), np.int32)
        if faces and len(tri) == 0:
            raise ValueError(f"obj_{obj:06d}.ply has no faces (element face 0): nothing to render")
        if len(tri) and (tri.min() < 0 or tri.max() >= len(pts)):
            raise ValueError(f"obj_{obj:06d}.ply: a face index lies outside its {len(pts)} vertices")
        mesh[obj] = (pts, tri)
    return info, mesh


class BopTree:
    """Index of a BOP tree (module doc) with the interface PoseDataset uses of its LineMOD index: `items`,
    `model_points`, `mesh`, `symmetries`, `read(i)`; also `info` = the tree's models_info.json entries and
    `frame_hw`. One item per GT instance: {"scene", "im", "gt" (index in the image's scene_gt list), "obj", "R" f64
    [3, 3], "t" f64 [3] metres, "K4" (fx, fy, cx, cy), "depth_scale", "bbox" = bbox_visib}.

    targets: the path of a test_targets_bop19.json-style list ({scene_id, im_id, obj_id, inst_count}); only its
    (scene, image, object) triples are kept. Instances with visib_fract < min_visib or px_count_visib == 0 are
    dropped: BOP-19's rule for which GT instances count. objlist: the objects to keep; default the sorted ids
    that remain. A scene without scene_gt_info.json raises FileNotFoundError naming write_gt_info.

    detections: None, or a detection file's path or rows (module doc). The items are still the GT instances kept
    above, each paired with one detection: among the rows whose (scene_id, image_id, category_id) are the item's and
    whose score >= det_min_score, the highest score, ties to the earliest row. Rows without a set mask pixel or with
    w <= 0 or h <= 0 are dropped before pairing. A paired item's "bbox" is the detection's, and it gains "score",
    "det" (the row's index) and "rle" (the mask's run list; the filled box's runs for a row without segmentation).
    A kept target without a detection yields no item and is listed in `missed` as (scene, im, obj); `objlist` stays
    the kept targets'. `det_stats` = {"rows", "used", "unused", "dropped"}: all rows, those paired, those not chosen
    for any kept target, those dropped before pairing. ValueError: a segmentation whose size is not the tree's frame
    size or whose runs do not fill it, and two or more kept instances of one object in one image.

    Whatever the detection mode, `instances` holds the kept GT instances (what `items` is without detections) and
    `inst_count` = {(scene, im, obj): n} the kept targets' instance counts: the targets file's own `inst_count` where
    a file is given, else the number of kept instances. eval_results matches against these.

    det_per_target: "best" (the pairing above, its refusal of multi-instance targets included) or "inst_count". With
    "inst_count" every kept target contributes one item per detection among its `inst_count` best rows (the same
    qualifying rule, score descending, ties to the earlier row); the items stand target by target in the order of
    `instances`, each target's by rank, with the crop box, score and runs of their row as above. An item still needs
    GT keys for the per-crop ADD records and the map losses: it takes those of the target's kept instance whose
    bbox_visib has the highest IoU with the detection's box (ties to the lowest GT index; two items may take the
    same instance). That association is provisional: it feeds only those columns, and no BOP recall reads it
    (eval_results matches estimates to instances by their pose errors). A target with fewer qualifying rows than
    `inst_count` adds its key to `missed` once per missing estimate, so len(items) + len(missed) is the sum of
    `inst_count`; `det_stats` keeps its meaning ("used" = the rows that became items).

    model_points: "vertices" (the random vertex subset above, which refuses a model with fewer than n_model_pts
    vertices) or "surface" (needs meshes=True): `model_points` stays empty here and PoseDataset fills it with
    models.sample_surface's points before its first batch."""

    def __init__(self, root: str, split: str = "test", targets: Optional[str] = None,
                 objlist: Optional[Sequence[int]] = None, n_model_pts: int = 2600, seed: int = 0, meshes: bool = False,
                 min_visib: float = 0.1, detections=None, det_min_score: float = 0.0, det_per_target: str = "best",
                 model_points: str = "vertices"):
        if det_per_target not in ("best", "inst_count"):
            raise ValueError(f"det_per_target must be 'best' or 'inst_count', got {det_per_target!r}")
        if model_points == "surface" and not meshes:
            raise ValueError("model_points='surface' samples the model points on the objects' meshes: it needs meshes=True")
        self.root, self.split = root, split
        self.det_per_target = det_per_target
        self.missed: List[Tuple[int, int, int]] = []
        self.det_stats: Optional[Dict[str, int]] = None
        want = None
        if targets is not None:
            with open(targets) as f:
                want = {(int(e["scene_id"]), int(e["im_id"]), int(e["obj_id"])): int(e.get("inst_count", 0))
                        for e in json.load(f)}
        keep_obj = None if objlist is None else {int(o) for o in objlist}
        self.items: List[Dict[str, object]] = []
        self.frame_hw: Optional[Tuple[int, int]] = None
        for sc in scene_ids(root, split):
            sdir = _scene_dir(root, split, sc)
            gt = _load_json(os.path.join(sdir, "scene_gt.json"))
            cam = _load_json(os.path.join(sdir, "scene_camera.json"))
            ipath = os.path.join(sdir, "scene_gt_info.json")
            if not os.path.exists(ipath):
                raise FileNotFoundError(f"{ipath} is missing: a tree without it (recorded or rendered by the user) "
                                        "gets one from bop_scene.write_gt_info(root, split, device)")
            ginfo = _load_json(ipath)
            for im in sorted(gt):
                K = [float(k) for k in cam[im]["cam_K"]]
                for g, (e, gi) in enumerate(zip(gt[im], ginfo[im])):
                    obj = int(e["obj_id"])
                    if want is not None and (sc, im, obj) not in want:
                        continue
                    if keep_obj is not None and obj not in keep_obj:
                        continue
                    if float(gi["visib_fract"]) < min_visib or int(gi["px_count_visib"]) == 0:
                        continue
                    self.items.append({"scene": sc, "im": im, "gt": g, "obj": obj,
                                       "R": np.array(e["cam_R_m2c"], np.float64).reshape(3, 3),
                                       "t": np.array(e["cam_t_m2c"], np.float64) / 1000.0,
                                       "K4": (K[0], K[4], K[2], K[5]),
                                       "depth_scale": float(cam[im].get("depth_scale", 1.0)),
                                       "bbox": [float(v) for v in gi["bbox_visib"]]})
        self.objlist = sorted({int(it["obj"]) for it in self.items}) if objlist is None else [int(o) for o in objlist]
        if self.items:
            it = self.items[0]
            from PIL import Image
            with Image.open(os.path.join(self._sdir(it), "depth", f"{int(it['im']):06d}.png")) as di:
                self.frame_hw = (di.size[1], di.size[0])
        self.instances: List[Dict[str, object]] = list(self.items)
        self.inst_count: Dict[Tuple[int, int, int], int] = {}
        for it in self.instances:
            self.inst_count[_key(it)] = self.inst_count.get(_key(it), 0) + 1
        if want is not None:  # the targets file's own count, where it states one
            self.inst_count = {k: (want[k] if want[k] > 0 else n) for k, n in self.inst_count.items()}
        if detections is not None:
            self._pair(detections, float(det_min_score))
        self.info, mesh = load_models(root, self.objlist, faces=meshes)
        self.mesh: Dict[int, Tuple[np.ndarray, np.ndarray]] = mesh if meshes else {}
        self.symmetries: Dict[int, np.ndarray] = {}
        self.model_points: Dict[int, np.ndarray] = {}
        rng = np.random.default_rng(seed)
        for obj in self.objlist:  # the LineMOD index's subsampling, draw for draw
            pts = mesh[obj][0]
            oi = self.info.get(obj, {})
            if meshes:
                self.symmetries[obj] = bop.symmetry_set(oi.get("symmetries_discrete"), oi.get("symmetries_continuous"))
            if model_points == "surface":  # PoseDataset samples them on the mesh before its first batch
                continue
            if len(pts) < n_model_pts:
                raise ValueError(f"obj_{obj:06d}.ply has {len(pts)} vertices < num_pt_mesh_large = {n_model_pts}")
            if len(pts) > n_model_pts:
                pts = pts[np.sort(rng.choice(len(pts), n_model_pts, replace=False))]
            self.model_points[obj] = pts.astype(np.float32)

    def _pair(self, detections, min_score: float) -> None:
        """Pair the kept targets with detection rows (class doc): each target's best row, or with
        det_per_target="inst_count" its inst_count best, one item each."""
        counted = self.det_per_target == "inst_count"
        rows, cand, dropped = _candidates(detections, [_key(it) for it in self.instances], min_score)
        groups: Dict[Tuple[int, int, int], List[Dict[str, object]]] = {}
        for it in self.instances:
            key = _key(it)
            if key in groups and not counted:
                raise ValueError(f"target (scene {key[0]}, image {key[1]}, object {key[2]}) has more than one kept GT "
                                 "instance (inst_count > 1): matching several estimates to several instances is out of "
                                 "scope with detections")
            groups.setdefault(key, []).append(it)
        items = []
        for key, inst in groups.items():
            n = self.inst_count[key] if counted else 1
            top = _by_score(rows, cand[key], nan_ok=not counted)[:n]
            for j in top:
                # the GT keys are lent by the kept instance whose bbox_visib overlaps the row's box most: "best" has
                # one instance per target, argmax takes the lowest GT index on ties
                ious = [_box_iou(it["bbox"], rows[j]["bbox"]) for it in inst]
                items.append(self._det_item(inst[int(np.argmax(ious))], rows, j))
            self.missed += [key] * (n - len(top))
        self.items = items
        self.det_stats = {"rows": len(rows), "used": len(items), "unused": len(rows) - len(items) - dropped,
                          "dropped": dropped}

    def _det_item(self, it, rows, j: int) -> Dict[str, object]:
        """The GT instance `it` as an item whose box, score and mask runs are detection row j's."""
        H, W = self.frame_hw if self.frame_hw else (0, 0)
        r = rows[j]
        seg = r.get("segmentation")
        if seg is None:
            runs = rle.box_counts(*r["bbox"], H, W)
        else:
            if tuple(seg["size"]) != (H, W):
                raise ValueError(f"detection {j}: segmentation.size {list(seg['size'])} is not the tree's "
                                 f"frame size {[H, W]}")
            runs = list(seg["counts"])
            if min(runs) < 0 or sum(runs) != H * W:
                raise ValueError(f"detection {j}: its runs do not fill the {H} x {W} frame")
        return dict(it, bbox=[float(v) for v in r["bbox"]], score=float(r["score"]), det=j, rle=runs)

    def has_symmetry(self, obj: int) -> bool:
        oi = self.info.get(obj, {})
        return bool(oi.get("symmetries_discrete")) or bool(oi.get("symmetries_continuous"))

    def _sdir(self, it) -> str:
        return _scene_dir(self.root, self.split, it["scene"])

    def read_image(self, scene: int, im: int, depth_scale: float):
        """(rgb u8 [H, W, 3], depth f32 [H, W] metres) of one image."""
        from PIL import Image
        sdir = _scene_dir(self.root, self.split, scene)
        with Image.open(_image_path(sdir, "rgb", im)) as ri:
            rgb = np.array(ri.convert("RGB"))
        return rgb, read_depth(sdir, im, depth_scale)

    def read_mask(self, i: int) -> np.ndarray:
        from PIL import Image
        it = self.items[i]
        with Image.open(os.path.join(self._sdir(it), "mask_visib", f"{int(it['im']):06d}_{int(it['gt']):06d}.png")) as li:
            label = np.array(li)
        return ((label[:, :, 0] if label.ndim == 3 else label) != 0).astype(np.uint8)

    def read(self, i: int):
        it = self.items[i]
        rgb, depth = self.read_image(int(it["scene"]), int(it["im"]), float(it["depth_scale"]))
        return rgb, depth, self.read_mask(i)


def _box_iou(a, b) -> float:
    """Intersection over union of two (x, y, w, h) boxes as plain rectangles; 0.0 without a union."""
    ax, ay, aw, ah = (float(v) for v in a)
    bx, by, bw, bh = (float(v) for v in b)
    iw = max(0.0, min(ax + aw, bx + bw) - max(ax, bx))
    ih = max(0.0, min(ay + ah, by + bh) - max(ay, by))
    inter = iw * ih
    union = max(aw, 0.0) * max(ah, 0.0) + max(bw, 0.0) * max(bh, 0.0) - inter
    return inter / union if union > 0.0 else 0.0


def _candidates(detections, keys, min_score: float):
    """Which detection rows qualify for which kept target (BopTree's class doc): (the rows, {key of `keys`: its
    qualifying rows' indices in file order}, the rows dropped for a box with w <= 0 or h <= 0 or a mask without a set
    pixel). A row qualifies unless its score is below min_score."""
    rows = read_detections(detections) if isinstance(detections, (str, os.PathLike)) else _check_rows(detections, "rows")
    cand: Dict[Tuple[int, int, int], List[int]] = {k: [] for k in keys}
    dropped = 0
    for j, r in enumerate(rows):
        seg = r.get("segmentation")
        if r["bbox"][2] <= 0 or r["bbox"][3] <= 0 or (seg is not None and sum(seg["counts"][1::2]) <= 0):
            dropped += 1
            continue
        key = (r["scene_id"], r["image_id"], r["category_id"])
        if key in cand and not r["score"] < min_score:
            cand[key].append(j)
    return rows, cand, dropped


def _by_score(rows, js: List[int], nan_ok: bool) -> List[int]:
    """The row indices `js` (in file order) by score descending, ties to the earlier row: "best" takes the first,
    "inst_count" the first inst_count. A NaN score compares false with everything, and each mode keeps what that has
    always meant for it. "inst_count" (nan_ok=False) asked for score >= det_min_score, so it never takes such a row.
    "best" scanned the rows and replaced the one it held only for a strictly greater score: a NaN row that stands
    first in file order is never displaced, any other is never picked."""
    nan = lambda j: rows[j]["score"] != rows[j]["score"]  # noqa: E731
    if nan_ok and js and nan(js[0]):
        return js[:1]
    return sorted((j for j in js if not nan(j)), key=lambda j: -rows[j]["score"])   # stable: file order on ties


DET_KEYS = ("scene_id", "image_id", "category_id", "score", "bbox")


def _check_rows(rows, where: str) -> List[Dict[str, object]]:
    """Detection rows in this module's normal form: ints, a float score, bbox as 4 floats, segmentation (if any)
    as {"counts": run list, "size": [H, W]} (a compressed string is decoded here), time (if any) a float.
    ValueError with the entry's index for a missing required key, a bbox that is not 4 numbers, or a segmentation
    without both keys."""
    if not isinstance(rows, (list, tuple)):
        raise ValueError(f"{where}: a list of detections expected, got {type(rows).__name__}")
    out = []
    for j, r in enumerate(rows):
        if not isinstance(r, dict):
            raise ValueError(f"{where}: entry {j} is not an object")
        for k in DET_KEYS:
            if k not in r:
                raise ValueError(f"{where}: entry {j} has no '{k}'")
        bb = r["bbox"]
        if not isinstance(bb, (list, tuple)) or len(bb) != 4 or not all(
                isinstance(v, (int, float)) and not isinstance(v, bool) for v in bb):
            raise ValueError(f"{where}: entry {j}: bbox must be 4 numbers [x, y, w, h], got {bb!r}")
        e = {"scene_id": int(r["scene_id"]), "image_id": int(r["image_id"]), "category_id": int(r["category_id"]),
             "score": float(r["score"]), "bbox": [float(v) for v in bb]}
        seg = r.get("segmentation")
        if seg is not None:
            if not isinstance(seg, dict) or "counts" not in seg or "size" not in seg:
                raise ValueError(f"{where}: entry {j}: segmentation needs both 'counts' and 'size'")
            c = seg["counts"]
            try:
                runs = rle.counts_from_string(c) if isinstance(c, str) else [int(v) for v in c]
                size = [int(v) for v in seg["size"]]
            except (TypeError, ValueError) as err:
                raise ValueError(f"{where}: entry {j}: bad segmentation ({err})") from None
            if len(size) != 2:
                raise ValueError(f"{where}: entry {j}: segmentation.size must be [H, W], got {seg['size']!r}")
            e["segmentation"] = {"counts": runs, "size": size}
        if "time" in r:
            e["time"] = float(r["time"])
        out.append(e)
    return out


def read_detections(path) -> List[Dict[str, object]]:
    """A file in BOP's detection / segmentation result format (module doc) as rows in _check_rows' normal form."""
    with open(path) as f:
        return _check_rows(json.load(f), str(path))


def write_detections(path, rows) -> None:
    """The same format, masks as run lists; read_detections returns what was written."""
    with open(path, "w") as f:
        json.dump(_check_rows(rows, "rows"), f)


def _mask_row(sc, im, obj, score, bbox, counts, size, time=None) -> Dict[str, object]:
    """One detection row with a mask in _check_rows' normal form; without `time` the key is left out."""
    return {"scene_id": int(sc), "image_id": int(im), "category_id": int(obj), "score": float(score),
            "bbox": [float(v) for v in bbox], "segmentation": {"counts": counts, "size": [int(size[0]), int(size[1])]},
            **({} if time is None else {"time": float(time)})}


def gt_detections(tree: "BopTree") -> List[Dict[str, object]]:
    """Oracle detections of a tree built without detections: one row per item, from its bbox_visib and its
    mask_visib PNG, with score 1.0. A dataset built on them equals the tree's own PNG mode (an upper-bound run)."""
    if tree.det_stats is not None:
        raise ValueError("gt_detections reads bbox_visib: build the tree without detections")
    rows = []
    for i, it in enumerate(tree.items):
        m = tree.read_mask(i)
        rows.append(_mask_row(*_key(it), 1.0, it["bbox"], rle.encode(m), m.shape))
    return rows


def _save_json(path: str, content: Dict[int, object]) -> None:
    with open(path, "w") as f:
        json.dump({str(k): v for k, v in sorted(content.items())}, f, indent=1)


def _require(dataset, message: str, layout: bool = False, meshes: bool = False) -> None:
    """ValueError(message) unless `dataset` is a PoseDataset with layout="bop" (layout=True) and / or with
    meshes=True (meshes=True)."""
    if (layout and getattr(dataset, "layout", "linemod") != "bop") or (meshes and not getattr(dataset, "meshes", False)):
        raise ValueError(message)


def _refuse(path: str, overwrite: bool) -> None:
    if os.path.exists(path) and not overwrite:
        raise FileExistsError(f"{path} exists (overwrite=True replaces it)")


def _visibility(verts, faces, ranges, R, t, K4, depth, frame, delta: float, masks: bool = True):
    """bop.visibility of B poses whose operands are host lists: (first face, faces), R (9 or [3, 3] f64), t (f64
    metres), (fx, fy, cx, cy) and the index into depth's frames, per pose; verts / faces / depth on the device."""
    return bop.visibility(verts, faces, torch.tensor(ranges, dtype=torch.int32), torch.from_numpy(np.stack(R)),
                          torch.from_numpy(np.stack(t)), torch.tensor(K4, dtype=torch.float32), depth,
                          torch.tensor(frame, dtype=torch.int32), 1.0, delta, masks=masks)


def _gt_batches(root: str, split: str, device, fname: str, overwrite: bool, batch: int, delta: float, masks: bool):
    """What the ground-truth writers share. Reads every scene's scene_gt.json and puts the meshes of the objects they
    name on `device`, concatenated. Then yields per scene (scene id, its directory, the path of its `fname`, its
    scene_gt.json, its instances [(image, GT index, scene_gt entry)] in image and GT order, the split's objects,
    batches); `batches` yields, per at most `batch` instances and only when asked, (that slice of the instances,
    bop.visibility's result for it: the slice's distinct images' depth frames are read once). FileExistsError for an
    existing `fname` unless overwrite, before anything is computed for that scene."""
    from .runtime import h2d
    device = torch.device(device)
    scenes = scene_ids(root, split)
    gts = {sc: _load_json(os.path.join(_scene_dir(root, split, sc), "scene_gt.json")) for sc in scenes}
    objs = sorted({int(e["obj_id"]) for gt in gts.values() for v in gt.values() for e in v})
    _, mesh = load_models(root, objs)
    v0 = f0 = 0
    frange, vs, fs = {}, [], []
    for obj in objs:
        v, f = mesh[obj]
        vs.append(v)
        fs.append(f + v0)
        frange[obj] = (f0, len(f))
        v0, f0 = v0 + len(v), f0 + len(f)
    verts = h2d(torch.from_numpy(np.concatenate(vs)), device)
    faces = h2d(torch.from_numpy(np.concatenate(fs).astype(np.int32)), device)

    def visibility(sdir, cam, part):
        ims = list(dict.fromkeys(im for im, _, _ in part))
        depth = np.stack([read_depth(sdir, im, float(cam[im].get("depth_scale", 1.0))) for im in ims])
        K = [[float(k) for k in cam[im]["cam_K"]] for im, _, _ in part]
        return _visibility(verts, faces, [frange[int(e["obj_id"])] for _, _, e in part],
                           [np.array(e["cam_R_m2c"], np.float64) for _, _, e in part],
                           [np.array(e["cam_t_m2c"], np.float64) / 1000.0 for _, _, e in part],
                           [[k[0], k[4], k[2], k[5]] for k in K], h2d(torch.from_numpy(depth), device),
                           [ims.index(im) for im, _, _ in part], delta, masks)

    step = max(1, int(batch))
    for sc in scenes:
        sdir = _scene_dir(root, split, sc)
        _refuse(os.path.join(sdir, fname), overwrite)
        cam = _load_json(os.path.join(sdir, "scene_camera.json"))
        inst = [(im, g, e) for im in sorted(gts[sc]) for g, e in enumerate(gts[sc][im])]
        yield (sc, sdir, os.path.join(sdir, fname), gts[sc], inst, objs,
               ((inst[lo:lo + step], visibility(sdir, cam, inst[lo:lo + step])) for lo in range(0, len(inst), step)))


def _info_entry(q: Sequence[int], fract: float) -> Dict[str, object]:
    """One scene_gt_info.json entry from a row of bop.visibility's info (ints) and its visib_fract."""
    return {"bbox_obj": q[3:7], "bbox_visib": q[7:11], "px_count_all": q[0], "px_count_valid": q[1],
            "px_count_visib": q[2], "visib_fract": float(fract)}


def write_gt_info(root: str, split: str, device, masks: bool = False, delta: float = bop.DELTA, batch: int = 64,
                  overwrite: bool = False) -> Dict[int, Dict[int, List[Dict[str, object]]]]:
    """The GPU counterpart of BOP's calc_gt_info / calc_gt_masks for every scene of `root`/`split`:
    bop.visibility over the scene's GT instances in batches of `batch` (each batch decodes its distinct images
    once), written as scene_gt_info.json with BOP's six keys (INFO_KEYS) and, with masks=True, the
    mask/%06d_%06d.png and mask_visib/%06d_%06d.png images (0 / 255). Refuses to overwrite an existing
    scene_gt_info.json or mask file unless overwrite=True (FileExistsError, before anything is computed for that
    scene). Returns {scene: {image: [entry per instance]}}. The two departures from BOP's scripts that
    bop.visibility states apply: bbox_obj is clipped to the frame, and pixels are sampled at integer coordinates."""
    from PIL import Image
    out = {}
    for sc, sdir, ipath, gt, inst, _, batches in _gt_batches(root, split, device, "scene_gt_info.json", overwrite, batch,
                                                           delta, masks):
        if masks:
            for sub in ("mask", "mask_visib"):
                os.makedirs(os.path.join(sdir, sub), exist_ok=True)
                for im, g, _ in inst:
                    _refuse(os.path.join(sdir, sub, f"{im:06d}_{g:06d}.png"), overwrite)
        entries = {im: [None] * len(gt[im]) for im in gt}
        for part, res in batches:
            info, fract = res["info"].cpu().numpy(), res["visib_fract"].cpu().numpy()   # one read-back per batch
            planes = {k: res[k].cpu().numpy() for k in ("mask", "mask_visib")} if masks else {}
            for j, (im, g, _) in enumerate(part):
                entries[im][g] = _info_entry([int(x) for x in info[j]], fract[j])
                for sub, pl in planes.items():
                    Image.fromarray(pl[j] * np.uint8(255)).save(os.path.join(sdir, sub, f"{im:06d}_{g:06d}.png"))
        _save_json(ipath, entries)
        out[sc] = entries
    return out


def write_gt_coco(root: str, split: str, device, visib: bool = True, min_visib: float = 0.1, batch: int = 64,
                  overwrite: bool = False) -> Dict[int, Dict[str, object]]:
    """The GPU counterpart of BOP's calc_gt_coco for every scene of `root`/`split`: COCO ground truth with the
    instances' masks as compressed RLE. Per scene bop.visibility over the GT instances in batches of `batch`, as
    write_gt_info runs it, then rle.encode_planes of the batch's mask_visib planes (visib=False: the full
    silhouettes `mask`), so only the runs leave the device. Written as scene_gt_coco.json:
      "images"       id = the image id, file_name relative to the scene directory (rgb/%06d.png, or .jpg where the
                     tree holds that), width, height
      "annotations"  id (1, 2, .. in image and GT order), image_id, category_id = obj_id, iscrowd 0, area = the
                     plane's pixel count, bbox = the instance's bbox_visib (bbox_obj with visib=False) as write_gt_info
                     gives it, segmentation = {"counts": COCO's compressed string, "size": [H, W]}, ignore =
                     visib_fract < min_visib
      "categories"   id, name "%d" for every object of the split's ground truth
    Refuses to overwrite an existing scene_gt_coco.json unless overwrite=True (FileExistsError, before anything is
    computed for that scene). Returns {scene: that dict}. The layout is written from the published COCO / BOP
    formats and is not checked against the BOP toolkit's own output (the toolkit is not a dependency). The two
    departures from BOP's scripts that bop.visibility states apply: bbox_obj is clipped to the frame, and pixels are
    sampled at integer coordinates."""
    out = {}
    plane, px, box = ("mask_visib", 2, slice(7, 11)) if visib else ("mask", 0, slice(3, 7))
    for sc, sdir, cpath, _, _, objs, batches in _gt_batches(root, split, device, "scene_gt_coco.json", overwrite, batch,
                                                          bop.DELTA, True):
        images, annotations = {}, []
        for part, res in batches:
            H, W = (int(v) for v in res[plane].shape[1:])
            runs = rle.encode_planes(res[plane])
            info, fract = res["info"].cpu().numpy(), res["visib_fract"].cpu().numpy()
            for j, (im, g, e) in enumerate(part):
                if im not in images:
                    jpg = not os.path.exists(os.path.join(sdir, "rgb", f"{im:06d}.png")) and os.path.exists(
                        os.path.join(sdir, "rgb", f"{im:06d}.jpg"))
                    images[im] = {"id": im, "file_name": f"rgb/{im:06d}{'.jpg' if jpg else '.png'}", "width": W, "height": H}
                q = [int(x) for x in info[j]]
                annotations.append({"id": len(annotations) + 1, "image_id": im, "category_id": int(e["obj_id"]),
                                    "iscrowd": 0, "area": q[px], "bbox": q[box],
                                    "segmentation": {"counts": rle.counts_to_string(runs[j]), "size": [H, W]},
                                    "ignore": bool(float(fract[j]) < min_visib)})
        coco = {"images": [images[im] for im in sorted(images)], "annotations": annotations,
                "categories": [{"id": obj, "name": "%d" % obj} for obj in objs]}
        with open(cpath, "w") as f:
            json.dump(coco, f)
        out[sc] = coco
    return out


MODEL_KEYS = ("diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z")   # calc_model_info's seven


def _model_ids(root: str) -> List[int]:
    """The ids of the models/obj_%06d.ply files of a tree, sorted."""
    names = os.listdir(os.path.join(root, "models"))
    return sorted(int(n[4:10]) for n in names if len(n) == 14 and n.startswith("obj_") and n.endswith(".ply")
                  and n[4:10].isdigit())


def _stage_models(root: str, objs: Sequence[int], device, faces: bool, unit: float = 1000.0):
    """The models of `objs` on `device`, concatenated: (verts f32 [Vtot, 3] metres as every loader of the project
    holds them (ply_vtx / 1000 rounded to f32; unit=1.0 keeps the file's own f32 values), faces int32 [Ftot, 3] into
    verts or None, vert_range, face_range as host int32 [O, 2])."""
    from .dataset import ply_faces, ply_vtx
    from .runtime import h2d
    vs, fs, vr, fr = [], [], [], []
    v0 = f0 = 0
    for obj in objs:
        p = os.path.join(root, "models", f"obj_{int(obj):06d}.ply")
        v = (ply_vtx(p) / unit).astype(np.float32).reshape(-1, 3)
        f = ply_faces(p).astype(np.int32).reshape(-1, 3) if faces else np.zeros((0, 3), np.int32)
        vs.append(v), fs.append(f + v0), vr.append((v0, len(v))), fr.append((f0, len(f)))
        v0, f0 = v0 + len(v), f0 + len(f)
    verts = h2d(torch.from_numpy(np.concatenate(vs).reshape(-1, 3)), device)
    tri = h2d(torch.from_numpy(np.concatenate(fs).reshape(-1, 3).astype(np.int32)), device) if faces else None
    return verts, tri, torch.tensor(vr, dtype=torch.int32).reshape(-1, 2), torch.tensor(fr, dtype=torch.int32).reshape(-1, 2)


def _model_entries(objs: Sequence[int], ext) -> Dict[int, Dict[str, float]]:
    """models.extent's result (metres) as models_info.json entries (millimetres): every number is the f64 metre value
    x 1000.0, and size = max x 1000 - min x 1000."""
    out = {}
    for j, obj in enumerate(objs):
        lo = [float(x) * 1000.0 for x in ext["min"][j].tolist()]
        hi = [float(x) * 1000.0 for x in ext["max"][j].tolist()]
        out[int(obj)] = {"diameter": float(ext["diameter"][j]) * 1000.0, "min_x": lo[0], "min_y": lo[1], "min_z": lo[2],
                         "size_x": hi[0] - lo[0], "size_y": hi[1] - lo[1], "size_z": hi[2] - lo[2]}
    return out


def model_info(root: str, device, objs: Optional[Sequence[int]] = None) -> Dict[int, Dict[str, float]]:
    """The GPU counterpart of BOP's calc_model_info: {obj: {"diameter", "min_x", "min_y", "min_z", "size_x", "size_y",
    "size_z"}} in the files' millimetres, as Python floats, for every models/obj_%06d.ply of `root` (or those named).
    The PLYs are read with dataset.ply_vtx (ASCII only: a binary PLY keeps raising its ValueError), all objects go
    through one models.extent call, concatenated, and the diameter is the maximum over all vertex pairs (no
    subsampling). The numbers describe the vertices that the project renders and scores with, load_models' f32 metres
    (the file's millimetres / 1000), scaled back by 1000 in f64: they agree with the file's own decimals to f32
    rounding (a few 1e-8 of the value)."""
    from . import models
    objs = _model_ids(root) if objs is None else [int(o) for o in objs]
    if not objs:
        return {}
    verts, _, vr, _ = _stage_models(root, objs, device, faces=False)
    return _model_entries(objs, models.extent(verts, vr))


def write_models_info(root: str, device, overwrite: bool = False) -> Dict[int, Dict[str, object]]:
    """Writes models/models_info.json (BOP's format, millimetres) from model_info(root, device): the one file without
    which BopTree does not open a tree. Refuses an existing file unless overwrite=True (FileExistsError, before
    anything is computed); with overwrite=True an existing file's `symmetries_discrete` / `symmetries_continuous` are
    carried over per object, since neither this nor calc_model_info produces them. Returns the written entries."""
    path = os.path.join(root, "models", "models_info.json")
    _refuse(path, overwrite)
    old = _load_json(path) if os.path.exists(path) else {}
    out: Dict[int, Dict[str, object]] = {}
    for obj, e in model_info(root, device).items():
        out[obj] = dict(e)
        for k in ("symmetries_discrete", "symmetries_continuous"):
            if k in old.get(obj, {}):
                out[obj][k] = old[obj][k]
    _save_json(path, out)
    return out


def write_models_eval(root: str, device, n: int = 4096, oversample: int = 4, seed: int = 0, overwrite: bool = False,
                      objs: Optional[Sequence[int]] = None) -> Dict[int, str]:
    """Writes models_eval/obj_%06d.ply for every models/obj_%06d.ply of `root` (or those named): n points drawn
    uniformly on the model's surface with their flat normals (models.sample_surface, thinned by FPS from n x oversample
    candidates), the resampled models that BOP evaluates on. The samples are taken on the file's own f32 vertices, so
    the output is in the model's own unit. Each file is ASCII with `x y z nx ny nz` per vertex and `element face 0`,
    every number printed with 9 significant digits: dataset.ply_vtx reads back the sampled f32 bits. The generator row
    is the object id, so one object written alone gets the same file as in a full write. Refuses an existing file
    unless overwrite=True (FileExistsError, before anything is computed); a model without area raises ValueError
    before anything is written. The PLYs are read with dataset.ply_vtx / ply_faces (ASCII only). Returns {obj: path}."""
    from . import models
    objs = _model_ids(root) if objs is None else [int(o) for o in objs]
    out_dir = os.path.join(root, "models_eval")
    paths = {obj: os.path.join(out_dir, f"obj_{obj:06d}.ply") for obj in objs}
    for path in paths.values():
        _refuse(path, overwrite)
    if not objs:
        return {}
    verts, tri, _, fr = _stage_models(root, objs, device, faces=True, unit=1.0)
    s = models.sample_surface(verts, tri, fr, n, seed=seed, row_id=torch.tensor(objs, dtype=torch.int32),
                              oversample=oversample)
    status = s["status"].cpu().tolist()
    bad = [obj for obj, st in zip(objs, status) if st != 0]
    if bad:
        raise ValueError(f"models without surface area (no faces, or only degenerate ones): {bad}")
    rows = torch.cat([s["points"], s["normals"]], dim=2).cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    for j, obj in enumerate(objs):
        head = ["ply", "format ascii 1.0", "comment surface samples of models/obj_%06d.ply" % obj,
                f"element vertex {n}"] + [f"property float {k}" for k in ("x", "y", "z", "nx", "ny", "nz")] + [
                "element face 0", "property list uchar int vertex_indices", "end_header"]
        with open(paths[obj], "w") as f:
            f.write("\n".join(head) + "\n")
            f.write("".join(" ".join("%.9g" % x for x in row) + "\n" for row in rows[j]))
    return paths


def check_models_info(root: str, device, syms: bool = True) -> Dict[int, Dict[str, object]]:
    """Compares a tree's models/models_info.json with its PLYs, per object that the file lists: {"diameter_file",
    "diameter" (computed as model_info does), "extent_diff": the largest absolute difference of the six min_* / size_*
    numbers, all millimetres} and, with syms=True (which needs the PLYs' faces), {"residual": the list of
    models.symmetry_residual of every member of bop.symmetry_set(...) of the file's entry (the identity first) as a
    fraction of the computed diameter, "worst": the index of the largest}. It reports and does not judge: no
    threshold, nothing raised. An exact symmetry of the mesh gives 0, a symmetry of the shape that the mesh
    approximates about its tessellation's sag, a wrong entry (mm / m mix-up, wrong axis, offset off the axis) a
    sizeable fraction."""
    from . import models
    info = _load_json(os.path.join(root, "models", "models_info.json"))
    objs = sorted(info)
    if not objs:
        return {}
    verts, tri, vr, fr = _stage_models(root, objs, device, faces=syms)
    calc = _model_entries(objs, models.extent(verts, vr))
    out: Dict[int, Dict[str, object]] = {}
    for obj in objs:
        e, c = info[obj], calc[obj]
        out[obj] = {"diameter_file": float(e["diameter"]), "diameter": c["diameter"],
                    "extent_diff": max(abs(float(e[k]) - c[k]) for k in MODEL_KEYS[1:])}
    if syms:
        sets = [bop.symmetry_set(info[o].get("symmetries_discrete"), info[o].get("symmetries_continuous")) for o in objs]
        first = [0] + list(accumulate(len(s) for s in sets))
        sr = torch.tensor([(first[j], len(s)) for j, s in enumerate(sets)], dtype=torch.int32)
        res = models.symmetry_residual(verts, tri, vr, fr, torch.from_numpy(np.concatenate(sets)), sr).tolist()
        for j, obj in enumerate(objs):
            dia_m = out[obj]["diameter"] / 1000.0
            frac = [r / dia_m for r in res[first[j]:first[j + 1]]]
            out[obj]["residual"] = frac
            out[obj]["worst"] = max(range(len(frac)), key=lambda i: frac[i])
    return out


def _row_pose(row):
    """A result row's pose in metres: (R f64 [9] row-major, t f64 [3])."""
    return np.asarray(row["R"], np.float64).reshape(9), np.asarray(row["t"], np.float64).reshape(3) / 1000.0


def _rows_by(rows, width: int, known):
    """Result rows sorted into a tree's keys: ({the first `width` of (scene_id, im_id, obj_id): its rows' indices, in
    order} over the rows whose triple `known` accepts, in order of first appearance; the number of rows it refuses)."""
    by: Dict[tuple, List[int]] = {}
    ignored = 0
    for r, row in enumerate(rows):
        key = (int(row["scene_id"]), int(row["im_id"]), int(row["obj_id"]))
        if known(key):
            by.setdefault(key[:width], []).append(r)
        else:
            ignored += 1
    return by, ignored


def _image_chunks(tree, images, chunk_images: int, device):
    """`images` = [(scene, image)] in chunks of at most chunk_images: per chunk (its images, their depth frames f32
    [n, H, W] on `device`), each frame read once and through read_depth alone (no RGB is decoded)."""
    from .runtime import h2d
    scale = {_key(it)[:2]: float(it["depth_scale"]) for it in tree.instances}
    step = max(1, int(chunk_images))
    for lo in range(0, len(images), step):
        ims = images[lo:lo + step]
        yield ims, h2d(torch.from_numpy(np.stack([
            read_depth(_scene_dir(tree.root, tree.split, sc), im, scale[(sc, im)]) for sc, im in ims])), device)


def _taking_part(n_top: int, n_est: int) -> int:
    """How many of a target's n_est rows take part in the matching: its n_top best, all of them for n_top <= 0."""
    return n_est if n_top <= 0 else min(n_top, n_est)


def result_masks(dataset, rows, device, chunk_images: int = 32, delta: float = bop.DELTA):
    """The visible masks of estimated poses as detection rows: result rows as read_results returns them (t in
    millimetres) become rows in _check_rows' normal form, BOP's detection / segmentation result format, so a pose
    result file yields a segmentation result file, and PoseDataset(layout="bop", detections=...) can crop and mask a
    second pass from a first pass's poses. `dataset` is a PoseDataset(layout="bop", meshes=True).

    Per chunk of at most `chunk_images` distinct images, as in eval_results, the depth frames are read once; the
    chunk's estimates go through bop.visibility under their own poses, 64 at a time, and rle.encode_planes of
    mask_visib brings back the runs alone. Each estimate with a visible pixel gives one _mask_row (the row's ids, score
    and time, bbox = the estimate's bbox_visib, the run list), in the order of `rows`. Returns (rows, {"empty": the
    estimates without a visible pixel (behind the camera, outside the frame, hidden), which give no row, "ignored":
    the rows whose image or object the tree does not hold})."""
    device = torch.device(device)
    tree = dataset.tree
    _require(dataset, "result_masks needs a PoseDataset with layout='bop' and meshes=True", layout=True, meshes=True)
    mesh = dataset._mesh_for(device)
    K4 = {_key(it)[:2]: it["K4"] for it in tree.instances}
    by_image, ignored = _rows_by(rows, 2, lambda k: k[:2] in K4 and k[2] in mesh["range"])
    out: List[Optional[Dict[str, object]]] = [None] * len(rows)
    empty = 0
    for ims, depth in _image_chunks(tree, list(by_image), chunk_images, device):
        H, W = int(depth.shape[1]), int(depth.shape[2])
        est = [(r, f) for f, key in enumerate(ims) for r in by_image[key]]
        for b0 in range(0, len(est), 64):                # write_gt_info's batch: 2 x 64 planes at a time
            part = est[b0:b0 + 64]
            R, t = zip(*(_row_pose(rows[r]) for r, _ in part))
            res = _visibility(mesh["verts"], mesh["faces"], [mesh["range"][int(rows[r]["obj_id"])] for r, _ in part], R, t,
                              [K4[ims[f]] for _, f in part], depth, [f for _, f in part], delta)
            runs = rle.encode_planes(res["mask_visib"])
            info = res["info"].cpu().numpy()
            for j, (r, _) in enumerate(part):
                q = [int(x) for x in info[j]]
                if q[2] == 0:
                    empty += 1
                    continue
                row = rows[r]
                out[r] = _mask_row(row["scene_id"], row["im_id"], row["obj_id"], row["score"], q[7:11], runs[j], (H, W),
                                   row["time"])
    return [e for e in out if e is not None], {"empty": empty, "ignored": ignored}


def write_result_masks(path, dataset, rows, device, chunk_images: int = 32, delta: float = bop.DELTA):
    """result_masks followed by write_detections(path, ...): a pose result file's segmentation result file. Returns
    what result_masks returns."""
    det, stats = result_masks(dataset, rows, device, chunk_images, delta)
    write_detections(path, det)
    return det, stats


def _render_frames(mesh, frames, H: int, W: int):
    """scene.render of per-frame lists of (object, R f64 [9], t f64 [3] metres, K4), each frame's list its instances in
    order, over dataset._mesh_for's `mesh`: (scene.render's result, the instances' objects in the whole list's order)."""
    from . import scene as kscene
    flat = [e for fr in frames for e in fr]
    first = list(accumulate((len(fr) for fr in frames), initial=0))
    res = kscene.render(mesh["verts"], mesh["faces"], [mesh["range"][o] for o, _, _, _ in flat],
                        np.stack([r for _, r, _, _ in flat]) if flat else np.zeros((0, 9)),
                        np.stack([t for _, _, t, _ in flat]) if flat else np.zeros((0, 3)),
                        np.asarray([k for _, _, _, k in flat], np.float32).reshape(-1, 4),
                        [(a, len(fr)) for a, fr in zip(first, frames)], H, W)
    return res, [o for o, _, _, _ in flat]


def vis_results(dataset, rows, out_dir: str, device, gt: bool = True, diff: bool = False, chunk_images: int = 8,
                alpha: int = 128, radius: int = 1, tol: float = 0.02, overwrite: bool = False) -> Dict[str, int]:
    """Pictures of estimated poses on their frames, the counterpart of the BOP toolkit's vis_est_poses: result rows as
    read_results returns them (t in millimetres) are drawn over the RGB image they belong to. `dataset` is a
    PoseDataset(layout="bop", meshes=True).

    Per chunk of at most `chunk_images` distinct images, RGB and depth are read once per image (tree.read_image). Each
    image's rows become its instances, in row order, and scene.render draws them into one z-buffer, one object hiding
    another; scene.overlay blends them over the image, each in scene.palette's colour of its object id, lit by the flat
    shade, with weight alpha / 256 and an outline `radius` pixels wide. With `gt` the image's kept GT instances
    (tree.instances) are rendered as a second scene, and the outlines of its instance map are drawn on top in green.
    With `diff` scene.depth_diff colours the rendered depth against the observed one (metres, so depth_scale = 1.0),
    saturated at `tol`. Only the finished u8 images come back to the host.

    Written with PIL: {out_dir}/{scene:06d}/{im:06d}.png and, with `diff`, {im:06d}_diff.png. An existing file is
    refused unless overwrite=True (FileExistsError, before anything is written). Returns {"images": the images written,
    "drawn": the rows drawn on them, "ignored": the rows whose image or object the tree does not hold}."""
    from PIL import Image
    from . import scene as kscene
    from .runtime import h2d
    device = torch.device(device)
    _require(dataset, "vis_results needs a PoseDataset with layout='bop' and meshes=True", layout=True, meshes=True)
    tree = dataset.tree
    mesh = dataset._mesh_for(device)
    cam = {_key(it)[:2]: (it["K4"], float(it["depth_scale"])) for it in tree.instances}
    by_image, ignored = _rows_by(rows, 2, lambda k: k[:2] in cam and k[2] in mesh["range"])
    images = list(by_image)
    paths = {key: os.path.join(out_dir, f"{key[0]:06d}", f"{key[1]:06d}") for key in images}
    for key in images:
        for suffix in (".png",) + (("_diff.png",) if diff else ()):
            _refuse(paths[key] + suffix, overwrite)
    truth: Dict[Tuple[int, int], List[Dict[str, object]]] = {}
    for it in tree.instances if gt else ():
        truth.setdefault(_key(it)[:2], []).append(it)

    step = max(1, int(chunk_images))
    drawn = 0
    for lo in range(0, len(images), step):
        ims = images[lo:lo + step]
        read = [tree.read_image(sc, im, cam[(sc, im)][1]) for sc, im in ims]
        rgb = h2d(torch.from_numpy(np.stack([r for r, _ in read])), device)
        H, W = int(rgb.shape[1]), int(rgb.shape[2])
        est, objs = _render_frames(mesh, [[(int(rows[r]["obj_id"]), *_row_pose(rows[r]), cam[key][0])
                                            for r in by_image[key]] for key in ims], H, W)
        outline = None
        if gt:
            outline = _render_frames(mesh, [[(int(it["obj"]), np.asarray(it["R"], np.float64).reshape(9),
                                              np.asarray(it["t"], np.float64), it["K4"]) for it in truth.get(key, ())]
                                            for key in ims], H, W)[0]["inst"]
        pics = [kscene.overlay(rgb, est["inst"], est["shade"], kscene.palette(objs), alpha, radius, gt=outline)]
        if diff:
            obs = h2d(torch.from_numpy(np.stack([d for _, d in read])), device)
            pics.append(kscene.depth_diff(est["depth"], obs, 1.0, tol))
        host = [p.cpu().numpy() for p in pics]
        for f, key in enumerate(ims):
            os.makedirs(os.path.dirname(paths[key]), exist_ok=True)
            Image.fromarray(host[0][f]).save(paths[key] + ".png")
            if diff:
                Image.fromarray(host[1][f]).save(paths[key] + "_diff.png")
            drawn += len(by_image[key])
    return {"images": len(images), "drawn": drawn, "ignored": ignored}


def net_mask_rows(rows, runs, info, H: int, W: int):
    """The network's own masks as detection rows (host only): `rows` = result rows as evaluate.result_rows /
    read_results give them, runs[k] = the run list of row k's full-frame H x W mask and info[k] its five ints (pixel
    count, x, y, w, h), as rle.paste_masks and rle.encode_planes return them. Row k gives one _mask_row (the
    row's ids, score and time, bbox = [x, y, w, h] of info, the run list), as result_masks does, in the order of `rows`.
    A row whose pixel count is 0 gives no row. Returns (rows, {"empty": the number of those})."""
    if not len(rows) == len(runs) == len(info):
        raise ValueError(f"{len(rows)} rows, {len(runs)} run lists and {len(info)} info rows: one of each per row")
    out, empty = [], 0
    for row, r, q in zip(rows, runs, info):
        q = [int(v) for v in q]
        if q[0] == 0:
            empty += 1
            continue
        out.append(_mask_row(row["scene_id"], row["im_id"], row["obj_id"], row["score"], q[1:5], [int(v) for v in r],
                             (H, W), row["time"]))
    return out, {"empty": empty}


RESULT_HEADER = "scene_id,im_id,obj_id,score,R,t,time"


def write_results(path: str, rows) -> None:
    """BOP's result CSV, one estimate per row: `rows` = dicts with scene_id, im_id, obj_id, score, R (9 numbers,
    row-major), t (3 numbers, millimetres) and time (seconds, -1 = not measured). Floats are written with repr,
    so read_results returns them bit for bit."""
    with open(path, "w") as f:
        f.write(RESULT_HEADER + "\n")
        for r in rows:
            R = " ".join(repr(float(x)) for x in np.asarray(r["R"], np.float64).reshape(9))
            t = " ".join(repr(float(x)) for x in np.asarray(r["t"], np.float64).reshape(3))
            f.write(f"{int(r['scene_id'])},{int(r['im_id'])},{int(r['obj_id'])},{float(r['score'])!r},{R},{t},"
                    f"{float(r['time'])!r}\n")


def read_results(path: str) -> List[Dict[str, object]]:
    with open(path) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    if not lines or lines[0] != RESULT_HEADER:
        raise ValueError(f"{path}: the first line must be '{RESULT_HEADER}'")
    rows = []
    for n, ln in enumerate(lines[1:], 2):
        tok = ln.split(",")
        if len(tok) != 7:
            raise ValueError(f"{path}:{n}: 7 comma-separated fields expected, got {len(tok)}")
        R, t = np.array(tok[4].split(), np.float64), np.array(tok[5].split(), np.float64)
        if R.size != 9 or t.size != 3:
            raise ValueError(f"{path}:{n}: R holds 9 and t 3 numbers")
        rows.append({"scene_id": int(tok[0]), "im_id": int(tok[1]), "obj_id": int(tok[2]), "score": float(tok[3]),
                     "R": R.reshape(3, 3), "t": t, "time": float(tok[6])})
    return rows


def _rank(scores: Sequence[float]) -> List[int]:
    """Indices by score descending, ties to the lower index, a NaN score as -inf (krrn_bop_match_f64's order)."""
    key = [float("-inf") if s != s else float(s) for s in scores]
    return sorted(range(len(key)), key=lambda i: (-key[i], i))


def _keep_best(rows, idx: List[int], limit: int) -> List[int]:
    """`idx`, indices into `rows`, cut to its `limit` best-scored rows (_rank's order), kept in the order of `idx`."""
    return [idx[a] for a in sorted(_rank([float(rows[r]["score"]) for r in idx])[:limit])]


def _pair_layout(n_a: Sequence[int], n_b: Sequence[int]):
    """The kernels' group layout: (side a's (first, count) ranges, side b's, each n_a x n_b block's offset, pairs)."""
    a0, b0, p0 = (list(accumulate(n, initial=0)) for n in (n_a, n_b, [a * b for a, b in zip(n_a, n_b)]))
    return list(zip(a0, n_a)), list(zip(b0, n_b)), p0[:-1], p0[-1]


def eval_results(dataset, rows, device, chunk_images: int = 32, delta: float = bop.DELTA,
                 taus: Sequence[float] = bop.TAUS) -> Dict[str, object]:
    """Score result rows against a tree the way the BOP-19 protocol does (the toolkit's eval_bop19_pose): per
    (scene, image, object) target the `inst_count` best-scored estimates are greedily matched to the target's GT
    instances, once per error function and threshold of correctness, and recall = matched instances / kept
    instances. `dataset` is a PoseDataset(layout="bop", meshes=True); `rows` are result rows as read_results
    returns them (several per target allowed, t in millimetres).

    The targets are the tree's kept GT instances (BopTree.instances) grouped by (scene, image, object); n_top is
    BopTree.inst_count. Per chunk of at most `chunk_images` distinct images the depth frames are read once, every
    group is expanded into its n_est x n_gt (estimate, instance) pairs, bop.vsd and bop.mssd_mspd give the pairs'
    errors, and bop.match_poses matches every group at the thresholds bop.THETAS (VSD), THETAS x the object's
    diameter (MSSD) and THETAS_PX x width / 640 (MSPD); the matched counts are summed per object as integers on the
    device and read back once at the end. A row whose key is no kept target is ignored and counted in "ignored"; a
    target without rows still counts in the denominator. A target with more than bop.MATCH_MAX rows keeps its
    MATCH_MAX best-scored ones (the kernel's order), one with more instances than that raises ValueError.

    Returns bop.fold_bop's dict with `missed` (AR_VSD, AR_MSSD, AR_MSPD, AR, "count" = the estimates that took part,
    "targets" = the kept instances, "per_obj"), plus "ignored" and "matches": per kept instance, in
    BopTree.instances order, the index in `rows` of the estimate matched to it at the loosest MSSD threshold, or -1.
    Where every target has one instance and one row this equals fold_bop(..., missed=...) on the same poses."""
    from .runtime import h2d
    device = torch.device(device)
    tree = dataset.tree
    _require(dataset, "eval_results needs a PoseDataset with layout='bop' and meshes=True", layout=True, meshes=True)
    mesh = dataset._mesh_for(device)
    T, NT, C = len(taus), len(bop.THETAS), len(taus) + 2
    width = float((tree.frame_hw or (0, bop.FRAME_W))[1])
    groups: Dict[Tuple[int, int, int], List[int]] = {}
    for i, it in enumerate(tree.instances):
        groups.setdefault(_key(it), []).append(i)
    by, ignored = _rows_by(rows, 3, groups.__contains__)
    for key, inst in groups.items():
        if len(inst) > bop.MATCH_MAX:
            raise ValueError(f"target {key} has {len(inst)} kept instances > {bop.MATCH_MAX}")
    est = {k: _keep_best(rows, by.get(k, []), bop.MATCH_MAX) for k in groups}
    take = {k: _taking_part(tree.inst_count[k], len(est[k])) for k in groups}
    objs = list(dict.fromkeys(k[2] for k in groups))
    tp_obj = torch.zeros((max(1, len(objs)), C, NT), dtype=torch.int64, device=device)
    images = list(dict.fromkeys(k[:2] for k in groups))
    th, th_px = np.asarray(bop.THETAS), np.asarray(bop.THETAS_PX)
    pending = []                                             # per chunk: (instance indices, row indices, match column)
    for ims, depth in _image_chunks(tree, images, chunk_images, device):
        frame = {im: f for f, im in enumerate(ims)}
        keys = [k for k in groups if k[:2] in frame]
        er, gr, po, P = _pair_layout([len(est[k]) for k in keys], [len(groups[k]) for k in keys])
        erows, slots = [r for k in keys for r in est[k]], [i for k in keys for i in groups[k]]   # the ranges' rows
        nt, thr, gobj = [], [], []
        Re, te, Rg, tg, K4, fi, fr, vr, sr, dia = [], [], [], [], [], [], [], [], [], []
        for key in keys:
            inst, rws, obj = groups[key], est[key], key[2]
            d = float(tree.info[obj]["diameter"]) / 1000.0
            nt.append(tree.inst_count[key])
            gobj.append(objs.index(obj))
            thr.append(np.stack([th] * T + [np.array([t * d for t in th]), np.array([t * (width / 640.0) for t in th_px])]))
            for r in rws:
                R, t = _row_pose(rows[r])
                for i in inst:
                    it = tree.instances[i]
                    Re.append(R), te.append(t), Rg.append(it["R"].reshape(9)), tg.append(it["t"])
                    K4.append(it["K4"]), fi.append(frame[key[:2]]), dia.append(d)
                    fr.append(mesh["range"][obj]), vr.append(mesh["vrange"][obj]), sr.append(mesh["srange"][obj])
        if P:
            f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))      # noqa: E731
            i32 = lambda a: torch.tensor(a, dtype=torch.int32)               # noqa: E731
            Kt = torch.tensor(K4, dtype=torch.float32)
            pose = (f64(Re), f64(te), f64(Rg), f64(tg))
            v = bop.vsd(mesh["verts"], mesh["faces"], i32(fr), *pose, Kt, depth, i32(fi), f64(dia), 1.0, delta, taus)
            m = bop.mssd_mspd(mesh["verts"], i32(vr), *pose, Kt, mesh["syms"], i32(sr))
            err = torch.cat([v["e_vsd"], m["mssd"][:, None], m["mspd"][:, None]], 1)
        else:
            err = torch.zeros((0, C), dtype=torch.float64, device=device)
        score = torch.tensor([float(rows[r]["score"]) for r in erows], dtype=torch.float64)
        res = bop.match_poses(score, err, torch.tensor(er, dtype=torch.int32), torch.tensor(gr, dtype=torch.int32),
                              torch.tensor(po, dtype=torch.int32), torch.from_numpy(np.stack(thr)),
                              torch.tensor(nt, dtype=torch.int32), len(slots), device)
        tp_obj.index_add_(0, h2d(torch.tensor(gobj, dtype=torch.int64), device), res["tp"].to(torch.int64))
        pending.append((slots, erows, res["match"][:, T, NT - 1]))
    tp = tp_obj.cpu().numpy()                                # the one read-back of the counts
    matches = [-1] * len(tree.instances)
    for slots, erows, col in pending:
        for i, x in zip(slots, col.cpu().tolist()):
            matches[i] = erows[x] if x >= 0 else -1
    n_obj = {o: sum(len(v) for k, v in groups.items() if k[2] == o) for o in objs}
    c_obj = {o: sum(take[k] for k in groups if k[2] == o) for o in objs}
    out: Dict[str, object] = bop.recalls_from_tp(tp[:len(objs)].sum(0), len(tree.instances), sum(take.values()))
    out["per_obj"] = {o: bop.recalls_from_tp(tp[a], n_obj[o], c_obj[o]) for a, o in enumerate(objs)}
    out["ignored"], out["matches"] = ignored, matches
    return out


def _coco_gt(gt) -> Dict[int, Dict[str, object]]:
    """eval_coco's ground truth as {scene: coco dict}: read from the scenes' scene_gt_coco.json for a (root, split)
    pair, passed through for the dict write_gt_coco returns."""
    if isinstance(gt, dict):
        return {int(sc): c for sc, c in gt.items()}
    if not (isinstance(gt, (tuple, list)) and len(gt) == 2):
        raise ValueError("gt must be a (root, split) pair or the {scene: coco dict} that write_gt_coco returns")
    root, split = str(gt[0]), str(gt[1])
    out = {}
    for sc in scene_ids(root, split):
        path = os.path.join(_scene_dir(root, split, sc), "scene_gt_coco.json")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} is missing: write_gt_coco(root, split, device) writes it")
        with open(path) as f:
            out[sc] = json.load(f)
    return out


def eval_coco(gt, rows, device, iou_type: str = "segm", use_ignore: bool = True, chunk_images: int = 32
              ) -> Dict[str, object]:
    """Score a detection or segmentation result file with COCO's average precision, the metric of BOP's 2D
    detection and 2D segmentation tasks (the toolkit's eval_bop22_coco, which takes it from pycocotools). `gt`: a
    (root, split) pair whose scenes' scene_gt_coco.json are read (FileNotFoundError names write_gt_coco when one is
    missing), or the {scene: coco dict} that write_gt_coco returns. `rows`: detection rows in _check_rows' normal form
    (read_detections gives them). iou_type "segm" compares masks (every row must carry a `segmentation` whose `size`
    equals its image's [height, width]: otherwise ValueError with the row's index), "bbox" compares `bbox`.

    A group is one (scene_id, image_id, category_id), so image ids may repeat across scenes; the groups are the
    triples that hold a ground truth or a row, in sorted order. A row whose scene, image or category `gt` does not
    hold is counted in "ignored". A ground truth is ignored where it is a crowd, where its `ignore` is set
    (use_ignore=False drops this clause, which is stock pycocotools; write_gt_coco sets it for visib_fract <
    min_visib), or where its `area` lies outside the area range. A group with more than coco.MATCH_MAX detections
    keeps its MATCH_MAX best-scored ones (the kernel's order), as eval_results does; one with more ground truths than
    that raises ValueError. Per chunk of at most `chunk_images` images: one rle.iou (or rle.box_iou) call over every
    group's n_det x n_gt pairs, whose run lists never become planes, and one coco.match call at coco.IOU_THRS x
    coco.AREA_RNG with maxDet 100. A detection's area is its mask's pixel count (its box's w h for "bbox"), a ground
    truth's its annotation's `area`. Everything is read back once, at the end, and coco.accumulate / coco.summarize
    fold it on the host.

    Returns AP, AP50, AP75, AP_small, AP_medium, AP_large, AR1, AR10, AR100 (-1 where nothing defines one), "per_obj":
    {category: {"AP", "AR100"}}, "count" = the rows that took part, "targets" = the ground-truth annotations,
    "ignored". Written from the published definitions; not checked against pycocotools' own output, which is not a
    dependency."""
    from . import coco as kc
    if iou_type not in ("segm", "bbox"):
        raise ValueError(f"iou_type must be 'segm' or 'bbox', got {iou_type!r}")
    device = torch.device(device)
    segm = iou_type == "segm"
    gts = _coco_gt(gt)
    size: Dict[Tuple[int, int], List[int]] = {}
    cats = sorted({int(c["id"]) for coco in gts.values() for c in coco["categories"]})
    gt_by: Dict[Tuple[int, int, int], List[Dict[str, object]]] = {}
    for sc in sorted(gts):
        for im in gts[sc]["images"]:
            size[(sc, int(im["id"]))] = [int(im["height"]), int(im["width"])]
        for a in gts[sc]["annotations"]:
            gt_by.setdefault((sc, int(a["image_id"]), int(a["category_id"])), []).append(a)
    for key, anns in gt_by.items():
        if len(anns) > kc.MATCH_MAX:
            raise ValueError(f"group {key} has {len(anns)} ground truths > {kc.MATCH_MAX}")
    det_by: Dict[Tuple[int, int, int], List[int]] = {}
    ignored = 0
    for r, row in enumerate(rows):
        key = (int(row["scene_id"]), int(row["image_id"]), int(row["category_id"]))
        seg = row.get("segmentation")
        if segm and seg is None:
            raise ValueError(f"row {r} has no segmentation: iou_type='segm' compares masks")
        if key[:2] not in size or key[2] not in cats:
            ignored += 1
            continue
        if segm and [int(v) for v in seg["size"]] != size[key[:2]]:
            raise ValueError(f"row {r}: segmentation.size {seg['size']} is not its image's {size[key[:2]]}")
        det_by.setdefault(key, []).append(r)
    det_by = {key: _keep_best(rows, rs, kc.MATCH_MAX) for key, rs in det_by.items()}
    keys = sorted(set(gt_by) | set(det_by))
    images = sorted({k[:2] for k in keys})
    step = max(1, int(chunk_images))
    runs_of = lambda seg: rle.counts_from_string(seg["counts"]) if isinstance(seg["counts"], str) else seg["counts"]  # noqa: E731
    cat_of, d_rng, g_rng, scores, pending = [], [], [], [], []
    n_det = n_gt = 0
    for lo in range(0, len(images), step):
        part = set(images[lo:lo + step])
        ck = [k for k in keys if k[:2] in part]
        d_items = [r for k in ck for r in det_by.get(k, [])]
        g_items = [a for k in ck for a in gt_by.get(k, [])]
        D = len(d_items)
        dr, gr, po, _ = _pair_layout([len(det_by.get(k, [])) for k in ck], [len(gt_by.get(k, [])) for k in ck])
        pair = [(d, D + j) for (d0, nd), (g0, ng) in zip(dr, gr) for d in range(d0, d0 + nd) for j in range(g0, g0 + ng)]
        crowd = [int(g_items[j - D].get("iscrowd", 0)) != 0 for _, j in pair]
        for k, (d0, nd), (g0, ng) in zip(ck, dr, gr):
            cat_of.append(cats.index(k[2]))
            d_rng.append((n_det + d0, nd)), g_rng.append((n_gt + g0, ng))
        if segm:
            lists = [rows[r]["segmentation"]["counts"] for r in d_items] + [runs_of(a["segmentation"]) for a in g_items]
            offs = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64)
            res = rle.iou(np.concatenate([np.asarray(c, np.int64) for c in lists]) if lists else np.zeros(0, np.int64),
                          offs, pair, crowd, device)
            det_area = res["area"][:D].to(torch.float64)
        else:
            boxes = [rows[r]["bbox"] for r in d_items] + [a["bbox"] for a in g_items]
            res = rle.box_iou(np.asarray(boxes, np.float64).reshape(-1, 4), pair, crowd, device)
            det_area = res["area"][:D]
        flags = [(1 if int(a.get("iscrowd", 0)) else 0) | (2 if use_ignore and a.get("ignore", False) else 0)
                 for a in g_items]
        sc = np.array([float(rows[r]["score"]) for r in d_items], np.float64)
        m = kc.match(sc, np.array(dr, np.int32).reshape(-1, 2), np.array(gr, np.int32).reshape(-1, 2),
                     np.array(po, np.int32), res["iou"], det_area, np.array([float(a["area"]) for a in g_items], np.float64),
                     np.array(flags, np.int32), device=device)
        scores.append(sc)
        pending.append(m)
        n_det, n_gt = n_det + len(d_items), n_gt + len(g_items)
    A, T = len(kc.AREA_RNG), len(kc.IOU_THRS)
    if pending:                                          # the one read-back: every chunk's outputs as one int32 tensor
        flat = torch.cat([t.reshape(-1).to(torch.int32) for k in ("rank", "dt_match", "dt_ig", "gt_ig") for t in
                          (m[k] for m in pending)]).cpu().numpy()
    else:
        flat = np.zeros(0, np.int32)
    cut = np.cumsum([0, n_det, n_det * A * T, n_det * A * T, n_gt * A])
    rank, dt_match = flat[cut[0]:cut[1]], flat[cut[1]:cut[2]].reshape(n_det, A, T).copy()
    dt_ig, gt_ig = flat[cut[2]:cut[3]].reshape(n_det, A, T), flat[cut[3]:cut[4]].reshape(n_gt, A)
    # dt_match indexes the chunk's ground truths: nothing below needs more than matched or not
    acc = kc.accumulate(cat_of, np.array(d_rng, np.int64).reshape(-1, 2), np.array(g_rng, np.int64).reshape(-1, 2),
                        np.concatenate(scores) if scores else np.zeros(0), rank, dt_match, dt_ig, gt_ig, len(cats))
    out = kc.summarize(acc, cats=cats)
    out["count"], out["targets"], out["ignored"] = n_det, n_gt, ignored
    return out
