"""A tiny BOP tree that holds objects several times in one image, for the multi-instance matching tests, built from
tests/bop_scene_ref.py's meshes and camera and tests/bop_ref.py's helpers (not a test).

write_tree: scene 1, frames of 48 x 64, camera K_TINY, depth_scale 1.0.
  image 0   object 2 (the small icosphere, declared symmetric about z) three times and object 3 (the larger one)
            twice, side by side: five instances, two targets with inst_count 3 and 2
  image 1   object 3 once and object 1 (the tetrahedron) once
The observed depth is bop_ref.observed of the nearest surface (no occluding plane), quantised to millimetres;
scene_gt_info.json and the mask PNGs come from bop_scene_ref.visibility. Also a test_targets_bop19.json.

result_rows: result rows (t in millimetres) for that tree. Every instance of image 0 but the second of object 3
and the object-3 instance of image 1 get their GT pose perturbed by bop_ref.perturbed; the first instance of
object 2 gets a second, near-duplicate estimate (four rows for a target of three: the lowest-scored does not take
part); object 3 of image 0 gets one gross pose in place of its second instance's estimate; one row names a target the
tree does not hold; target (1, 1, 1) gets no row."""
import os

import numpy as np
from PIL import Image

import bop_ref as br
import bop_scene_ref as sr
import bop_tree
import raster_ref as rr

H, W = sr.H, sr.W
# image id: [(obj, z, col, row)]
LAYOUT = {0: [(2, 1.00, 10.3, 11.6), (3, 1.05, 19.7, 34.2), (2, 0.95, 32.4, 12.3), (3, 1.10, 47.2, 33.6),
              (2, 1.05, 54.1, 11.8)],
          1: [(3, 0.90, 20.4, 24.7), (1, 0.50, 45.3, 22.8)]}


def write_tree(root, split="test", seed=21):
    """Returns {"inst": [(scene, im, gt index, obj, R, t)], "targets": the list's path}."""
    rng = np.random.default_rng(seed)
    bop_tree.write_models(root, (2,))
    K4 = np.asarray(sr.K_TINY, np.float32)
    fx, fy, cx, cy = (float(k) for k in K4)
    sdir = os.path.join(root, split, "000001")
    for sub in ("rgb", "depth", "mask", "mask_visib"):
        os.makedirs(os.path.join(sdir, sub), exist_ok=True)
    gt, cam, ginfo, targets, out = {}, {}, {}, [], []
    for im_id, layout in LAYOUT.items():
        inst, nearest = [], np.zeros((H, W))
        for obj, z, col, row in layout:
            v, f = sr.meshes()[obj]
            R = rr._small_rot(rng) if obj == 1 else rr.rotation(rng)
            t = rr._centre_t(z, col, row, K4=[float(k) for k in K4])
            inst.append((obj, v, f, np.asarray(R, np.float64), np.asarray(t, np.float64)))
            d, _ = br.depth_image(v, f, R, t, K4, H, W)
            nearest = np.where((d > 0.0) & ((nearest == 0.0) | (d < nearest)), d, nearest)
        raw = np.round(br.observed(nearest, rng, occlude=False).astype(np.float64)).astype(np.uint16)
        depth = (raw.astype(np.float64) / 1000.0).astype(np.float32)
        Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(os.path.join(sdir, "rgb", f"{im_id:06d}.png"))
        Image.fromarray(raw).save(os.path.join(sdir, "depth", f"{im_id:06d}.png"))
        cam[str(im_id)] = {"cam_K": [fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0], "depth_scale": 1.0}
        gt[str(im_id)], ginfo[str(im_id)] = [], []
        for g, (obj, v, f, R, t) in enumerate(inst):
            res = sr.visibility(v, f, R, t, K4, depth)
            sr.check_conditions(res)
            gt[str(im_id)].append({"cam_R_m2c": [float(x) for x in R.reshape(-1)], "cam_t_m2c": [float(x) * 1000.0 for x in t],
                                   "obj_id": int(obj)})
            ginfo[str(im_id)].append(bop_tree.info_entry(res))
            for sub in ("mask", "mask_visib"):
                Image.fromarray(res[sub].astype(np.uint8) * np.uint8(255)).save(
                    os.path.join(sdir, sub, f"{im_id:06d}_{g:06d}.png"))
            out.append((1, im_id, g, int(obj), R, t))
        for obj in sorted({i[0] for i in inst}):
            targets.append({"scene_id": 1, "im_id": im_id, "obj_id": int(obj), "inst_count": sum(1 for i in inst if i[0] == obj)})
    bop_tree._dump(os.path.join(sdir, "scene_gt.json"), gt)
    bop_tree._dump(os.path.join(sdir, "scene_camera.json"), cam)
    bop_tree._dump(os.path.join(sdir, "scene_gt_info.json"), ginfo)
    path = os.path.join(root, "test_targets_bop19.json")
    bop_tree._dump(path, targets)
    return {"inst": out, "targets": path}


def result_rows(made, seed=4):
    """(rows, {"dup": the two row indices aimed at one instance, "gross": the gross row's index, "unknown": the index
    of the row without a target, "bare": the key of the target without rows})."""
    rng = np.random.default_rng(seed)
    inst = {(im, g): (obj, R, t) for _, im, g, obj, R, t in made["inst"]}

    def row(im, obj, score, R, t):
        return {"scene_id": 1, "im_id": im, "obj_id": obj, "score": float(score), "R": np.asarray(R, np.float64).reshape(3, 3),
                "t": np.asarray(t, np.float64) * 1000.0, "time": -1.0}

    def near(im, g, score):
        obj, R, t = inst[(im, g)]
        return row(im, obj, score, *br.perturbed(rng, R, t))

    K4 = [float(k) for k in sr.K_TINY]
    rows = [near(0, 0, 0.8),                             # 0  object 2, instance 0
            near(0, 1, 0.7),                             # 1  object 3, instance 1
            near(0, 2, 0.9),                             # 2  object 2, instance 2
            row(0, 3, 0.6, rr.rotation(rng), rr._centre_t(0.8, 40.3, 8.6, K4=K4)),   # 3  gross, object 3
            near(0, 4, 0.5),                             # 4  object 2, instance 4
            near(0, 0, 0.85),                            # 5  the near-duplicate of row 0
            row(3, 2, 0.99, np.eye(3), [0.0, 0.0, 1.0]),  # 6  image 3 does not exist
            near(1, 0, 0.4)]                             # 7  object 3 of image 1; nothing for (1, 1, 1)
    return rows, {"dup": (0, 5), "gross": 3, "unknown": 6, "bare": (1, 1, 1)}
