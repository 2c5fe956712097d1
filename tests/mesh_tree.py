"""Writes a small LineMOD-layout tree like tests/linemod_tree.py whose models/obj_XX.ply carry faces
(icospheres), so that PoseDataset(gt_maps=True) can render the GT maps. The depth and mask images are
rendered from the same mesh and pose by the numpy rasteriser (tests/raster_ref.py): object depth over a
1.5 m background with a few sensor holes; the label mask is the coverage minus the object's top three
rows, so that label, depth and coverage all differ."""
import os

import numpy as np
import yaml
from PIL import Image

import raster_ref as rr

RADIUS = 0.03          # metres; 17 px at 1 m (crop size 40), 34 px at 0.5 m (crop size 80)
SUBDIV = 2             # 320 faces, 162 vertices
WIN = 120              # the square window the object is rendered into (it fits at either depth)


def write_tree(root, objs=(6, 2), per_obj=(3, 3), depths=(1.0, 0.5, 1.0), seed=0, subdiv=SUBDIV):
    """per_obj[k] frames for objs[k], frame f at depth depths[f % len(depths)]. Returns {"mesh": {obj: (verts f32
    [V, 3] metres as the loader reads them, faces int32 [F, 3])}, (obj, im_id): {"R", "t", "cover", "depth_mm",
    "mask", "bbox"}}."""
    rng = np.random.default_rng(seed)
    written = {"mesh": {}}
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    for k, obj in enumerate(objs):
        v, f = rr.icosphere(subdiv, RADIUS)
        v = v * (1.0 + 0.005 * k)                       # every object its own size (all snap to crops of 40 / 80)
        lines = [f"{a:.4f} {b:.4f} {c:.4f}" for a, b, c in v * 1000.0]
        with open(os.path.join(root, "models", f"obj_{obj:02d}.ply"), "w") as fh:
            fh.write(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\n"
                     f"property float z\nelement face {len(f)}\nproperty list uchar int vertex_indices\n"
                     "property uchar red\nend_header\n")
            fh.write("\n".join(lines) + "\n")
            fh.write("".join(f"3 {a} {b} {c} 255\n" for a, b, c in f))
        vm = np.array([np.float32(ln.split()) for ln in lines], dtype=np.float32) / 1000.0  # dataset.ply_vtx / 1000
        written["mesh"][obj] = (vm, f.copy())
        croot = os.path.join(root, "data", f"{obj:02d}")
        for sub in ("rgb", "depth", "mask"):
            os.makedirs(os.path.join(croot, sub), exist_ok=True)
        ids = [3 * i + 1 for i in range(per_obj[k])]
        meta = {}
        for fi, im in enumerate(ids):
            z = depths[fi % len(depths)]
            col, row = rng.uniform(80, rr.W - 80), rng.uniform(80, rr.H - 80)
            R, t = rr.rotation(rng), rr._centre_t(z, col, row)
            rmin, cmin = int(row) - WIN // 2, int(col) - WIN // 2
            res = rr.render(vm, f, R, t, rr.LM_K4, rmin, cmin, WIN, vm[:1], margins=False)
            cover = np.zeros((rr.H, rr.W), bool)
            cover[rmin:rmin + WIN, cmin:cmin + WIN] = res["cover"]
            depth = np.full((rr.H, rr.W), 1.5)
            depth[rmin:rmin + WIN, cmin:cmin + WIN] = np.where(res["cover"], res["depth"], 1.5)
            depth[rng.random((rr.H, rr.W)) < 0.02] = 0.0
            dmm = np.round(depth * 1000.0).astype(np.uint16)
            ys, xs = np.nonzero(cover)
            label = cover.copy()
            label[:ys.min() + 3] = False
            m = (label * 255).astype(np.uint8)
            rgb = rng.integers(0, 256, size=(rr.H, rr.W, 3), dtype=np.uint8)
            Image.fromarray(rgb).save(os.path.join(croot, "rgb", f"{im:04d}.png"))
            Image.fromarray(dmm).save(os.path.join(croot, "depth", f"{im:04d}.png"))
            Image.fromarray(np.stack([m, m, m], -1)).save(os.path.join(croot, "mask", f"{im:04d}.png"))
            bbox = [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]
            entry = {"cam_R_m2c": [float(x) for x in R.reshape(-1)], "cam_t_m2c": [float(x) * 1000.0 for x in t],
                     "obj_bb": bbox, "obj_id": obj}
            meta[im] = ([{"cam_R_m2c": [1.0, 0, 0, 0, 1, 0, 0, 0, 1], "cam_t_m2c": [0.0, 0.0, 1.0],
                          "obj_bb": [0, 0, 10, 10], "obj_id": 5}] if obj == 2 else []) + [entry]
            written[(obj, im)] = {"R": R, "t": t, "cover": cover, "depth_mm": dmm, "mask": m, "bbox": bbox}
        with open(os.path.join(croot, "gt.yml"), "w") as fh:
            yaml.safe_dump(meta, fh)
        with open(os.path.join(croot, "test.txt"), "w") as fh:
            fh.write("".join(f"{im:04d}\n" for im in ids))
    return written
