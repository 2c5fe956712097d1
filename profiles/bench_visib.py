"""Micro-bench: GT visibility (krrn_bop_visib_u8) beside VSD (krrn_bop_vsd_f32) on profiles/bench_bop.py's inputs:
B = 64 instances of an icosphere of 20480 faces (radius 7 cm at about 0.8 m: about 100 px across a 640 x 480 frame),
random GT poses, VSD's estimates a few degrees / millimetres away, one observed frame per instance. HIP-event time
per call, warm-up first, median of 5 groups of 10 (bench_raster.timed), the three timed in alternating rounds:
  visib_planes     krrn_bop_visib_u8 writing mask and mask_visib (2 x 307 KB per instance, after two memsets)
  visib_no_planes  krrn_bop_visib_u8 with both planes NULL (counts, boxes and visib_fract only)
  vsd              krrn_bop_vsd_f32 (two renders per instance, nothing written)
and bop_scene.write_gt_info over a BOP tree holding the tiny test tree's shapes (tests/bop_scene_ref.py: three
instances per image of a tetrahedron and two icospheres) scaled to 640 x 480 frames, in images per second with and
without the PNGs. Plain timing, no counters.

usage (GPU box):  python3 profiles/bench_visib.py [--out profiles/visib.json] [--images 32]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_raster import timed  # noqa: E402

B, SUBDIV, RADIUS = 64, 5, 0.07


def kernels(dev, rounds=3):
    import torch
    import bop_ref as br
    import raster_ref as rr
    from pose_estimation_amd import _lib, bop
    from pose_estimation_amd.runtime import P, ptr
    rng = np.random.default_rng(0)
    v, f = rr.icosphere(SUBDIV, RADIUS)
    v = v.astype(np.float32)
    R_gt = np.stack([rr.rotation(rng) for _ in range(B)])
    cen = np.stack([rng.uniform(100, rr.W - 100, B), rng.uniform(100, rr.H - 100, B)], 1)
    t_gt = np.stack([rr._centre_t(rng.uniform(0.75, 0.85), c[0], c[1]) for c in cen])
    est = [br.perturbed(rng, R_gt[b], t_gt[b]) for b in range(B)]
    R_est, t_est = np.stack([e[0] for e in est]), np.stack([e[1] for e in est])
    tt = torch.from_numpy
    verts, faces = tt(v).to(dev), tt(f).to(dev)
    fr = torch.tensor([[0, len(f)]] * B, dtype=torch.int32, device=dev)
    Re, te, Rg, tg = (tt(a).reshape(B, -1).to(dev) for a in (R_est, t_est, R_gt, t_gt))
    K4 = torch.tensor([rr.LM_K4] * B, dtype=torch.float32, device=dev)
    frame = torch.arange(B, dtype=torch.int32, device=dev)
    # observed frames: the GT silhouette's own depth (from a first visibility call over an empty observation: its
    # mask, at the instance's centre depth) over a 1.5 m background, 2 % holes (metres)
    empty = torch.zeros((B, rr.H, rr.W), dtype=torch.float32, device=dev)
    sil = bop.visibility(verts, faces, fr, Rg, tg, K4, empty, frame)["mask"].bool()
    depth = torch.where(sil, tg.reshape(B, 3)[:, 2].float().view(B, 1, 1).expand(B, rr.H, rr.W), torch.full_like(empty, 1.5))
    depth[torch.rand((B, rr.H, rr.W), device=dev) < 0.02] = 0.0
    depth = depth.contiguous()
    dia = torch.full((B,), 2 * RADIUS, dtype=torch.float64, device=dev)
    taus = torch.tensor(bop.TAUS, dtype=torch.float64, device=dev)
    T = len(bop.TAUS)
    ws = torch.empty((B, 8), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 2 + T), dtype=torch.int32, device=dev)
    e_vsd = torch.empty((B, T), dtype=torch.float64, device=dev)
    vws = torch.empty((B, bop.VISIB_WS), dtype=torch.int32, device=dev)
    mask = torch.empty((B, rr.H, rr.W), dtype=torch.uint8, device=dev)
    mvis = torch.empty((B, rr.H, rr.W), dtype=torch.uint8, device=dev)
    info = torch.empty((B, 11), dtype=torch.int32, device=dev)
    fract = torch.empty((B,), dtype=torch.float64, device=dev)
    st = P(torch.cuda.current_stream(dev).cuda_stream)

    def vsd():
        _lib.call("krrn_bop_vsd_f32", ptr(verts), verts.shape[0], ptr(faces), faces.shape[0], ptr(fr), ptr(Re), ptr(te),
                  ptr(Rg), ptr(tg), ptr(K4), ptr(depth), B, rr.H, rr.W, ptr(frame), 1.0, ptr(dia), bop.DELTA, ptr(taus), T,
                  B, ptr(ws), ptr(counts), ptr(e_vsd), st)

    def visib(m, mv):
        _lib.call("krrn_bop_visib_u8", ptr(verts), verts.shape[0], ptr(faces), faces.shape[0], ptr(fr), ptr(Rg), ptr(tg),
                  ptr(K4), ptr(depth), B, rr.H, rr.W, ptr(frame), 1.0, bop.DELTA, B, ptr(vws), ptr(m), ptr(mv), ptr(info),
                  ptr(fract), st)

    fns = {"visib_planes": lambda: visib(mask, mvis), "visib_no_planes": lambda: visib(None, None), "vsd": vsd}
    out = {k: [] for k in fns}
    for _ in range(rounds):                   # alternating: other people's work shares the machine
        for k, fn in fns.items():
            out[k].append(timed(fn))
    fns["visib_planes"]()
    torch.cuda.synchronize()
    res = {k: {"ms_median_per_round": [r["ms_median"] for r in v], "ms_median": float(np.median([r["ms_median"] for r in v])),
               "ms_min": min(r["ms_min"] for r in v), "ms_max": max(r["ms_max"] for r in v)} for k, v in out.items()}
    res["px_count_all_mean"] = float(info[:, 0].double().mean())
    res["visib_fract_mean"] = float(fract.mean())
    res["plane_bytes_per_call"] = 2 * B * rr.H * rr.W
    return res


def gt_info(dev, images, reps=3):
    """write_gt_info on `images` 640 x 480 images of the tiny test tree's shapes (K and pixel positions x 10)."""
    import torch
    from PIL import Image
    import bop_scene_ref as sr
    import bop_tree
    import raster_ref as rr
    from pose_estimation_amd import bop_scene
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as root:
        bop_tree.write_models(root)
        sdir = os.path.join(root, "test", "000001")
        os.makedirs(os.path.join(sdir, "depth"))
        gt, cam = {}, {}
        lay = [l for name in sr.IMAGES for l in sr._LAYOUT[name][6] if l[0] != "norange"]
        fx, fy, cx, cy = (float(k) for k in rr.LM_K4)
        for im in range(images):
            gt[str(im)] = []
            for k in range(3):
                _, obj, z, col, row, _ = lay[(3 * im + k) % len(lay)]
                t = rr._centre_t(z, 10.0 * col + rng.uniform(-20, 20), 10.0 * row + rng.uniform(-20, 20))
                gt[str(im)].append({"cam_R_m2c": [float(x) for x in rr.rotation(rng).reshape(-1)],
                                    "cam_t_m2c": [float(x) * 1000.0 for x in t], "obj_id": obj})
            cam[str(im)] = {"cam_K": [fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0], "depth_scale": 1.0}
            d = np.full((rr.H, rr.W), 1000, np.uint16)          # a plane at 1 m: in front of some, behind others
            d[rng.random(d.shape) < 0.02] = 0
            Image.fromarray(d).save(os.path.join(sdir, "depth", f"{im:06d}.png"))
        for name, c in (("scene_gt.json", gt), ("scene_camera.json", cam)):
            with open(os.path.join(sdir, name), "w") as fh:
                json.dump(c, fh)
        out = {"images": images, "instances_per_image": 3, "frame": [rr.H, rr.W]}
        for masks in (False, True):
            rates = []
            for rep in range(reps + 1):       # the first run warms up and is dropped
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bop_scene.write_gt_info(root, "test", dev, masks=masks, overwrite=True)
                torch.cuda.synchronize()
                if rep:
                    rates.append(images / (time.perf_counter() - t0))
            out["images_per_s_with_pngs" if masks else "images_per_s_json_only"] = [round(r, 1) for r in rates]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--images", type=int, default=32)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    result = {"kernels": ["krrn_bop_visib_u8", "krrn_bop_vsd_f32"], "B": B, "faces": 20 * 4 ** SUBDIV,
              "box": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
                      "cus": torch.cuda.get_device_properties(0).multi_processor_count, "torch": torch.__version__,
                      "hip": torch.version.hip}}
    result.update(kernels(dev))
    print(json.dumps(result), flush=True)
    if args.images:
        result["write_gt_info"] = gt_info(dev, args.images)
        print(json.dumps(result["write_gt_info"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
