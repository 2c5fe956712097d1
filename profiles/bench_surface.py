"""One wall-clock measurement of bop_scene.write_models_eval (pose_estimation_amd/models.sample_surface underneath) on the
largest mesh at hand, the torus of profiles/bench_models.py (20 000 vertices / 40 000 faces), written as a one-model
tree in a temporary folder: reading the PLY, staging it, the draw of n x oversample candidates, the FPS thinning, the
read-back and the ASCII file, end to end, the first and only call of the process (so code-object loading is inside).
Beside it the second call of models.sample_surface alone on the staged mesh (host clock around a synchronise). One run
each: model preparation happens once per tree, and no speed claim rests on these numbers.

usage (GPU box):  python3 profiles/bench_surface.py [--out profiles/surface_eval.txt] [--n 4096] [--oversample 4]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_models import torus  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--oversample", type=int, default=4)
    args = ap.parse_args()
    import torch
    from pose_estimation_amd import bop_scene, models
    dev = torch.device("cuda", 0)
    v, f = torus()
    prop = torch.cuda.get_device_properties(0)
    out = {"kernels": ["krrn_surface_sample_f64", "krrn_fps_f32", "krrn_gather_rows_f32"],
           "box": {"gpu": torch.cuda.get_device_name(0), "arch": prop.gcnArchName, "cus": prop.multi_processor_count,
                   "torch": torch.__version__, "hip": torch.version.hip},
           "mesh": {"verts": len(v), "faces": len(f)}, "n": args.n, "oversample": args.oversample}
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "models"))
        with open(os.path.join(root, "models", "obj_000001.ply"), "w") as fh:
            fh.write(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\n"
                     f"property float z\nelement face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
            fh.write("".join("%.4f %.4f %.4f\n" % tuple(p) for p in v.astype(np.float64) * 1000.0))
            fh.write("".join("3 %d %d %d\n" % tuple(t) for t in f))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        paths = bop_scene.write_models_eval(root, dev, n=args.n, oversample=args.oversample)
        out["write_models_eval_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["file_bytes"] = os.path.getsize(paths[1])
        mm = np.loadtxt(paths[1], skiprows=13)[:, :3]
    # the samples lie on the torus (R = 80 mm, r = 30 mm) up to the tessellation's sag
    rho = np.hypot(np.hypot(mm[:, 0], mm[:, 1]) - 80.0, mm[:, 2])
    out["tube_radius_mm_min_max"] = [round(float(rho.min()), 4), round(float(rho.max()), 4)]
    vd, fd = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    fr = torch.tensor([[0, len(f)]], dtype=torch.int32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = models.sample_surface(vd, fd, fr, args.n, row_id=[1], oversample=args.oversample)
    torch.cuda.synchronize()
    out["sample_surface_second_call_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["area_m2"] = float(s["area"][0])
    out["area_torus_m2"] = 4 * np.pi ** 2 * 0.08 * 0.03
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("python3 profiles/bench_surface.py --n %d --oversample %d\n" % (args.n, args.oversample)
                     + json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
