"""Micro-bench of the model-info kernels (pose_estimation_amd/models.py), at sizes a scanned object model has:
  extent            krrn_model_extent_f64 on one object of 20 000 and one of 200 000 random vertices
  extent_host       the same 20 000-vertex diameter by a chunked numpy brute force on this machine's host (wall clock,
                    one run after a warm-up chunk); it must give the same d2, bit for bit
  residual          krrn_symmetry_residual_f64 on a torus mesh of 20 000 vertices / 40 000 faces with 1 symmetry and
                    with the 315 of a continuous axis
Device events around each call after a warm-up, the median of --runs runs (default 10). Plain timing, no counters.

usage (GPU box):  python3 profiles/bench_models.py [--out profiles/models_extent.txt] [--runs 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, runs, warm=2):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "runs": runs}


def host_d2(v, chunk=256):
    """The restatement's pair walk (tests/models_ref.py), chunked over the rows."""
    x = v.astype(np.float64)
    best = 0.0
    for i in range(0, len(x), chunk):
        dx = x[i:i + chunk, None, 0] - x[None, :, 0]
        dy = x[i:i + chunk, None, 1] - x[None, :, 1]
        dz = x[i:i + chunk, None, 2] - x[None, :, 2]
        best = max(best, float(((dx * dx + dy * dy) + dz * dz).max()))
    return best


def torus(n=100, m=200, R=0.08, r=0.03):
    """n x m vertices, 2 n m faces, closed: every vertex is a corner of six faces."""
    u, w = np.meshgrid(np.arange(n) * 2 * np.pi / n, np.arange(m) * 2 * np.pi / m, indexing="ij")
    v = np.stack([(R + r * np.cos(u)) * np.cos(w), (R + r * np.cos(u)) * np.sin(w), r * np.sin(u)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    a, b, c, d = i * m + j, ((i + 1) % n) * m + j, ((i + 1) % n) * m + (j + 1) % m, i * m + (j + 1) % m
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v.astype(np.float32), f.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--runs", type=int, default=10)
    args = ap.parse_args()
    import torch
    from pose_estimation_amd import _lib, bop
    from pose_estimation_amd.runtime import P, ptr
    dev = torch.device("cuda", 0)
    st = P(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(0)
    prop = torch.cuda.get_device_properties(0)
    out = {"kernels": ["krrn_model_extent_f64", "krrn_symmetry_residual_f64"],
           "box": {"gpu": torch.cuda.get_device_name(0), "arch": prop.gcnArchName, "cus": prop.multi_processor_count,
                   "torch": torch.__version__, "hip": torch.version.hip}}
    d2 = torch.empty(1, dtype=torch.float64, device=dev)
    box = torch.empty((1, 6), dtype=torch.float64, device=dev)
    for n in (20000, 200000):
        v = rng.normal(size=(n, 3)).astype(np.float32)
        vd = torch.from_numpy(v).to(dev)
        vr = torch.tensor([[0, n]], dtype=torch.int32, device=dev)
        out[f"extent_{n}"] = timed(lambda: _lib.call("krrn_model_extent_f64", ptr(vd), n, ptr(vr), 1, n, ptr(d2), ptr(box), st),
                                   args.runs)
        out[f"extent_{n}"]["d2"] = float(d2.cpu()[0])
        if n == 20000:
            host_d2(v[:2048])
            t0 = time.perf_counter()
            h = host_d2(v)
            out["extent_host_20000"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "d2": h,
                                        "same_bits_as_device": h == out[f"extent_{n}"]["d2"]}
        print(json.dumps({k: out[k] for k in out if k.startswith("extent")}), flush=True)
    v, f = torus()
    vd, fd = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    vr = torch.tensor([[0, len(v)]], dtype=torch.int32, device=dev)
    fr = torch.tensor([[0, len(f)]], dtype=torch.int32, device=dev)
    for name, S in (("residual_ns1", bop.symmetry_set()),
                    ("residual_ns315", bop.symmetry_set(continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}]))):
        sy = torch.from_numpy(S).to(dev)
        sr = torch.tensor([[0, len(S)]], dtype=torch.int32, device=dev)
        res2 = torch.empty(len(S), dtype=torch.float64, device=dev)
        out[name] = timed(lambda: _lib.call("krrn_symmetry_residual_f64", ptr(vd), len(v), ptr(fd), len(f), ptr(vr), ptr(fr),
                                            ptr(sy), len(S), ptr(sr), 1, len(v), len(f), ptr(res2), st), args.runs, warm=1)
        r = res2.cpu().numpy()
        out[name].update({"verts": len(v), "faces": len(f), "symmetries": len(S),
                          "worst_residual_over_diameter": float(np.sqrt(r.max()) / 0.22)})
        print(json.dumps({name: out[name]}), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("python3 profiles/bench_models.py --runs %d\n" % args.runs + json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
