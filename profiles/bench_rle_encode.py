"""Micro-bench: run lists of 64 visibility planes at 480 x 640, the two ways. The planes come from bop.visibility (an
icosphere of 5 cm radius under 64 poses spread over the frame, 0.35 .. 0.9 m away, against a wall at 1.2 m). The
former path reads the planes back whole and runs the host's rle.encode on each; rle.encode_planes encodes on the GPU
(krrn_rle_encode_u8) and reads back the runs. Host clock around work that ends in a read-back, and HIP events around
encode_gpu alone (the three kernels and the binding's allocations); warm-up, the median, min and max.

    python profiles/bench_rle_encode.py [--reps 50] [--out rle_encode_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import raster_ref as rr  # noqa: E402
from pose_estimation_amd import bop, rle  # noqa: E402


def _stats(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def _host(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                             # ends in a read-back
        ms.append((time.perf_counter() - t0) * 1e3)
    return _stats(ms)


def _events(fn, reps, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return _stats(ms)


def planes(dev, n=64, H=480, W=640, seed=0):
    rng = np.random.default_rng(seed)
    v, f = rr.icosphere(2, 0.05)
    R = np.stack([rr.rotation(rng) for _ in range(n)])
    t = np.stack([rr._centre_t(rng.uniform(0.35, 0.9), rng.uniform(60, W - 60), rng.uniform(60, H - 60)) for _ in range(n)])
    depth = torch.full((1, H, W), 1.2, dtype=torch.float32, device=dev)
    res = bop.visibility(torch.from_numpy(v.astype(np.float32)).to(dev), torch.from_numpy(f).to(dev),
                         torch.tensor([[0, len(f)]] * n, dtype=torch.int32), torch.from_numpy(R), torch.from_numpy(t),
                         torch.tensor([rr.LM_K4] * n, dtype=torch.float32), depth, torch.zeros(n, dtype=torch.int32))
    return res["mask_visib"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m = planes(dev)
    n, H, W = m.shape
    want = [rle.encode(p) for p in m.cpu().numpy()]
    assert rle.encode_planes(m) == want
    res = {"masks": n, "frame": [H, W], "runs_per_mask": float(np.mean([len(r) for r in want])),
           "pixels_per_mask": float(m.sum().item()) / n, "plane_bytes": n * H * W,
           "run_bytes": 4 * n * max(len(r) for r in want)}
    res["readback_ms"] = _host(lambda: m.cpu(), args.reps)
    res["host_path_ms"] = _host(lambda: [rle.encode(p) for p in m.cpu().numpy()], args.reps)
    res["encode_planes_ms"] = _host(lambda: rle.encode_planes(m), args.reps)
    res["encode_gpu_ms"] = _events(lambda: rle.encode_gpu(m), args.reps * 4)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
