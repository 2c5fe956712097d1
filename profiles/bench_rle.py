"""Micro-bench: rle.decode (krrn_rle_decode_u8) of 64 disc masks at 480 x 640, beside the host decode it replaces
(numpy np.repeat per mask, then the upload of the 64 planes), and an eval epoch in detection mode beside the same
dataset in PNG mode on a 64-frame 480 x 640 BOP tree (tests/bop_tree.write_twin). HIP events, warm-up, the median.

    python profiles/bench_rle.py [--reps 200] [--frames 64] [--out rle_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bop_tree  # noqa: E402
import rle_ref as rf  # noqa: E402
from pose_estimation_amd import KRRN, bop_scene, make_config, rle  # noqa: E402
from pose_estimation_amd.dataset import PoseDataset  # noqa: E402
from pose_estimation_amd.evaluate import test_epoch  # noqa: E402
from pose_estimation_amd.synthetic import init_weights  # noqa: E402


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
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W, n = 480, 640, 64
    runs = rf.encode(rf.disc(H, W))
    counts, offs = np.tile(np.asarray(runs), n), np.arange(n + 1) * len(runs)
    out = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    res = {"masks": n, "frame": [H, W], "runs_per_mask": len(runs)}
    res["decode_call_ms"] = _events(lambda: rle.decode(counts, offs, H, W, dev, out=out), args.reps)   # checks + staging + launches
    t0 = time.perf_counter()
    for _ in range(5):
        planes = np.stack([rf.decode(runs, H, W) for _ in range(n)])
    res["host_decode_ms"] = (time.perf_counter() - t0) / 5 * 1e3
    pinned = torch.from_numpy(planes).pin_memory()
    res["upload_ms"] = _events(lambda: out.copy_(pinned, non_blocking=True), args.reps)
    assert np.array_equal(rle.decode(counts, offs, H, W, dev)["mask"].cpu().numpy(), planes)

    with tempfile.TemporaryDirectory() as d:
        bop_tree.write_twin(os.path.join(d, "lm"), os.path.join(d, "bop"), frames=args.frames)
        mk = lambda **kw: PoseDataset("test", 500, False, os.path.join(d, "bop"), 0.0, 8, cls_type="cat",  # noqa: E731
                                      n_model_pts=150, layout="bop", meshes=True, **kw)
        rows = bop_scene.gt_detections(mk().tree)
        model = KRRN(cfg=make_config(num_cls=1, backbone="w18"))
        init_weights(model, 0)
        model = model.to(dev).eval()
        for name, kw in (("png", {}), ("detections", {"detections": rows})):
            ds = mk(**kw)
            times = []
            for _ in range(5):                           # the first two warm the plans up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out_ep = test_epoch(model, ds, bs=64, device=dev)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            res[f"epoch_{name}_crops_per_s"] = out_ep["test_count"] / float(np.median(times[2:]))
            res[f"epoch_{name}_s"] = times
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
