"""Micro-bench: rle.iou (krrn_rle_iou_f64) on 64 images x 15 detections x 15 ground truths of disc and ring masks at
480 x 640 (14 400 pairs), beside the composition the tree allowed before it: rle.decode of both sides, then a torch
`&` / sum per pair (one broadcast [15, 15, H W] per image). HIP events, warm-up, the median; the two forms alternate
in one process and their intersections are compared. Prints one JSON line with the times and the bytes each form
moves, computed from the shapes.

    python profiles/bench_coco_iou.py [--reps 30] [--images 64] [--out coco_iou_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from pose_estimation_amd import _lib, rle  # noqa: E402
from pose_estimation_amd.runtime import h2d, ptr, stream_ptr  # noqa: E402

H, W, PER = 480, 640, 15


def _events(fn, reps, warm=5):
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


def _masks(rng, n):
    """n run lists: discs and rings (a disc without a smaller concentric one) scattered over the frame."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        cy, cx, r = rng.uniform(0.3 * H, 0.7 * H), rng.uniform(0.3 * W, 0.7 * W), rng.uniform(40.0, 120.0)
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        m = d2 <= r * r
        if i % 2:
            m &= d2 > (0.5 * r) ** 2
        out.append(rle.encode(m))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n_img = args.images
    rng = np.random.default_rng(0)
    runs = _masks(rng, 2 * PER * n_img)                  # per image: its 15 detections, then its 15 ground truths
    n = len(runs)
    counts = np.concatenate([np.asarray(r, np.int64) for r in runs])
    offs = np.concatenate([[0], np.cumsum([len(r) for r in runs])])
    pair = np.array([(2 * PER * i + d, 2 * PER * i + PER + g) for i in range(n_img) for d in range(PER) for g in range(PER)])
    P = len(pair)
    res = {"images": n_img, "masks": n, "pairs": P, "frame": [H, W], "runs": int(len(counts)),
           "runs_per_mask": float(len(counts)) / n}

    # the run-list form: the whole call (host checks, staging, two launches), and the two launches alone
    res["rle_iou_call_ms"] = _events(lambda: rle.iou(counts, offs, pair, None, dev), args.reps)
    cd, od = h2d(torch.from_numpy(counts.astype(np.int32)), dev), h2d(torch.from_numpy(offs.astype(np.int32)), dev)
    pd = h2d(torch.from_numpy(pair.astype(np.int32)), dev)
    n_ints = ctypes.c_longlong(0)
    _lib.call("krrn_rle_iou_ws", len(counts), ctypes.byref(n_ints))
    ws = torch.empty((n_ints.value,), dtype=torch.int32, device=dev)
    inter = torch.empty((P,), dtype=torch.int32, device=dev)
    iou = torch.empty((P,), dtype=torch.float64, device=dev)
    area = torch.empty((n,), dtype=torch.int32, device=dev)
    launches = lambda: _lib.call("krrn_rle_iou_f64", ptr(cd), len(counts), ptr(od), n, ptr(pd), None, P, ptr(ws),  # noqa: E731
                                 ptr(inter), ptr(iou), ptr(area), stream_ptr(dev))

    # the composition: decode both sides to planes, then per image one broadcast `&` and a sum
    planes = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    inter_c = torch.empty((n_img, PER, PER), dtype=torch.int64, device=dev)

    def decode():
        rle.decode(counts, offs, H, W, dev, out=planes)

    def and_sum():
        flat = planes.view(n_img, 2, PER, H * W)
        for i in range(n_img):
            inter_c[i] = (flat[i, 0][:, None, :] & flat[i, 1][None, :, :]).sum(-1)

    def composition():
        decode()
        and_sum()

    for name, fn in (("rle_iou_launches_ms", launches), ("composition_ms", composition), ("rle_iou_launches_again_ms", launches),
                     ("composition_again_ms", composition), ("decode_ms", decode), ("and_sum_ms", and_sum)):
        res[name] = _events(fn, args.reps)
    launches(), composition()
    torch.cuda.synchronize()
    assert torch.equal(inter.to(torch.int64), inter_c.view(-1)), "the two forms disagree"
    res["inter_sum"] = int(inter.sum())

    # bytes, from the shapes: the scan reads the counts and writes two ints per run; a pair reads both lists' scans at
    # most once (the walked runs, and a search path per walked run end: an upper bound, L2 serves most of it)
    rp = res["runs_per_mask"]
    res["rle_iou_bytes"] = int(len(counts) * 4 * 3 + P * (2 * rp * 4 * 2 + 8 + 4 + 8))
    res["composition_bytes"] = int(len(counts) * 4 * 2 + n * H * W + P * 2 * H * W + P * 8)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
