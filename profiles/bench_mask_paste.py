"""Micro-bench: krrn_mask_paste_f32 at B = 64 crops of S = 120, C1 = 2, into 480 x 640 planes, and krrn_rle_encode_u8
on the same planes beside it for scale. The logits are a disc of foreground per crop under noise (so the masks have an
object's shape and a ragged edge), cut from a wider tensor as pred["mask"] is; windows are spread over the frame, some
cut by a border. HIP events around rle.paste_masks with device-side chan / rc (two launches and the binding's two
allocations) and around rle.encode_gpu (three launches, four allocations); warm-up, the median, min and max.

    python profiles/bench_mask_paste.py [--reps 200] [--out mask_paste_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import paste_ref as pr  # noqa: E402
from pose_estimation_amd import rle  # noqa: E402


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S, C1, H, W, wide = 64, 120, 2, 480, 640, 8
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:S, 0:S]
    disc = (((yy - 0.5 * S) / (0.4 * S)) ** 2 + ((xx - 0.5 * S) / (0.3 * S)) ** 2 <= 1.0).astype(np.float32)
    l = rng.standard_normal((B, wide, S, S)).astype(np.float32) * 0.3
    l[:, 1] += 2.0 * disc - 1.0
    rc = np.stack([rng.integers(-30, H - S + 30, B), rng.integers(-30, W - S + 30, B)], 1)
    chan = np.ones(B, np.int64)
    view = torch.from_numpy(l).to(dev)[:, 0:C1]
    cd, rd = torch.from_numpy(chan.astype(np.int32)).to(dev), torch.from_numpy(rc.astype(np.int32)).to(dev)
    res = rle.paste_masks(view, cd, rd, H, W)
    want = pr.paste(l[:, 0:C1], chan, rc, H, W)
    assert np.array_equal(res["mask"].cpu().numpy(), want[0]) and np.array_equal(res["info"].cpu().numpy(), want[1])
    runs = rle.encode_planes(res["mask"])
    out = {"crops": B, "S": S, "C1": C1, "frame": [H, W], "plane_bytes": B * H * W, "logit_bytes": 4 * B * C1 * S * S,
           "pixels_per_mask": float(want[0].sum()) / B, "runs_per_mask": float(np.mean([len(r) for r in runs]))}
    out["paste_masks_ms"] = _events(lambda: rle.paste_masks(view, cd, rd, H, W), args.reps)
    planes = res["mask"]
    out["paste_masks_out_ms"] = _events(lambda: rle.paste_masks(view, cd, rd, H, W, out=planes), args.reps)
    out["encode_gpu_ms"] = _events(lambda: rle.encode_gpu(planes), args.reps)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
