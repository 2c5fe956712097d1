"""Micro-bench: krrn_icp_refine_f32 (icp.refine, the ICP pose refinement) on batches of noisy synthetic
scenes: per crop a 2600-point model (a bumpy ellipsoid of about 12 x 8 x 6 cm), a ground-truth pose at
about 0.8 m, a cloud of N = 1000 points from the half of the model that faces the camera with 1 mm
noise and 5 % outliers, and a start pose 3 degrees and N(0, 5 mm) off. B = 64 and 256, max_iter 20,
max_dist 20 mm; HIP-event time per launch and the passes the crops used.

usage (GPU box):  python3 profiles/bench_icp.py [--out profiles/r7_icp.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, M, MAX_ITER, MAX_DIST = 1000, 2600, 20, 0.02


def rodrigues(axis, deg):
    k = axis / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def scenes(B, seed=0):
    rng = np.random.default_rng(seed)
    R0, t0 = np.zeros((B, 3, 3), np.float32), np.zeros((B, 3), np.float32)
    cloud, model = np.zeros((B, N, 3), np.float32), np.zeros((B, M, 3), np.float32)
    Rgt, tgt = np.zeros((B, 3, 3)), np.zeros((B, 3))
    for b in range(B):
        u = rng.normal(size=(M, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        r = 1.0 + 0.1 * np.sin(5.0 * u[:, 0]) * np.cos(4.0 * u[:, 1]) + 0.05 * np.sin(7.0 * u[:, 2])
        m = (u * r[:, None] * np.array([0.06, 0.04, 0.03])).astype(np.float32)
        Rg = rodrigues(rng.normal(size=3), rng.uniform(0.0, 360.0))
        tg = np.array([0.05, -0.03, 0.8]) + rng.normal(scale=0.01, size=3)
        pc = m.astype(np.float64) @ Rg.T + tg
        near = np.argsort(pc[:, 2], kind="stable")[:M // 2]
        c = pc[rng.choice(near, N, replace=True)] + rng.normal(scale=1e-3, size=(N, 3))
        out = rng.random(N) < 0.05
        c[out] += rng.choice([-0.2, 0.2], size=(int(out.sum()), 3))
        R0[b] = rodrigues(rng.normal(size=3), 3.0) @ Rg
        t0[b] = tg + rng.normal(scale=0.005, size=3)
        cloud[b], model[b], Rgt[b], tgt[b] = c, m, Rg, tg
    return R0, t0, cloud, model, Rgt, tgt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from pose_estimation_amd import _lib, icp
    from pose_estimation_amd.runtime import P, ptr

    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    result = {"kernel": "krrn_icp_refine_f32", "N": N, "M": M, "max_iter": MAX_ITER, "max_dist_m": MAX_DIST,
              "tol": icp.TOL, "min_pairs": icp.MIN_PAIRS,
              "scenes": "bumpy-ellipsoid model, camera-facing half, 1 mm noise, 5 % outliers, start 3 deg / 5 mm off",
              "runs": []}
    for B in (64, 256):
        R0, t0, cloud, model, Rgt, tgt = scenes(B)
        d = [torch.from_numpy(x).to(dev) for x in (R0, t0, cloud, model)]
        md = torch.full((B,), MAX_DIST, dtype=torch.float32, device=dev)
        R, t, info = icp.solve(*d, md, MAX_ITER)
        stream = P(torch.cuda.current_stream(dev).cuda_stream)

        def launch():
            _lib.check(lib.krrn_icp_refine_f32(ptr(d[0]), ptr(d[1]), ptr(d[2]), N, ptr(d[3]), M, ptr(md), MAX_ITER,
                                               icp.TOL, icp.MIN_PAIRS, ptr(R), ptr(t), ptr(info["passes"]),
                                               ptr(info["pairs"]), ptr(info["rmse"]), ptr(info["status"]),
                                               ptr(info["nn_idx"]), B, stream), "krrn_icp_refine_f32")

        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):  # 5 timed groups of 10 launches
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                launch()
            b_.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b_) / 10)
        passes = info["passes"].cpu().numpy()
        status = info["status"].cpu().numpy()
        Rn, tn = R.double().cpu().numpy(), t.double().cpu().numpy()
        mo = model.astype(np.float64)
        add = lambda Rx, tx: np.linalg.norm((mo @ Rx.transpose(0, 2, 1) + tx[:, None]) -  # noqa: E731
                                            (mo @ Rgt.transpose(0, 2, 1) + tgt[:, None]), axis=2).mean(1)
        a0, a1 = add(R0.astype(np.float64), t0.astype(np.float64)), add(Rn, tn)
        run = {"B": B, "ms_per_launch_median": round(float(np.median(times)), 4),
               "ms_per_launch_min": round(float(min(times)), 4), "ms_per_launch_max": round(float(max(times)), 4),
               "us_per_crop": round(float(np.median(times)) / B * 1e3, 2),
               "passes_mean": round(float(passes.mean()), 2), "passes_min": int(passes.min()),
               "passes_max": int(passes.max()),
               "status_counts": {icp.STATUS[s]: int((status == s).sum()) for s in range(4)},
               "pairs_mean": round(float(info["pairs"].float().mean()), 1),
               "add_mm_before_mean": round(float(a0.mean() * 1e3), 3), "add_mm_after_mean": round(float(a1.mean() * 1e3), 3)}
        result["runs"].append(run)
        print(json.dumps(run), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
