"""Micro-bench: krrn_umeyama_ransac_f32 (estimateSimilarityTransform, lib/transform/umeyama.py:8-98) on
a B = 64 batch of synthetic crops (exact model coordinates of a known pose, cloud = R obj + t with
1 mm noise and 10 % outliers), N = 1000, H = 128; the PnP step (bench_pnp.py's call) on the same
xyz maps beside it.

usage (GPU box):  python3 profiles/bench_umeyama.py
CPU leg (where the reference is checked out; the same 64 crops, its own numpy function, its own draws):
                  python3 profiles/bench_umeyama.py --cpu-reference /path/to/reference
"""
import contextlib
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N, S, H = int(os.environ.get("B", 64)), 1000, 120, 128
K4 = np.array([572.4114, 573.57043, 325.2611, 242.04899], np.float32)
ext = np.array([0.067, 0.1276, 0.1175])
lfb = np.array([-0.0335, -0.0638, -0.0587])


def scene():
    rng = np.random.default_rng(0)
    xyz = np.zeros((B, 3, S, S), np.float32)
    choose = np.zeros((B, 1, N), np.int64)
    xm = np.zeros((B, N, 1), np.float32)
    ym = np.zeros((B, N, 1), np.float32)
    src = np.zeros((B, N, 3), np.float32)
    cloud = np.zeros((B, N, 3), np.float32)
    for b in range(B):
        ax = rng.normal(size=3)
        th = np.linalg.norm(ax)
        k = ax / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.1)])
        pix = rng.choice(S * S, N, replace=False)
        u32 = rng.random((N, 3)).astype(np.float32)
        obj = (u32.astype(np.float64) * ext + lfb).astype(np.float32)
        pc = obj.astype(np.float64) @ R.T + t
        img = np.stack([K4[0] * pc[:, 0] / pc[:, 2] + K4[2], K4[1] * pc[:, 1] / pc[:, 2] + K4[3]], 1)
        img += rng.normal(scale=0.4, size=img.shape)
        out = rng.random(N) < 0.1
        img[out] += rng.uniform(-20, 20, size=(out.sum(), 2))
        c = pc + rng.normal(scale=1e-3, size=pc.shape)
        c[out] = t + rng.uniform(-0.15, 0.15, size=(int(out.sum()), 3))
        xyz[b].reshape(3, -1)[:, pix] = u32.T
        choose[b, 0] = pix
        xm[b, :, 0], ym[b, :, 0] = img[:, 0], img[:, 1]
        src[b], cloud[b] = obj, c
    return xyz, choose, xm, ym, src, cloud


xyz, choose, xm, ym, src, cloud = scene()

if len(sys.argv) > 2 and sys.argv[1] == "--cpu-reference":
    sys.path.insert(0, sys.argv[2])
    from lib.transform.umeyama import estimateSimilarityTransform as ref_est
    np.random.seed(0)
    best = 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            for b in range(B):
                ref_est(src[b], cloud[b])
        best = min(best, time.perf_counter() - t0)
    print(f"B={B} N={N}: reference numpy estimateSimilarityTransform on the CPU: {best * 1e3:.1f} ms per batch "
          f"({best / B * 1e6:.0f} us per crop), best of 3")
    sys.exit(0)

import torch  # noqa: E402

from pose_estimation_amd import _lib, pose, umeyama  # noqa: E402
from pose_estimation_amd.runtime import P, ptr  # noqa: E402

dev = torch.device("cuda", 0)
data = {"choose": torch.from_numpy(choose).to(dev), "x_map_choosed": torch.from_numpy(xm).to(dev),
        "y_map_choosed": torch.from_numpy(ym).to(dev), "intrinsic": torch.from_numpy(np.tile(K4, (B, 1))).to(dev),
        "extent": torch.from_numpy(np.tile(ext, (B, 1))).to(dev),
        "lfborder": torch.from_numpy(np.tile(lfb, (B, 1))).to(dev), "cloud": torch.from_numpy(cloud).to(dev)}
pred = {"xyz": torch.from_numpy(xyz).to(dev)}
sel = pose.draw_sel(B, N, 256).to(dev)
_, _, pinfo = pose.get_pose(pred, data, sel=sel, return_info=True)
R, t, info = pose.get_pose_umeyama(pred, data, n_hyp=H, return_info=True)
assert torch.equal(info["src"].cpu(), torch.from_numpy(src))
subs, src_d, dst_d = info["subsets"], info["src"], data["cloud"]
counts, best = torch.empty_like(info["hyp_counts"]), torch.empty_like(info["best_hyp"])
scale, inl, mask = torch.empty_like(info["scale"]), torch.empty_like(info["inliers"]), torch.empty_like(info["mask"])
R2, t2 = torch.empty_like(R), torch.empty_like(t)
stream = P(torch.cuda.current_stream(dev).cuda_stream)
lib = _lib.lib()


def kernel_only():
    _lib.check(lib.krrn_umeyama_ransac_f32(ptr(src_d), ptr(dst_d), N, ptr(subs), H, umeyama.INLIER_FRAC,
                                           umeyama.CONFIDENCE, umeyama.MIN_RATIO, ptr(counts), ptr(scale), ptr(R2),
                                           ptr(t2), ptr(inl), ptr(best), ptr(mask), B, stream), "umeyama")


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b_.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b_) / reps * 1e3


us_k = timed(kernel_only)
us_u = timed(lambda: pose.get_pose_umeyama(pred, data, subsets=subs))
us_p = timed(lambda: pose.get_pose(pred, data, sel=sel, subsets=pinfo["subsets"]))
assert torch.equal(R2, R) and torch.equal(t2, t)
inl_f = inl.float()
print(f"B={B} N={N} H={H}: krrn_umeyama_ransac_f32 {us_k:8.1f} us; get_pose_umeyama (model points + solver) "
      f"{us_u:8.1f} us; get_pose (PnP, P=256, H=100) {us_p:8.1f} us; umeyama inliers mean {inl_f.mean():.1f} "
      f"min {int(inl_f.min())}", flush=True)
