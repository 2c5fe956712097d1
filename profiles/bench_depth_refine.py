"""Micro-bench: pose.refine_pose_depth beside pose.refine_pose_icp on the same 64 crops of a LineMOD-layout tree
written by tests/mesh_tree.py (one object, a 320-face icosphere 6 cm across at 1 m: crop size 40, about 900 rendered
pixels per crop on a 640 x 480 frame). Both start from the GT pose 2 degrees and 3.5 mm off. HIP-event time per
call over the whole call (staging, launches, kernels), warm-up first, median of 7 groups of 5 calls, the two timed
in alternating rounds. Plain timing, no counters.

usage (GPU box):  python3 profiles/bench_depth_refine.py [--out profiles/depth_refine.json]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B = 64
OFF_T, OFF_DEG = (0.002, -0.0015, 0.0025), 2.0


def timed(fn, groups=7, per=5, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(groups):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / per)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    import mesh_tree
    from pose_estimation_amd import depth_refine, icp
    from pose_estimation_amd.dataset import PoseDataset
    from pose_estimation_amd.pose import refine_pose_depth, refine_pose_icp
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as root:
        mesh_tree.write_tree(root, objs=(6,), per_obj=(B,), depths=(1.0,))
        ds = PoseDataset("test", 500, False, root, 0.0, 8, cls_type="cat", n_model_pts=150, meshes=True)
        data = ds.batch(list(range(B)), dev, verify=True)
    a = np.deg2rad(OFF_DEG)
    k = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    dR = torch.tensor(np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx), dtype=torch.float32, device=dev)
    Rg, tg = data["target_r"].reshape(B, 3, 3), data["target_t"].reshape(B, 3)
    R0, t0 = (dR @ Rg).contiguous(), tg + torch.tensor(OFF_T, dtype=torch.float32, device=dev)
    dia = torch.tensor(ds.diameter, dtype=torch.float32).to(dev)[data["cls_id"].reshape(B)]
    fns = {"depth": lambda: refine_pose_depth(R0, t0, data, ds, dia),
           "icp": lambda: refine_pose_icp(R0, t0, data, diameter=dia)}
    res = {n: [] for n in fns}
    for _ in range(args.rounds):                                 # alternating: the box is shared with other work
        for n, fn in fns.items():
            res[n].append(timed(fn))
    out = {n: {"ms_median_per_round": [r["ms_median"] for r in v], "ms_min": min(r["ms_min"] for r in v),
               "ms_max": max(r["ms_max"] for r in v)} for n, v in res.items()}
    out["ratio_depth_over_icp"] = float(np.median(out["depth"]["ms_median_per_round"]) /
                                        np.median(out["icp"]["ms_median_per_round"]))

    def err(R, t):
        c = ((R @ Rg.transpose(1, 2)).diagonal(dim1=1, dim2=2).sum(1).double() - 1.0) / 2.0
        return (float(torch.rad2deg(torch.acos(c.clamp(-1, 1))).median()), float((t - tg).norm(dim=1).median() * 1e3))

    Rd, td, info_d = refine_pose_depth(R0, t0, data, ds, dia, return_info=True)
    Ri, ti, info_i = refine_pose_icp(R0, t0, data, diameter=dia, return_info=True)
    torch.cuda.synchronize()
    out["median_error_deg_mm"] = {"start": err(R0, t0), "depth": err(Rd, td), "icp": err(Ri, ti)}
    out["status_counts"] = {"depth": torch.bincount(info_d["status"].long(), minlength=4).tolist(),
                            "icp": torch.bincount(info_i["status"].long(), minlength=4).tolist()}
    out["passes_mean"] = {"depth": float(info_d["passes"].double().mean()), "icp": float(info_i["passes"].double().mean())}
    out["pairs_mean"] = {"depth": float(info_d["pairs"].double().mean()), "icp": float(info_i["pairs"].double().mean())}
    out["defaults"] = {"depth": [depth_refine.MAX_ITER, depth_refine.DIST_FRAC], "icp": [icp.MAX_ITER, icp.DIST_FRAC]}
    out["box"] = {"gpu": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip}
    out.update(B=B, mesh_faces=320, frame=[480, 640], cloud_points=int(data["cloud"].shape[1]),
               model_points=int(data["model_points"].shape[1]))
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
