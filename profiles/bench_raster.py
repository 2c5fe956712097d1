"""Micro-bench: GT-map rendering (krrn_raster_maps_f32 + krrn_gt_maps_finish_f32) for B = 64 crops of S = 120
over an icosphere of 20480 faces (10242 vertices, radius 7 cm at about 0.8 m: about 100 px across), random
poses; HIP-event time per launch, the numpy restatement (tests/raster_ref.py) on the same crops on the
host, and an eval epoch with and without gt_maps over a LineMOD-layout tree written by tests/mesh_tree.py
(one object, 1280-face mesh, crops of 120), in alternating runs. Plain timing, no counters.

usage (GPU box):  python3 profiles/bench_raster.py [--out profiles/raster.json] [--frames 128] [--ref-crops 2]
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

B, S, SUBDIV, RADIUS, NR = 64, 120, 5, 0.07, 64


def timed(fn, groups=5, per=10):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(groups):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / per)
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def kernels(dev, ref_crops):
    import torch
    import raster_ref as rr
    from pose_estimation_amd import _lib, raster
    from pose_estimation_amd.runtime import P, ptr
    rng = np.random.default_rng(0)
    v, f = rr.icosphere(SUBDIV, RADIUS)
    v = v.astype(np.float32)
    R = np.stack([rr.rotation(rng) for _ in range(B)])
    cen = np.stack([rng.uniform(100, rr.W - 100, B), rng.uniform(100, rr.H - 100, B)], 1)
    t = np.stack([rr._centre_t(rng.uniform(0.75, 0.85), c[0], c[1]) for c in cen])
    boxes = [(int(c[1]) - S // 2, int(c[1]) + S // 2, int(c[0]) - S // 2, int(c[0]) + S // 2) for c in cen]
    tt = torch.from_numpy
    verts, faces = tt(v).to(dev), tt(f).to(dev)
    rp = raster.region_points(verts, NR)
    K4 = torch.tensor([rr.LM_K4] * B, dtype=torch.float32)
    args = (verts, faces, torch.tensor([[0, len(f)]] * B, dtype=torch.int32), tt(R), tt(t), K4, boxes,
            rp[None].expand(B, NR, 3).contiguous())
    maps = raster.render_maps(*args, frame_hw=(rr.H, rr.W))
    torch.cuda.synchronize()
    cover = float((maps["face"] >= 0).float().mean())
    # the same launches on fixed buffers
    fr, R64, t64 = args[2].to(dev), args[3].reshape(B, 9).to(dev), args[4].to(dev)
    Kd, rc, rpb = K4.to(dev), torch.tensor([[b[0], b[2]] for b in boxes], dtype=torch.int32, device=dev), args[7]
    st = P(torch.cuda.current_stream(dev).cuda_stream)

    def render():
        _lib.call("krrn_raster_maps_f32", ptr(verts), verts.shape[0], ptr(faces), faces.shape[0], ptr(fr), ptr(R64),
                  ptr(t64), ptr(Kd), ptr(rc), S, ptr(rpb), NR, B, ptr(maps["face"]), ptr(maps["depth"]),
                  ptr(maps["coord"]), ptr(maps["normal"]), ptr(maps["region"]), ptr(maps["cover_frame"]), rr.H, rr.W, st)

    pm = (maps["face"] >= 0).to(torch.uint8).view(B, 1, S, S)
    cls = torch.zeros(B, dtype=torch.int64, device=dev)
    ext = torch.full((B, 3), 0.14, dtype=torch.float64, device=dev)
    lfb = torch.full((B, 3), -0.07, dtype=torch.float64, device=dev)
    out = {"render": timed(render), "finish": timed(lambda: raster.finish_maps(maps, pm, cls, ext, lfb)),
           "covered_fraction": round(cover, 3)}
    same = True
    t0 = time.perf_counter()
    for b in range(ref_crops):
        ref = rr.render(v, f, R[b], t[b], rr.LM_K4, boxes[b][0], boxes[b][2], S, rp.cpu().numpy(), margins=False)
        same = same and bool(np.array_equal(ref["face"], maps["face"][b].cpu().numpy()))
    per = (time.perf_counter() - t0) / max(ref_crops, 1)
    out["host_numpy_s_per_crop"] = round(per, 3)
    out["host_numpy_s_per_64_crops_scaled"] = round(per * B, 1)
    out["host_crops_timed"] = ref_crops
    out["host_face_map_equals_gpu"] = same
    return out


def epochs(dev, frames, reps=3):
    import torch
    import mesh_tree
    from pose_estimation_amd import KRRN, make_config
    from pose_estimation_amd.dataset import PoseDataset
    from pose_estimation_amd.evaluate import test_epoch
    from pose_estimation_amd.loss import KRRNLoss
    from pose_estimation_amd.synthetic import init_weights
    with tempfile.TemporaryDirectory() as root:
        mesh_tree.write_tree(root, objs=(6,), per_obj=(frames,), depths=(0.36,), subdiv=3)
        ds = {g: PoseDataset("test", 1000, False, root, 0.0, 8, cls_type="cat", n_model_pts=600, gt_maps=g)
              for g in (False, True)}
        sizes = sorted({ds[True].crop_size(i) for i in range(frames)})
        m = KRRN(cfg=make_config(num_cls=1, backbone="w18"))
        init_weights(m, 0)
        m = m.to(dev).eval()
        crit = KRRNLoss(sym_list=[])
        res = {False: [], True: []}
        for rep in range(reps + 1):           # the first pair builds the plans and is dropped
            for g in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                test_epoch(m, ds[g], bs=64, device=dev, criterion=crit)
                torch.cuda.synchronize()
                if rep:
                    res[g].append(frames / (time.perf_counter() - t0))
    return {"frames": frames, "crop_sizes": sizes, "bs": 64, "mesh_faces": 1280,
            "crops_per_s_without_gt_maps": [round(x, 1) for x in res[False]],
            "crops_per_s_with_gt_maps": [round(x, 1) for x in res[True]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--ref-crops", type=int, default=2)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    result = {"kernels": ["krrn_raster_maps_f32", "krrn_gt_maps_finish_f32"], "B": B, "S": S, "faces": 20 * 4 ** SUBDIV,
              "box": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
                      "cus": torch.cuda.get_device_properties(0).multi_processor_count, "torch": torch.__version__,
                      "hip": torch.version.hip}}
    result.update(kernels(dev, args.ref_crops))
    print(json.dumps(result), flush=True)
    if args.frames:
        result["epoch"] = epochs(dev, args.frames)
        print(json.dumps(result["epoch"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
