"""Micro-bench: the BOP-19 pose errors for B = 64 crops of config 2's kind of object (an icosphere of 20480 faces,
10242 vertices, radius 7 cm at about 0.8 m: about 100 px across a 640 x 480 frame), random GT poses, estimates a
few degrees / millimetres away. HIP-event time per call, warm-up first, median of 5 groups of 10:
  vsd_fused      krrn_bop_vsd_f32 (three launches: boxes, render-and-compare over the whole frame, finish)
  vsd_composed   what the parent commit allows on the same inputs: two raster.render_maps calls over the object's
                 120-px window plus the elementwise compare and the counts in torch (f64)
  mssd_mspd      krrn_bop_mssd_mspd_f32 with NS = 1 and NS = 315
and an eval epoch with and without bop=True over a LineMOD-layout tree written by tests/mesh_tree.py (one object,
1280-face mesh), in alternating runs. Plain timing, no counters.

usage (GPU box):  python3 profiles/bench_bop.py [--out profiles/bop.json] [--frames 128]
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

from bench_raster import timed  # noqa: E402

B, S, SUBDIV, RADIUS, NR = 64, 120, 5, 0.07, 64


def kernels(dev):
    import torch
    import bop_ref as br
    import raster_ref as rr
    from pose_estimation_amd import _lib, bop, raster
    from pose_estimation_amd.runtime import P, ptr
    rng = np.random.default_rng(0)
    v, f = rr.icosphere(SUBDIV, RADIUS)
    v = v.astype(np.float32)
    R_gt = np.stack([rr.rotation(rng) for _ in range(B)])
    cen = np.stack([rng.uniform(100, rr.W - 100, B), rng.uniform(100, rr.H - 100, B)], 1)
    t_gt = np.stack([rr._centre_t(rng.uniform(0.75, 0.85), c[0], c[1]) for c in cen])
    est = [br.perturbed(rng, R_gt[b], t_gt[b]) for b in range(B)]
    R_est, t_est = np.stack([e[0] for e in est]), np.stack([e[1] for e in est])
    boxes = [(int(c[1]) - S // 2, int(c[1]) + S // 2, int(c[0]) - S // 2, int(c[0]) + S // 2) for c in cen]
    tt = torch.from_numpy
    verts, faces = tt(v).to(dev), tt(f).to(dev)
    fr = torch.tensor([[0, len(f)]] * B, dtype=torch.int32, device=dev)
    Re, te, Rg, tg = (tt(a).reshape(B, -1).to(dev) for a in (R_est, t_est, R_gt, t_gt))
    K4 = torch.tensor([rr.LM_K4] * B, dtype=torch.float32, device=dev)
    rp = raster.region_points(verts, NR)[None].expand(B, NR, 3).contiguous()
    # observed frames: the GT render over a 1.5 m background, 2 % holes (metres)
    gt = raster.render_maps(verts, faces, fr, Rg, tg, K4, boxes, rp)
    depth = torch.full((B, rr.H, rr.W), 1.5, device=dev)
    for b, (r0, r1, c0, c1) in enumerate(boxes):
        depth[b, r0:r1, c0:c1] = torch.where(gt["depth"][b] > 0, gt["depth"][b], depth[b, r0:r1, c0:c1])
    depth[torch.rand((B, rr.H, rr.W), device=dev) < 0.02] = 0.0
    frame = torch.arange(B, dtype=torch.int32, device=dev)
    dia = torch.full((B,), 2 * RADIUS, dtype=torch.float64, device=dev)
    taus = torch.tensor(bop.TAUS, dtype=torch.float64, device=dev)
    T = len(bop.TAUS)
    ws = torch.empty((B, 8), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 2 + T), dtype=torch.int32, device=dev)
    e_vsd = torch.empty((B, T), dtype=torch.float64, device=dev)
    st = P(torch.cuda.current_stream(dev).cuda_stream)

    def fused():
        _lib.call("krrn_bop_vsd_f32", ptr(verts), verts.shape[0], ptr(faces), faces.shape[0], ptr(fr), ptr(Re), ptr(te),
                  ptr(Rg), ptr(tg), ptr(K4), ptr(depth), B, rr.H, rr.W, ptr(frame), 1.0, ptr(dia), bop.DELTA, ptr(taus), T,
                  B, ptr(ws), ptr(counts), ptr(e_vsd), st)

    rows = torch.stack([torch.arange(b[0], b[1], device=dev) for b in boxes])[:, :, None].expand(B, S, S)
    cols = torch.stack([torch.arange(b[2], b[3], device=dev) for b in boxes])[:, None, :].expand(B, S, S)
    bidx = torch.arange(B, device=dev)[:, None, None].expand(B, S, S)
    fx, fy, cx, cy = (float(np.float32(k)) for k in rr.LM_K4)
    ray = torch.sqrt((((cols.double() - cx) / fx) ** 2 + ((rows.double() - cy) / fy) ** 2) + 1.0)
    tau_b = taus.view(1, T, 1, 1)

    def composed():
        d_est = raster.render_maps(verts, faces, fr, Re, te, K4, boxes, rp)["depth"].double() * ray
        d_gt = raster.render_maps(verts, faces, fr, Rg, tg, K4, boxes, rp)["depth"].double() * ray
        obs = depth[bidx, rows, cols].double() * ray

        def visib(m):
            return ((obs > 0) & (m > 0) & ((m - obs) <= bop.DELTA)) | ((obs == 0) & (m > 0))

        v_gt = visib(d_gt)
        v_est = visib(d_est) | (v_gt & (d_est > 0))
        inter, union = v_gt & v_est, v_gt | v_est
        cost = (d_gt - d_est).abs() / dia.view(B, 1, 1)
        steps = (inter[:, None] & (cost[:, None] >= tau_b)).sum((2, 3))
        un, it = union.sum((1, 2)), inter.sum((1, 2))
        return un, it, steps, torch.where(un[:, None] > 0, (steps + (un - it)[:, None]).double() / un[:, None], 1.0)

    fused()
    un, it, steps, e_c = composed()
    torch.cuda.synchronize()
    # the composition's depth maps are f32 and its window is the crop, so equality is not expected to the bit
    out = {"vsd_fused": timed(fused), "vsd_composed": timed(composed),
           "union_px_mean": float(counts[:, 0].double().mean()),
           "max_abs_e_vsd_difference_fused_vs_composed": float((e_vsd - e_c).abs().max())}
    for name, S12 in (("mssd_mspd_ns1", bop.symmetry_set()),
                      ("mssd_mspd_ns315", bop.symmetry_set(continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}]))):
        sy = tt(S12).to(dev)
        vr = torch.tensor([[0, len(v)]] * B, dtype=torch.int32, device=dev)
        sr = torch.tensor([[0, len(S12)]] * B, dtype=torch.int32, device=dev)
        m3, m2 = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
        mws = torch.empty(3 * B * bop.SYM_SPLIT, dtype=torch.float64, device=dev)
        out[name] = timed(lambda: _lib.call("krrn_bop_mssd_mspd_f32", ptr(verts), verts.shape[0], ptr(vr), ptr(Re), ptr(te),
                                            ptr(Rg), ptr(tg), ptr(K4), ptr(sy), sy.shape[0], ptr(sr), B, ptr(mws), ptr(m3),
                                            ptr(m2), P(0), st))
    return out


def epochs(dev, frames, reps=3):
    import torch
    import mesh_tree
    from pose_estimation_amd import KRRN, make_config
    from pose_estimation_amd.dataset import PoseDataset
    from pose_estimation_amd.evaluate import test_epoch
    from pose_estimation_amd.synthetic import init_weights
    with tempfile.TemporaryDirectory() as root:
        mesh_tree.write_tree(root, objs=(6,), per_obj=(frames,), depths=(0.36,), subdiv=3)
        ds = {g: PoseDataset("test", 1000, False, root, 0.0, 8, cls_type="cat", n_model_pts=600, meshes=g)
              for g in (False, True)}
        m = KRRN(cfg=make_config(num_cls=1, backbone="w18"))
        init_weights(m, 0)
        m = m.to(dev).eval()
        res = {False: [], True: []}
        for rep in range(reps + 1):           # the first pair builds the plans and is dropped
            for g in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = test_epoch(m, ds[g], bs=64, device=dev, bop=g)
                torch.cuda.synchronize()
                if rep:
                    res[g].append(frames / (time.perf_counter() - t0))
    return {"frames": frames, "bs": 64, "mesh_faces": 1280, "crop_sizes": sorted({ds[True].crop_size(i) for i in range(frames)}),
            "crops_per_s_without_bop": [round(x, 1) for x in res[False]],
            "crops_per_s_with_bop": [round(x, 1) for x in res[True]],
            "bop": {k: out["bop"][k] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR", "count")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=128)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    result = {"kernels": ["krrn_bop_vsd_f32", "krrn_bop_mssd_mspd_f32"], "B": B, "faces": 20 * 4 ** SUBDIV,
              "box": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
                      "cus": torch.cuda.get_device_properties(0).multi_processor_count, "torch": torch.__version__,
                      "hip": torch.version.hip}}
    result.update(kernels(dev))
    print(json.dumps(result), flush=True)
    if args.frames:
        result["epoch"] = epochs(dev, args.frames)
        print(json.dumps(result["epoch"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
