"""Micro-bench: the pose-candidate score (krrn_pose_score_f32) for B = 64 crops of bench_bop.py's object (an
icosphere of 20480 faces, radius 7 cm at about 0.8 m: about 100 px across a 640 x 480 frame), with C = 2 candidates
(an estimate a few degrees / millimetres off, the GT pose) and C = 4 (two coarser perturbations added), the mask =
the GT pose's visible mask (bop.visibility), the box = the 120-px crop. Beside it krrn_bop_vsd_f32 on the same
batch, which does the same two depth walks per crop as C = 2. HIP-event time per call, warm-up first, median of 5
groups of 10, the three timed in alternating rounds. Then an eval epoch with and without select="depth" over a
LineMOD-layout tree written by tests/mesh_tree.py (one object, 1280-face mesh), in alternating runs. Plain timing,
no counters.

usage (GPU box):  python3 profiles/bench_verify.py [--out profiles/verify.json] [--frames 128]
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

B, S, SUBDIV, RADIUS = 64, 120, 5, 0.07


def kernels(dev, rounds=3):
    import torch
    import bop_ref as br
    import raster_ref as rr
    from pose_estimation_amd import _lib, bop, raster, verify
    from pose_estimation_amd.runtime import P, ptr
    rng = np.random.default_rng(0)
    v, f = rr.icosphere(SUBDIV, RADIUS)
    v = v.astype(np.float32)
    R_gt = np.stack([rr.rotation(rng) for _ in range(B)])
    cen = np.stack([rng.uniform(100, rr.W - 100, B), rng.uniform(100, rr.H - 100, B)], 1)
    t_gt = np.stack([rr._centre_t(rng.uniform(0.75, 0.85), c[0], c[1]) for c in cen])
    near = [br.perturbed(rng, R_gt[b], t_gt[b]) for b in range(B)]
    far = [[br.perturbed(rng, R_gt[b], t_gt[b], deg=8, mm=15) for b in range(B)] for _ in range(2)]
    cand = [near, list(zip(R_gt, t_gt))] + far                   # priority order; the first two are VSD's pair
    R4 = np.stack([np.stack([c[b][0] for c in cand]) for b in range(B)])     # [B, 4, 3, 3]
    t4 = np.stack([np.stack([c[b][1] for c in cand]) for b in range(B)])     # [B, 4, 3]
    boxes = np.array([(int(c[1]) - S // 2, int(c[1]) + S // 2, int(c[0]) - S // 2, int(c[0]) + S // 2) for c in cen], np.int32)
    tt = torch.from_numpy
    verts, faces = tt(v).to(dev), tt(f).to(dev)
    fr = torch.tensor([[0, len(f)]] * B, dtype=torch.int32, device=dev)
    K4 = torch.tensor([rr.LM_K4] * B, dtype=torch.float32, device=dev)
    frame = torch.arange(B, dtype=torch.int32, device=dev)
    Rg, tg = tt(R_gt).reshape(B, 9).to(dev), tt(t_gt).to(dev)
    # observed frames: the GT render over a 1.5 m background, 2 % holes (metres); the mask is its visible part
    rp = raster.region_points(verts, 64)[None].expand(B, 64, 3).contiguous()
    gt = raster.render_maps(verts, faces, fr, Rg, tg, K4, [tuple(int(x) for x in b) for b in boxes], rp)
    depth = torch.full((B, rr.H, rr.W), 1.5, device=dev)
    for b, (r0, r1, c0, c1) in enumerate(boxes):
        depth[b, r0:r1, c0:c1] = torch.where(gt["depth"][b] > 0, gt["depth"][b], depth[b, r0:r1, c0:c1])
    depth[torch.rand((B, rr.H, rr.W), device=dev) < 0.02] = 0.0
    mask = bop.visibility(verts, faces, fr, Rg, tg, K4, depth, frame)["mask_visib"].contiguous()
    box = tt(boxes).to(dev)
    tau = torch.full((B,), verify.TAU, dtype=torch.float64, device=dev)
    st = P(torch.cuda.current_stream(dev).cuda_stream)
    outs = {}

    def scorer(C):
        R = tt(np.ascontiguousarray(R4[:, :C])).reshape(B, C, 9).to(dev)
        t = tt(np.ascontiguousarray(t4[:, :C])).to(dev)
        ws = torch.empty((B, C, 4), dtype=torch.int32, device=dev)
        counts = torch.empty((B, C, 6), dtype=torch.int32, device=dev)
        score = torch.empty((B, C), dtype=torch.float64, device=dev)
        best = torch.empty((B,), dtype=torch.int32, device=dev)
        Rs, ts = torch.empty((B, 9), device=dev), torch.empty((B, 3), device=dev)
        outs[C] = (counts, score, best)

        def run():
            _lib.call("krrn_pose_score_f32", ptr(verts), verts.shape[0], ptr(faces), faces.shape[0], ptr(fr), ptr(R), ptr(t),
                      C, ptr(K4), ptr(depth), ptr(mask), B, rr.H, rr.W, ptr(frame), ptr(box), 1.0, ptr(tau), B, ptr(ws),
                      ptr(counts), ptr(score), ptr(best), ptr(Rs), ptr(ts), st)
        return run

    Re, te = tt(np.ascontiguousarray(R4[:, 0])).reshape(B, 9).to(dev), tt(np.ascontiguousarray(t4[:, 0])).to(dev)
    dia = torch.full((B,), 2 * RADIUS, dtype=torch.float64, device=dev)
    taus = torch.tensor(bop.TAUS, dtype=torch.float64, device=dev)
    T = len(bop.TAUS)
    vws = torch.empty((B, 8), dtype=torch.int32, device=dev)
    vcounts = torch.empty((B, 2 + T), dtype=torch.int32, device=dev)
    e_vsd = torch.empty((B, T), dtype=torch.float64, device=dev)

    def vsd():
        _lib.call("krrn_bop_vsd_f32", ptr(verts), verts.shape[0], ptr(faces), faces.shape[0], ptr(fr), ptr(Re), ptr(te),
                  ptr(Rg), ptr(tg), ptr(K4), ptr(depth), B, rr.H, rr.W, ptr(frame), 1.0, ptr(dia), bop.DELTA, ptr(taus), T,
                  B, ptr(vws), ptr(vcounts), ptr(e_vsd), st)

    fns = {"vsd": vsd, "score_c2": scorer(2), "score_c4": scorer(4)}
    res = {k: [] for k in fns}
    for _ in range(rounds):                                      # alternating: the box is shared with other work
        for k, fn in fns.items():
            res[k].append(timed(fn))
    torch.cuda.synchronize()
    out = {k: {"ms_median_per_round": [r["ms_median"] for r in v], "ms_min": min(r["ms_min"] for r in v),
               "ms_max": max(r["ms_max"] for r in v)} for k, v in res.items()}
    c2, c4 = outs[2], outs[4]
    assert torch.equal(c2[0], c4[0][:, :2])                      # a candidate's counts do not depend on C
    out["best_histogram_c4"] = torch.bincount(c4[2].long(), minlength=4).tolist()
    out["mean_score_c4"] = [round(float(x), 4) for x in c4[1].mean(0)]
    out["render_px_mean"] = float(c4[0][:, 1, 0].double().mean())
    out["verify_max_c"] = verify.MAX_C
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
        ds = {g: PoseDataset("test", 1000, False, root, 0.0, 8, cls_type="cat", n_model_pts=600, meshes=True)
              for g in (None, "depth")}
        m = KRRN(cfg=make_config(num_cls=1, backbone="w18"))
        init_weights(m, 0)
        m = m.to(dev).eval()
        res = {None: [], "depth": []}
        for rep in range(reps + 1):           # the first pair builds the plans and is dropped
            for g in (None, "depth"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = test_epoch(m, ds[g], bs=64, device=dev, select=g)
                torch.cuda.synchronize()
                if rep:
                    res[g].append(frames / (time.perf_counter() - t0))
    return {"frames": frames, "bs": 64, "mesh_faces": 1280, "candidates": 2,
            "crops_per_s_without_select": [round(x, 1) for x in res[None]],
            "crops_per_s_with_select": [round(x, 1) for x in res["depth"]], "select": out["select"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=128)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    result = {"kernels": ["krrn_pose_score_f32", "krrn_bop_vsd_f32"], "B": B, "faces": 20 * 4 ** SUBDIV,
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
