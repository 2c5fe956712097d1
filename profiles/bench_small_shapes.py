"""Micro-bench of krrn_conv_small_f32 on arbitrary shapes at B = 64 (no residual, the plan's (nw, ks) from
ops.small_conv_config): best of five back-to-back runs of 50 launches. Default shapes: four HRNet-W18
fuse-layer convs (cin -> cout, kernel / stride, input side). SHAPES="cin,cout,side,k,stride;..." times others
(profiles/conv_small_tail_ab.txt: the two-quad-tail shapes). KRRN_HIP_LIB selects a kernel-variant build
(profiles/build_variant.sh).

usage (GPU box): python3 profiles/bench_small_shapes.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pose_estimation_amd import _lib, ops  # noqa: E402
from pose_estimation_amd.runtime import P, ptr  # noqa: E402

dev = torch.device("cuda", 0)
B = 64
L = _lib.lib()
st = P(torch.cuda.current_stream().cuda_stream)
tag = os.path.basename(os.environ.get("KRRN_HIP_LIB", "in-tree"))
SHAPES = [(72, 36, 8, 1, 1), (36, 72, 15, 3, 2), (20, 36, 30, 3, 2), (36, 20, 15, 1, 1)]
if os.environ.get("SHAPES"):  # "cin,cout,H,k,s;..."
    SHAPES = [tuple(int(v) for v in t.split(",")) for t in os.environ["SHAPES"].split(";")]
for cin, cout, H, k, s in SHAPES:
    g = torch.Generator().manual_seed(0)
    Ho = (H + 2 * ((k - 1) // 2) - k) // s + 1
    x = torch.randn(B, H, H, cin, generator=g).to(dev)
    w = (0.05 * torch.randn(cout, k * k * cin, generator=g)).to(dev)
    sc, bi = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
    out = torch.zeros(B, Ho, Ho, cout, device=dev)
    nw, ks = ops.small_conv_config(B * Ho * Ho, (cout + 15) // 16, cin)

    def run():
        _lib.check(L.krrn_conv_small_f32(ptr(x), cin, 0, B, H, H, cin, ptr(w), cout, cout, ptr(sc), ptr(bi), P(0), 0, 0,
                                         ptr(out), cout, 0, 0, k, s, nw, ks, st), "small")
    run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(5):
        a.record()
        for _ in range(50):
            run()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / 50 * 1e3)
    print(f"{tag:18s} {cin:3d}->{cout:3d} {k}x{k}/{s} {H:2d}px nw {nw} ks {ks}: back-to-back {best:6.1f} us", flush=True)
