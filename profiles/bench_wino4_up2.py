"""Micro-bench: the heads' first full-resolution conv (B = 64, 60 -> 120 px, 128 -> 128) as
  (a) krrn_resize_bilinear_f32 (align_corners, x2) + krrn_conv3x3_wino4_x3_f32 on the 120-px map,
  (b) krrn_conv3x3_wino4_x3_f32 with bit 1 of `relu` set: one launch reading the 60-px source,
  (p) the plain F(4x4) launch alone on the 120-px map,
alternating in one session: ROUNDS rounds of [a, b, p], each timed as a 20-launch burst (events around 20
launches after one untimed launch) and, with SUSTAINED=n, as n back-to-back launches. Also the error of (a)
and (b) against an f64 interpolate + conv of the first image.

usage (GPU box): python3 profiles/bench_wino4_up2.py      (ROUNDS=4 SUSTAINED=1000 ONLY=b for a counters run)
"""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pose_estimation_amd import _lib, ops  # noqa: E402
from pose_estimation_amd.runtime import P, ptr  # noqa: E402

dev = torch.device("cuda", 0)
B, C, Hs, Ws = 64, 128, 60, 60
H, W = 2 * Hs, 2 * Ws
L = _lib.lib()
g = torch.Generator().manual_seed(0)
conv = nn.Conv2d(C, C, 3, 1, 1, bias=False)
with torch.no_grad():
    conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (3.0 * C ** 0.5))
x = torch.relu(torch.randn(B, C, Hs, Ws, generator=g))
xa = ops.new_act(B, Hs, Ws, C, dev, cs=C)
xa.t.copy_(x.permute(0, 2, 3, 1).to(dev))
up = ops.new_act(B, H, W, C, dev, cs=C)
out = ops.new_act(B, H, W, C, dev, cs=C)
U4 = ops.wino_weights_x3(ops.wino4_weights(conv, dev, cin_p=C))
st = P(torch.cuda.current_stream().cuda_stream)
N = ptr(None)


def resize():
    _lib.check(L.krrn_resize_bilinear_f32(ptr(xa.t), B, Hs, Ws, C, 0, C, ptr(up.t), H, W, C, 0, N, 0, 0, 1, 0, st),
               "resize")


def plain():
    _lib.check(L.krrn_conv3x3_wino4_x3_f32(ptr(up.t), C, 0, B, H, W, C, ptr(U4), C, C, N, N, N, 0, 0, ptr(out.t), C, 0,
                                           1, st), "wino4")


def two():
    resize()
    plain()


def fused():
    _lib.check(L.krrn_conv3x3_wino4_x3_f32(ptr(xa.t), C, 0, B, H, W, C, ptr(U4), C, C, N, N, N, 0, 0, ptr(out.t), C, 0,
                                           3, st), "wino4 up2")


def ev_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


forms = [("a resize+plain", two), ("b fused", fused), ("p plain alone", plain)]
only = os.environ.get("ONLY")
if only:
    forms = [f for f in forms if f[0][0] in only.split(",")]
    resize()

if not os.environ.get("NOREF"):
    with torch.no_grad():
        ref = F.conv2d(F.interpolate(x[:1].double(), scale_factor=2, mode="bilinear", align_corners=True),
                       conv.weight.double(), padding=1).relu().permute(0, 2, 3, 1)
    for name, fn in forms:
        if name[0] == "p":
            continue
        out.t.zero_()
        fn()
        torch.cuda.synchronize()
        e = out.t[:1].double().cpu() - ref
        print(f"error {name}: max {float(e.abs().max() / ref.abs().max()):.2e} rms {float(e.norm() / ref.norm()):.2e}",
              flush=True)

sus = int(os.environ.get("SUSTAINED", "1000"))
for r in range(int(os.environ.get("ROUNDS", "4"))):
    line = f"round {r} burst20 us:"
    for name, fn in forms:
        line += f" | {name} {ev_time(fn, 20):7.1f}"
    print(line, flush=True)
    if sus:
        line = f"round {r} sustained{sus} us:"
        for name, fn in forms:
            line += f" | {name} {ev_time(fn, sus):7.1f}"
        print(line, flush=True)
