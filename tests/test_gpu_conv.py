"""Implicit-GEMM conv kernel vs a plain PyTorch fp32 reference of the same op."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pose_estimation_amd import ops

pytestmark = pytest.mark.gpu

TOL = dict(rtol=2e-4, atol=2e-4)


def _nhwc(x, dev, cs=None, co=0):
    B, C, H, W = x.shape
    a = ops.new_act(B, H, W, C, dev, cs=cs)
    a = a.slice(co, C) if co else a
    a.t[..., co:co + C] = x.permute(0, 2, 3, 1).to(dev)
    return a


def _bn(c, g):
    bn = nn.BatchNorm2d(c).eval()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.1 * torch.randn(c, generator=g))
        bn.bias.copy_(0.1 * torch.randn(c, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(c, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(c, generator=g))
    return bn


@pytest.mark.parametrize("cin,cout,k,s,H,bias,tile", [
    (3, 64, 3, 2, 33, False, 0), (64, 64, 3, 2, 60, False, 0), (18, 36, 3, 1, 15, False, 0),
    (270, 270, 3, 1, 30, True, 1), (256, 18, 3, 1, 30, False, 3), (144, 18, 1, 1, 4, False, 2),
    (72, 144, 3, 2, 8, False, 3), (128, 128, 3, 1, 61, False, 1)])
def test_conv_bn_relu_res(dev, cin, cout, k, s, H, bias, tile):
    g = torch.Generator().manual_seed(cin * 7 + cout)
    B = 3
    conv = nn.Conv2d(cin, cout, k, s, (k - 1) // 2, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(0.05 * torch.randn(conv.weight.shape, generator=g))
        if bias:
            conv.bias.copy_(0.1 * torch.randn(cout, generator=g))
    bn = _bn(cout, g)
    x = torch.randn(B, cin, H, H, generator=g)
    ref = bn(conv(x))
    res = torch.randn(ref.shape, generator=g)
    ref = torch.relu(ref + res).detach()
    spec = ops.make_conv(conv, bn, dev)
    xa = _nhwc(x, dev)
    Ho, Wo = ops.conv_out_hw(spec, H, H)
    out = ops.new_act(B, Ho, Wo, cout, dev, cs=ops.pad4(cout) + 8)
    ra = _nhwc(res, dev)
    ops.conv2d(xa, spec, out, res=ra, relu=True, tile=tile)
    torch.cuda.synchronize()
    got = out.t[..., :cout].permute(0, 3, 1, 2).cpu()
    torch.testing.assert_close(got, ref, **TOL)
    # pad channels stay exactly zero
    assert torch.count_nonzero(out.t[..., cout:]).item() == 0


@pytest.mark.parametrize("cin,cout,H,tile,splits", [
    (144, 144, 4, 8, 10), (72, 72, 8, 8, 4), (36, 36, 15, 8, 3), (18, 20, 30, 6, 16), (144, 144, 4, 3, 64),
    (64, 128, 9, 7, 5)])
def test_conv_splitk(dev, cin, cout, H, tile, splits):
    """Split-K (deterministic slice-ordered reduction + epilogue) vs torch, incl. the in-place
    residual of the HRNet fuse chain (res aliases out)."""
    g = torch.Generator().manual_seed(cin + 13 * splits)
    B = 16
    conv = nn.Conv2d(cin, cout, 3, 1, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(0.05 * torch.randn(conv.weight.shape, generator=g))
    bn = _bn(cout, g)
    x = torch.randn(B, cin, H, H, generator=g)
    res = torch.randn(B, cout, H, H, generator=g)
    ref = torch.relu(bn(conv(x)) + res).detach()
    spec = ops.make_conv(conv, bn, dev)
    xa = _nhwc(x, dev)
    out = _nhwc(res, dev)  # accumulate in place: out = relu(conv(x) + out)
    M, N = B * H * H, ops.pad4(cout)
    ws = torch.empty(splits * M * N, device=dev)
    ops.conv2d(xa, spec, out, res=out, relu=True, tile=tile, splits=splits, ws=ws)
    torch.cuda.synchronize()
    got = out.t[..., :cout].permute(0, 3, 1, 2).cpu()
    torch.testing.assert_close(got, ref, **TOL)
    # same result, bit for bit, on a second run (no atomics)
    out2 = _nhwc(res, dev)
    ops.conv2d(xa, spec, out2, res=out2, relu=True, tile=tile, splits=splits, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(out2.t, out.t)


@pytest.mark.parametrize("cin,cout,k,p,op,H", [(398, 128, 4, 1, 0, 30), (128, 128, 3, 1, 1, 30), (20, 12, 4, 1, 0, 7)])
def test_convT(dev, cin, cout, k, p, op, H):
    g = torch.Generator().manual_seed(11 + k)
    convT = nn.ConvTranspose2d(cin, cout, k, 2, p, output_padding=op, bias=False)
    with torch.no_grad():
        convT.weight.copy_(0.05 * torch.randn(convT.weight.shape, generator=g))
    bn = _bn(cout, g)
    x = torch.randn(2, cin, H, H, generator=g)
    ref = torch.relu(bn(convT(x))).detach()
    spec = ops.make_convT(convT, bn, dev)
    xa = _nhwc(x, dev)
    out = ops.new_act(2, 2 * H, 2 * H, cout, dev)
    ops.conv2d(xa, spec, out, relu=True)
    torch.cuda.synchronize()
    got = out.t[..., :cout].permute(0, 3, 1, 2).cpu()
    torch.testing.assert_close(got, ref, **TOL)


@pytest.mark.parametrize("cin,cout,k,s,H,tile,splits,kind", [
    (64, 64, 3, 2, 60, 2, 1, "conv"), (18, 36, 3, 1, 15, 6, 1, "conv"), (270, 132, 3, 1, 17, 8, 1, "conv"),
    (144, 144, 3, 1, 4, 8, 10, "conv"), (36, 20, 1, 1, 13, 7, 1, "conv"), (130, 64, 4, 1, 9, 1, 1, "convT"),
    (128, 72, 3, 1, 7, 4, 1, "convT"), (40, 132, 3, 1, 11, 3, 1, "conv"), (20, 24, 3, 2, 23, 5, 1, "conv")])
def test_conv_x3(dev, cin, cout, k, s, H, tile, splits, kind):
    """krrn_conv2d_x3_f32 (split-bf16 operands): the f32 tolerance against torch, within f32
    accumulation noise of the f32 kernel, pad channels zero; odd sizes, residual, split-K,
    transposed-conv parity classes."""
    g = torch.Generator().manual_seed(cin * 3 + cout + k)
    B = 3
    if kind == "conv":
        conv = nn.Conv2d(cin, cout, k, s, (k - 1) // 2, bias=True)
    else:
        conv = nn.ConvTranspose2d(cin, cout, k, 2, 1, output_padding=1 if k == 3 else 0, bias=True)
    with torch.no_grad():
        conv.weight.copy_(0.05 * torch.randn(conv.weight.shape, generator=g))
        conv.bias.copy_(0.1 * torch.randn(cout, generator=g))
    bn = _bn(cout, g)
    x = torch.randn(B, cin, H, H, generator=g)
    y = bn(conv(x))
    res = torch.randn(y.shape, generator=g)
    ref = torch.relu(y + res).detach()
    spec = ops.make_conv(conv, bn, dev) if kind == "conv" else ops.make_convT(conv, bn, dev)
    xa = _nhwc(x, dev)
    Ho, Wo = ref.shape[2:]
    ra = _nhwc(res, dev)
    outs = []
    for x3 in (False, True):
        out = ops.new_act(B, Ho, Wo, cout, dev, cs=ops.pad4(cout) + 4)
        out.t[..., :ops.pad4(cout)] = float("nan")
        ws = torch.empty(splits * B * Ho * Wo * ops.pad4(cout), device=dev) if splits > 1 else None
        ops.conv2d(xa, spec, out, res=ra, relu=True, tile=tile, splits=splits, ws=ws, x3=x3)
        torch.cuda.synchronize()
        outs.append(out.t.clone())
    f32, x3 = (o[..., :cout].permute(0, 3, 1, 2).cpu() for o in outs)
    torch.testing.assert_close(x3, ref, **TOL)
    torch.testing.assert_close(x3, f32, rtol=1e-5, atol=2e-6 * float(ref.abs().max()))
    assert torch.count_nonzero(outs[1][..., ops.pad4(cout):]).item() == 0


@pytest.mark.parametrize("cout", [70, 3, 130])
def test_conv_nchw_out(dev, cout):
    g = torch.Generator().manual_seed(5)
    conv = nn.Conv2d(128, cout, 1, 1, 0, bias=True)
    with torch.no_grad():
        conv.weight.copy_(0.05 * torch.randn(conv.weight.shape, generator=g))
        conv.bias.copy_(0.1 * torch.randn(cout, generator=g))
    x = torch.randn(2, 128, 37, 37, generator=g)
    ref = conv(x).detach()
    spec = ops.make_conv(conv, None, dev)
    xa = _nhwc(x, dev)
    out = torch.empty(2, cout, 37, 37, device=dev)
    ops.conv2d_nchw(xa, spec, out, n_store=cout)
    torch.cuda.synchronize()
    torch.testing.assert_close(out.cpu(), ref, **TOL)


def test_gemm_bias2(dev):
    g = torch.Generator().manual_seed(9)
    M, K, N, per = 3000, 1280, 1024, 1000
    a = torch.randn(M, K, generator=g)
    w = 0.03 * torch.randn(N, K, generator=g)
    b = 0.1 * torch.randn(N, generator=g)
    b2 = torch.randn(3, N, generator=g)
    ref = torch.relu(a @ w.t() + b + b2.repeat_interleave(per, 0))
    spec = ops.make_linear(w, b, None, dev)
    out = torch.zeros(M, N, device=dev)
    ops.gemm(a.to(dev), K, 0, M, spec, out, N, 0, relu=True, bias2=b2.to(dev), b2_div=per)
    torch.cuda.synchronize()
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("tile,x3", [(6, False), (8, False), (1, False), (6, True), (8, True), (1, True)])
def test_conv_group_matches_single(dev, tile, x3):
    """krrn_conv2d_group_f32 (x3: krrn_conv2d_group_x3_f32) over the four HRNet-W18 branch shapes
    (incl. split-K members) gives bit-identical results to the same problems launched one by one."""
    import ctypes
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, add_conv_group, conv_splits, Plan, ptr
    g = torch.Generator().manual_seed(5)
    shapes = [(20, 30), (36, 15), (72, 8), (144, 4)]
    B = 16
    plan = Plan(dev)
    probs, outs, refs = [], [], []
    for c, H in shapes:
        conv = nn.Conv2d(c, c, 3, 1, 1, bias=False)
        with torch.no_grad():
            conv.weight.copy_(0.05 * torch.randn(conv.weight.shape, generator=g))
        bn = _bn(c, g)
        x = torch.randn(B, c, H, H, generator=g)
        res = torch.randn(B, c, H, H, generator=g)
        spec = ops.make_conv(conv, bn, dev)
        xa, ra = _nhwc(x, dev), _nhwc(res, dev)
        out = ops.new_act(B, H, H, c, dev)
        ref = ops.new_act(B, H, H, c, dev)
        M, K = B * H * H, spec.cin_p * 9
        sp = conv_splits(M, ops.pad4(c), K, tile)
        ws = torch.empty(max(1, sp) * M * ops.pad4(c), device=dev)
        ops.conv2d(xa, spec, ref, res=ra, relu=True, tile=tile, splits=sp, ws=ws, x3=x3)
        w = ops.conv_weights_x3(spec.wt[0]) if x3 else spec.wt[0]
        probs.append(dict(x=ptr(xa.t), x_cs=xa.cs, x_co=0, B=B, Hi=H, Wi=H, cin_p=spec.cin_p, Hg=H, Wg=H, in_s=1,
                          taps=spec.taps[0], wt=ptr(w), N=ops.pad4(c), n_store=ops.pad4(c),
                          scale=ptr(spec.scale), bias=ptr(spec.bias), res=ptr(ra.t), res_cs=ra.cs, res_co=0,
                          out=ptr(out.t), out_cs=out.cs, out_co=0, Ho=H, Wo=H, relu=True, cin=c, cout=c))
        outs.append(out)
        refs.append((ref, spec, xa, ra, w))
    add_conv_group(plan, probs, tile=tile, x3=x3)
    plan.run({})
    torch.cuda.synchronize()
    for out, (ref, *_keep) in zip(outs, refs):
        assert torch.equal(out.t, ref.t)


@pytest.mark.parametrize("cin,k,op,x3,q", [(272, 4, 0, True, 16), (128, 3, 1, True, 16), (272, 4, 0, False, 16),
                                           (128, 3, 1, True, 32), (40, 4, 0, True, 8)])
def test_convT_group_kchunk(dev, cin, k, op, x3, q):
    """The grouped transposed conv with channel-chunk-major k (krrn_conv_desc.k_chunk = q, weights
    through ops.kchunk_weights) vs torch fp32 and vs the tap-major launch (same products, another
    summation order: within f32 accumulation noise)."""
    from pose_estimation_amd.runtime import add_conv_group, Plan, ptr
    g = torch.Generator().manual_seed(cin + k + q)
    B, H, cout = 3, 13, 128
    convT = nn.ConvTranspose2d(cin, cout, k, 2, 1, output_padding=op, bias=False)
    with torch.no_grad():
        convT.weight.copy_(0.05 * torch.randn(convT.weight.shape, generator=g))
    bn = _bn(cout, g)
    x = torch.randn(B, cin, H, H, generator=g)
    ref = torch.relu(bn(convT(x))).detach()
    spec = ops.make_convT(convT, bn, dev)
    xa = _nhwc(x, dev)
    Ho, Wo = ref.shape[2:]
    got = []
    for kc in (0, q):
        out = ops.new_act(B, Ho, Wo, cout, dev)
        out.t.fill_(float("nan"))
        plan = Plan(dev)
        probs, keep = [], []
        for w, taps, (ooy, oox) in zip(spec.wt, spec.taps, spec.cls_off):
            w = ops.kchunk_weights(w, len(taps), spec.cin_p, kc) if kc else w
            w = ops.conv_weights_x3(w) if x3 else w
            keep.append(w)
            probs.append(dict(x=ptr(xa.t), x_cs=xa.cs, x_co=0, B=B, Hi=H, Wi=H, cin_p=spec.cin_p, Hg=H, Wg=H, in_s=1,
                              taps=taps, wt=ptr(w), N=cout, n_store=cout, scale=ptr(spec.scale), bias=ptr(spec.bias),
                              out=ptr(out.t), out_cs=out.cs, out_co=0, Ho=Ho, Wo=Wo, osy=2, osx=2, ooy=ooy, oox=oox,
                              relu=True, cin=cin, cout=cout, k_chunk=kc))
        add_conv_group(plan, probs, tile=1 if x3 else 8, x3=x3)
        plan.run({})
        torch.cuda.synchronize()
        got.append(out.t[..., :cout].permute(0, 3, 1, 2).cpu())
    torch.testing.assert_close(got[1], ref, **TOL)
    torch.testing.assert_close(got[1], got[0], rtol=1e-5, atol=2e-6 * float(ref.abs().max()))


@pytest.mark.parametrize("x3,tile", [(False, 8), (False, 6), (True, 1), (True, 8)])
def test_conv_epilogue_float4_and_scalar(dev, x3, tile):
    """The implicit-GEMM conv's NHWC epilogue: float4 channel runs through the per-wave LDS square
    when every operand is 16-B aligned (out_co = 0), the per-element form otherwise (out_co = 1,
    res_co = 1); both with a per-crop bias2, a residual and a row tail, vs torch fp32 and each other."""
    g = torch.Generator().manual_seed(11 + tile + 5 * x3)
    B, cin, cout, H = 3, 36, 40, 13
    conv = nn.Conv2d(cin, cout, 3, 1, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(0.05 * torch.randn(conv.weight.shape, generator=g))
    bn = _bn(cout, g)
    x = torch.randn(B, cin, H, H, generator=g)
    res = torch.randn(B, cout, H, H, generator=g)
    b2 = torch.randn(B, cout, generator=g)
    ref = torch.relu(bn(conv(x)) + b2[:, :, None, None] + res).detach()
    spec = ops.make_conv(conv, bn, dev, cin_p=ops.pad4(cin))
    xa = _nhwc(x, dev)
    b2d = b2.to(dev).contiguous()
    got = []
    for co in (0, 1):
        ra = _nhwc(res, dev, cs=cout + 8, co=co)
        out = ops.new_act(B, H, H, cout, dev, cs=cout + 8)
        out.t.fill_(7.0)
        o = out.slice(co, cout)
        ops.conv2d(xa, spec, o, res=ra, relu=True, bias2=b2d, b2_div=H * H, tile=tile, x3=x3)
        torch.cuda.synchronize()
        t = out.t.cpu()
        got.append(t[..., co:co + cout].permute(0, 3, 1, 2))
        torch.testing.assert_close(got[-1], ref, **TOL)
        assert torch.all(t[..., :co] == 7.0) and torch.all(t[..., co + cout:] == 7.0)
    torch.testing.assert_close(got[0], got[1], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("cin,cout,H,W,co", [(128, 128, 30, 30, 0), (64, 72, 17, 23, 4), (272, 272, 15, 15, 0),
                                             (36, 40, 9, 8, 8), (20, 132, 61, 35, 0), (128, 64, 120, 120, 0)])
def test_conv3x3_winograd(dev, cin, cout, H, W, co):
    """Fused Winograd F(2x2,3x3) on split-bf16 operands (krrn_conv3x3_wino_x3_f32; odd sizes,
    channel-offset input, residual) vs torch fp32 conv (TOL) and vs an f64 conv + BN + residual + ReLU:
    max |err| <= 1.02516e-6 max |ref|. The bound is twice the largest ratio measured on the commit before
    the f32-MFMA Winograd (krrn_conv3x3_wino_f32, until then this test's cross-check) was removed, over
    both kernels and these six shapes (MI355X, fixed seeds; the factor 2 covers contraction and ordering
    changes between compiler versions):
        shape (cin, cout, H, W, co)     f32 kernel    split kernel
        (128, 128,  30,  30, 0)         5.1258e-07    4.0222e-07
        ( 64,  72,  17,  23, 4)         2.7275e-07    2.2781e-07
        (272, 272,  15,  15, 0)         4.7671e-07    4.9079e-07
        ( 36,  40,   9,   8, 8)         1.7520e-07    1.7275e-07
        ( 20, 132,  61,  35, 0)         1.6174e-07    1.5490e-07
        (128,  64, 120, 120, 0)         4.4906e-07    4.6666e-07
    F(4x4)'s larger transform constants get 1e-5 (test_conv3x3_winograd4)."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, ptr
    g = torch.Generator().manual_seed(cin + cout + H)
    B = 3
    conv = nn.Conv2d(cin, cout, 3, 1, 1, bias=True)
    with torch.no_grad():
        conv.weight.copy_(0.05 * torch.randn(conv.weight.shape, generator=g))
        conv.bias.copy_(0.1 * torch.randn(cout, generator=g))
    bn = _bn(cout, g)
    x = torch.randn(B, cin, H, W, generator=g)
    res = torch.randn(B, cout, H, W, generator=g)
    ref = torch.relu(bn(conv(x)) + res).detach()
    with torch.no_grad():
        s64 = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        y64 = F.conv2d(x.double(), conv.weight.double(), conv.bias.double(), padding=1)
        ref64 = torch.relu((y64 - bn.running_mean.double()[:, None, None]) * s64[:, None, None]
                           + bn.bias.double()[:, None, None] + res.double())
    cs = ops.pad4(cin) + co + 4
    xa = _nhwc(x, dev, cs=cs, co=co)
    spec = ops.make_conv(conv, bn, dev, cin_p=ops.pad4(cin))
    U3 = ops.wino_weights_x3(ops.wino_weights(conv, dev, cin_p=ops.pad4(cin)))
    ra = _nhwc(res, dev)
    out = ops.new_act(B, H, W, cout, dev, cs=ops.pad4(cout) + 4)
    np_ = ops.pad4(cout)
    L = _lib.lib()
    out.t.fill_(float("nan"))
    out.t[..., np_:] = 0.0
    _lib.check(L.krrn_conv3x3_wino_x3_f32(ptr(xa.t), xa.cs, xa.co, B, H, W, ops.pad4(cin), ptr(U3), np_, np_,
                                          ptr(spec.scale), ptr(spec.bias), ptr(ra.t), ra.cs, 0, ptr(out.t),
                                          out.cs, 0, 1, P(torch.cuda.current_stream().cuda_stream)), "wino_x3")
    torch.cuda.synchronize()
    got3 = out.t[..., :cout].permute(0, 3, 1, 2).cpu()
    torch.testing.assert_close(got3, ref, **TOL)
    assert torch.count_nonzero(out.t[..., np_:]).item() == 0
    err = float((got3.double() - ref64).abs().max() / ref64.abs().max())
    assert err <= 2 * 5.1258e-07, err


@pytest.mark.parametrize("cin,k,op,H,W,ci,co,relu,bias", [
    (272, 4, 0, 30, 30, 0, 0, 1, False),  # the folded deconv (myhrnet.py:314-326)
    (128, 3, 1, 30, 30, 0, 0, 1, False),  # XYZNet's first layer (krrn.py:47-49)
    (64, 4, 0, 13, 37, 4, 8, 0, True),    # ragged: rows not a multiple of 4, two 32-column blocks
    (8, 3, 1, 5, 3, 0, 4, 1, True),       # one chunk, a tiny grid (halo everywhere)
    (24, 2, 0, 9, 33, 0, 0, 1, False)])   # kernel 2: one tap per class, 2H - 2 output rows
def test_convT_s2(dev, cin, k, op, H, W, ci, co, relu, bias):
    """Stride-2 transposed conv, all four parity classes per block (krrn_convT_s2_x3_f32, convt.hip),
    channel-offset input / output, BN (+ conv bias), ReLU: vs torch fp32 (TOL), vs an f64 transposed
    conv (max |err| <= 2e-6 max |ref|: the split-bf16 products at f32 accuracy), and vs the grouped
    implicit GEMM it replaces (krrn_conv2d_group_x3_f32: same products, another summation order).
    NaN-filled output: every pixel and channel it owns is written, the channels past it untouched."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, add_conv_group, Plan, ptr
    g = torch.Generator().manual_seed(cin + k + H + W)
    B, cout = 3, 128
    convT = nn.ConvTranspose2d(cin, cout, k, 2, 1, output_padding=op, bias=bias)
    with torch.no_grad():
        convT.weight.copy_(torch.randn(convT.weight.shape, generator=g) / (2.0 * cin ** 0.5))
        if bias:
            convT.bias.copy_(0.1 * torch.randn(cout, generator=g))
    bn = _bn(cout, g)
    x = torch.randn(B, cin, H, W, generator=g)
    act = torch.relu if relu else (lambda t: t)
    ref = act(bn(convT(x))).detach()
    with torch.no_grad():
        s64 = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        y64 = F.conv_transpose2d(x.double(), convT.weight.double(), convT.bias.double() if bias else None,
                                 stride=2, padding=1, output_padding=op)
        ref64 = act((y64 - bn.running_mean.double()[:, None, None]) * s64[:, None, None]
                    + bn.bias.double()[:, None, None])
    Ho, Wo = ref.shape[2:]
    xa = _nhwc(x, dev, cs=cin + ci + 4, co=ci)
    spec = ops.make_convT(convT, bn, dev)
    U3, table = ops.convT_weights_x3(spec)
    out = ops.new_act(B, Ho, Wo, cout, dev, cs=cout + co + 4)
    out.t.fill_(float("nan"))
    _lib.check(_lib.lib().krrn_convT_s2_x3_f32(ptr(xa.t), xa.cs, xa.co, B, H, W, spec.cin_p, table, ptr(U3), cout,
                                               ptr(spec.scale), ptr(spec.bias), relu, ptr(out.t), out.cs, co, Ho,
                                               Wo, P(torch.cuda.current_stream().cuda_stream)), "convT_s2")
    torch.cuda.synchronize()
    t = out.t.cpu()
    assert torch.isnan(t[..., :co]).all() and torch.isnan(t[..., co + cout:]).all()
    got = t[..., co:co + cout].permute(0, 3, 1, 2)
    assert not torch.isnan(got).any()
    torch.testing.assert_close(got, ref, **TOL)
    err = float((got.double() - ref64).abs().max() / ref64.abs().max())
    assert err <= 2e-6, err
    if (Ho, Wo) != (2 * H, 2 * W):
        return  # the grouped launch below covers the whole 2H x 2W class grid (the model's convTs)
    # the grouped implicit GEMM on the same input
    grp = ops.new_act(B, Ho, Wo, cout, dev)
    plan, keep = Plan(dev), []
    probs = []
    for w, taps, (ooy, oox) in zip(spec.wt, spec.taps, spec.cls_off):
        keep.append(ops.conv_weights_x3(w))
        probs.append(dict(x=ptr(xa.t), x_cs=xa.cs, x_co=xa.co, B=B, Hi=H, Wi=W, cin_p=spec.cin_p, Hg=H, Wg=W, in_s=1,
                          taps=taps, wt=ptr(keep[-1]), N=cout, n_store=cout, scale=ptr(spec.scale),
                          bias=ptr(spec.bias), out=ptr(grp.t), out_cs=grp.cs, out_co=0, Ho=Ho, Wo=Wo, osy=2, osx=2,
                          ooy=ooy, oox=oox, relu=bool(relu), cin=cin, cout=cout))
    add_conv_group(plan, probs, tile=1, x3=True)
    plan.run({})
    torch.cuda.synchronize()
    torch.testing.assert_close(got, grp.t[..., :cout].permute(0, 3, 1, 2).cpu(), rtol=1e-5,
                               atol=2e-6 * float(ref.abs().max()))


@pytest.mark.parametrize("cin,cout,H,W,co,relu", [(128, 128, 32, 40, 0, 1), (64, 72, 33, 37, 4, 1),
                                                  (96, 128, 35, 64, 8, 0), (128, 64, 60, 60, 0, 1),
                                                  (128, 128, 120, 120, 0, 1)])
def test_conv3x3_winograd4(dev, cin, cout, H, W, co, relu):
    """Fused Winograd F(4x4,3x3) on split-bf16 operands (krrn_conv3x3_wino4_x3_f32): ragged tiles (H, W
    not multiples of 4 or of a block's 64 x 8 pixels), channel-offset input / output, residual, BN.
    vs torch fp32 (TOL) and vs an f64 conv: max |err| <= 1e-5 max |ref|. F(4x4)'s transform constants
    (up to 25 in B^T B, 8 in A^T, 1/24 in G) make its rounding error ~6x F(2x2)'s (RMS 7.4e-7 vs 1.2e-7
    of max|ref| in the round-5 CPU study); the f32 conv's own error is ~3e-7."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, ptr
    g = torch.Generator().manual_seed(cin + cout + H + W)
    B = 3 if H * W < 10000 else 2
    conv = nn.Conv2d(cin, cout, 3, 1, 1, bias=True)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (3.0 * cin ** 0.5))
        conv.bias.copy_(0.1 * torch.randn(cout, generator=g))
    bn = _bn(cout, g)
    x = torch.relu(torch.randn(B, cin, H, W, generator=g))
    res = torch.randn(B, cout, H, W, generator=g)
    act = torch.relu if relu else (lambda t: t)
    ref = act(bn(conv(x)) + res).detach()
    with torch.no_grad():
        s64 = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps))
        y64 = F.conv2d(x.double(), conv.weight.double(), conv.bias.double(), padding=1)
        ref64 = act((y64 - bn.running_mean.double()[:, None, None]) * s64[:, None, None]
                    + bn.bias.double()[:, None, None] + res.double())
    cs = ops.pad4(cin) + co + 4
    xa = _nhwc(x, dev, cs=cs, co=co)
    spec = ops.make_conv(conv, bn, dev, cin_p=ops.pad4(cin))
    U3 = ops.wino_weights_x3(ops.wino4_weights(conv, dev, cin_p=ops.pad4(cin)))
    ra = _nhwc(res, dev)
    np_ = ops.pad4(cout)
    out = ops.new_act(B, H, W, cout, dev, cs=np_ + co + 4)
    out.t.fill_(7.0)
    L = _lib.lib()
    _lib.check(L.krrn_conv3x3_wino4_x3_f32(ptr(xa.t), xa.cs, xa.co, B, H, W, ops.pad4(cin), ptr(U3), np_, np_,
                                           ptr(spec.scale), ptr(spec.bias), ptr(ra.t), ra.cs, 0, ptr(out.t), out.cs,
                                           co, relu, P(torch.cuda.current_stream().cuda_stream)), "wino4")
    torch.cuda.synchronize()
    t = out.t.cpu()
    got = t[..., co:co + cout].permute(0, 3, 1, 2)
    torch.testing.assert_close(got, ref, **TOL)
    err = float((got.double() - ref64).abs().max() / ref64.abs().max())
    assert err <= 1e-5, err
    assert torch.all(t[..., :co] == 7.0) and torch.all(t[..., co + np_:] == 7.0)


@pytest.mark.parametrize("cin,cout,H,W,co,p1,with_res,f4", [
    (128, 128, 120, 120, 0, 3, False, False), (64, 72, 17, 23, 4, 4, True, False), (20, 132, 9, 8, 0, 1, True, False),
    (36, 40, 7, 9, 8, 2, False, False), (128, 128, 120, 120, 0, 3, False, True), (64, 72, 33, 37, 4, 4, True, True),
    (96, 132, 40, 35, 8, 1, True, True)])
def test_conv3x3_winograd_head(dev, cin, cout, H, W, co, p1, with_res, f4):
    """krrn_conv3x3_wino_x3_head_f32 / krrn_conv3x3_wino4_x3_head_f32 (f4): the last head conv (+ BN,
    residual, ReLU) and a <= 4-output 1x1 + bias in one launch (NML's 120-px conv + nml_final at B = 3,
    ragged 64-channel blocks and tiles, odd maps) vs torch fp32; the NCHW channels past p1 are not
    written."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, ptr
    g = torch.Generator().manual_seed(cin + 3 * cout + H + p1)
    B = 3
    conv = nn.Conv2d(cin, cout, 3, 1, 1, bias=False)
    final = nn.Conv2d(cout, p1, 1)
    with torch.no_grad():
        conv.weight.copy_(0.05 * torch.randn(conv.weight.shape, generator=g))
        final.weight.copy_(0.1 * torch.randn(final.weight.shape, generator=g))
        final.bias.copy_(0.1 * torch.randn(p1, generator=g))
    bn = _bn(cout, g)
    x = torch.randn(B, cin, H, W, generator=g)
    res = torch.randn(B, cout, H, W, generator=g) if with_res else None
    h = bn(conv(x))
    ref = final(torch.relu(h + res if with_res else h)).detach()
    xa = _nhwc(x, dev, cs=ops.pad4(cin) + co + 4, co=co)
    spec = ops.make_conv(conv, bn, dev, cin_p=ops.pad4(cin))
    U3 = ops.wino_weights_x3((ops.wino4_weights if f4 else ops.wino_weights)(conv, dev, cin_p=ops.pad4(cin)))
    np_ = ops.pad4(cout)
    w1 = torch.zeros(4, np_, device=dev)
    w1[:p1, :cout] = final.weight.detach().reshape(p1, cout).to(dev)
    b1 = final.bias.detach().to(dev).contiguous()
    ra = _nhwc(res, dev) if with_res else None
    part = torch.full((((np_ + 63) // 64) * B * H * W * 4,), float("nan"), device=dev)
    out = torch.full((B, p1 + 1, H, W), -7.0, device=dev)
    L = _lib.lib()
    fn = L.krrn_conv3x3_wino4_x3_head_f32 if f4 else L.krrn_conv3x3_wino_x3_head_f32
    _lib.check(fn(ptr(xa.t), xa.cs, xa.co, B, H, W, ops.pad4(cin), ptr(U3), np_,
                                               ptr(spec.scale), ptr(spec.bias), ptr(ra.t) if ra else ptr(None),
                                               ra.cs if ra else 0, 0, 1, ptr(w1), ptr(b1), p1, ptr(part), ptr(out),
                                               p1 + 1, P(torch.cuda.current_stream().cuda_stream)), "wino_head")
    torch.cuda.synchronize()
    got = out.cpu()
    torch.testing.assert_close(got[:, :p1], ref, **TOL)
    assert torch.all(got[:, p1] == -7.0)


@pytest.mark.parametrize("B,cin,cout,H,W,co,nw,ks,k,st", [
    (3, 20, 18, 30, 30, 0, 2, 1, 3, 1), (64, 144, 144, 4, 4, 0, 1, 4, 3, 1), (8, 36, 36, 15, 15, 4, 3, 2, 3, 1),
    (5, 72, 72, 8, 8, 0, 1, 4, 3, 1), (2, 12, 40, 7, 9, 0, 2, 2, 3, 1), (3, 4, 8, 5, 6, 0, 1, 1, 3, 1),
    # the fuse layers' stride-2 downsamples (odd and even sizes) and 1x1 projections
    (4, 20, 36, 30, 30, 0, 3, 2, 3, 2), (3, 36, 72, 15, 15, 0, 3, 4, 3, 2), (6, 72, 144, 8, 8, 4, 3, 4, 3, 2),
    (2, 20, 20, 7, 9, 0, 2, 1, 3, 2), (5, 36, 20, 15, 15, 0, 2, 2, 1, 1), (7, 144, 72, 4, 4, 4, 3, 4, 1, 1),
    (2, 72, 36, 8, 8, 0, 3, 1, 1, 1)])
def test_conv_small(dev, B, cin, cout, H, W, co, nw, ks, k, st):
    """LDS-staged direct conv (HRNet branch BasicBlocks, fuse-layer downsamples / projections):
    blocks spanning several images / rows, channel-offset input, residual + ReLU, partial
    16-channel tiles, vs torch fp32."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, ptr
    g = torch.Generator().manual_seed(cin * cout + H + 7 * k + st)
    conv = nn.Conv2d(cin, cout, k, st, (k - 1) // 2, bias=False)
    with torch.no_grad():
        conv.weight.copy_(0.1 * torch.randn(conv.weight.shape, generator=g))
    bn = _bn(cout, g)
    x = torch.randn(B, cin, H, W, generator=g)
    y = bn(conv(x)).detach()
    Ho, Wo = y.shape[2], y.shape[3]
    res = torch.randn(B, cout, Ho, Wo, generator=g)
    ref = torch.relu(y + res)
    cs = ops.pad4(cin) + co + 4
    xa = _nhwc(x, dev, cs=cs, co=co)
    spec = ops.make_conv(conv, bn, dev, cin_p=ops.pad4(cin))
    ra = _nhwc(res, dev)
    np_ = ops.pad4(cout)
    out = ops.new_act(B, Ho, Wo, cout, dev, cs=np_ + 4)
    out.t.fill_(float("nan"))
    out.t[..., np_:] = 0.0
    _lib.check(_lib.lib().krrn_conv_small_f32(ptr(xa.t), xa.cs, xa.co, B, H, W, ops.pad4(cin), ptr(spec.wt[0]), np_,
                                              np_, ptr(spec.scale), ptr(spec.bias), ptr(ra.t), ra.cs, 0, ptr(out.t),
                                              out.cs, 0, 1, k, st, nw, ks, P(torch.cuda.current_stream().cuda_stream)),
               "small conv")
    torch.cuda.synchronize()
    got = out.t[..., :cout].permute(0, 3, 1, 2).cpu()
    torch.testing.assert_close(got, ref, **TOL)
    assert torch.count_nonzero(out.t[..., np_:]).item() == 0


@pytest.mark.parametrize("B,HW,cin,cout,co,oc,Cx", [(3, 1000, 128, 72, 0, 0, 72), (2, 777, 128, 3, 0, 0, 3),
                                                   (4, 64, 20, 40, 4, 5, 50), (1, 130, 256, 80, 0, 0, 80),
                                                   (2, 1000, 128, 9, 0, 3, 12),
                                                   # the narrow (N <= 4) form: cin 32 / 64 / 128, odd HW
                                                   (3, 1000, 64, 2, 4, 1, 4), (2, 33, 32, 4, 0, 0, 4),
                                                   (5, 4800, 128, 3, 0, 0, 3), (1, 31, 128, 1, 0, 2, 3)])
def test_conv1x1_nchw(dev, B, HW, cin, cout, co, oc, Cx):
    """krrn_conv1x1_nchw_f32 (the heads' final 1x1 convs) vs torch fp32: ragged pixel tiles, K not a
    multiple of 16, channel-offset input and output."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, ptr
    g = torch.Generator().manual_seed(HW + cin + cout)
    W = HW // 2 if HW % 2 == 0 else HW
    H = HW // W
    conv = nn.Conv2d(cin, cout, 1, bias=True)
    with torch.no_grad():
        conv.weight.copy_(0.1 * torch.randn(conv.weight.shape, generator=g))
        conv.bias.copy_(torch.randn(cout, generator=g))
    x = torch.randn(B, cin, H, W, generator=g)
    ref = conv(x).detach()
    xa = _nhwc(x, dev, cs=ops.pad4(cin) + co + 4, co=co)
    spec = ops.make_conv(conv, None, dev, cin_p=ops.pad4(cin))
    out = torch.full((B, Cx, H, W), float("nan"), device=dev)
    _lib.check(_lib.lib().krrn_conv1x1_nchw_f32(ptr(xa.t), xa.cs, xa.co, B, HW, ops.pad4(cin), ptr(spec.wt[0]),
                                                ops.pad4(cout), cout, ptr(spec.scale), ptr(spec.bias), ptr(out), Cx, oc,
                                                P(torch.cuda.current_stream().cuda_stream)), "conv1x1 nchw")
    torch.cuda.synchronize()
    torch.testing.assert_close(out[:, oc:oc + cout].cpu(), ref, **TOL)
    if oc:
        assert torch.isnan(out[:, :oc]).all()


@pytest.mark.parametrize("B,HW,cout,co,oc,Cx", [(3, 1000, 72, 0, 0, 72), (2, 777, 72, 4, 0, 72), (4, 64, 40, 0, 5, 50),
                                                (1, 130, 80, 0, 0, 80), (2, 1000, 50, 8, 3, 60), (2, 4, 72, 0, 0, 72),
                                                (5, 4800, 72, 0, 0, 72)])
def test_conv1x1_nchw_x3(dev, B, HW, cout, co, oc, Cx):
    """krrn_conv1x1_nchw_x3_f32 (split-bf16 operands, the xyz head's final conv) vs torch fp32 and an
    f64 evaluation: ragged pixel tiles, odd HW (the scalar NCHW store), channel-offset input and
    output, nothing written outside the output slice."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, ptr
    cin = 128
    g = torch.Generator().manual_seed(HW + cout + 3)
    W = HW // 2 if HW % 2 == 0 else HW
    H = HW // W
    conv = nn.Conv2d(cin, cout, 1, bias=True)
    with torch.no_grad():
        conv.weight.copy_(0.1 * torch.randn(conv.weight.shape, generator=g))
        conv.bias.copy_(torch.randn(cout, generator=g))
    x = torch.randn(B, cin, H, W, generator=g)
    with torch.no_grad():
        ref = conv(x)
        ref64 = conv.double()(x.double())
    xa = _nhwc(x, dev, cs=cin + co + 4, co=co)
    spec = ops.make_conv(conv.float(), None, dev, cin_p=cin)
    w3 = ops.quad_weights_x3(spec.wt[0], ops.pad4(cout), cin)
    out = torch.full((B, Cx, H, W), float("nan"), device=dev)
    _lib.check(_lib.lib().krrn_conv1x1_nchw_x3_f32(ptr(xa.t), xa.cs, xa.co, B, HW, cin, ptr(w3), ops.pad4(cout), cout,
                                                   ptr(spec.scale), ptr(spec.bias), ptr(out), Cx, oc,
                                                   P(torch.cuda.current_stream().cuda_stream)), "conv1x1 nchw x3")
    torch.cuda.synchronize()
    got = out[:, oc:oc + cout].cpu()
    torch.testing.assert_close(got, ref, **TOL)
    err = float((got.double() - ref64).abs().max())
    err32 = float((ref.double() - ref64).abs().max())
    assert err <= max(4 * err32, 2e-6 * float(ref64.abs().max())), (err, err32)
    assert torch.isnan(out[:, :oc]).all() and torch.isnan(out[:, oc + cout:]).all()



