"""The F(4x4) Winograd conv reading the half-resolution source of UpsamplingBilinear2d(2) (bit 1 of the
`relu` flags of krrn_conv3x3_wino4_x3_f32 / krrn_conv3x3_wino4_x3_head_f32): the upsample folded into
the input transform, against an f64 interpolate + conv. Sizes are source -> conv size; a block of the
fused form is 32 x 1 tiles = 128 x 4 output pixels x 64 output channels, 8 input channels per chunk."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pose_estimation_amd import ops

pytestmark = pytest.mark.gpu

TOL = dict(rtol=2e-4, atol=2e-4)  # the conv tests' own (test_gpu_conv.py)


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


def _up(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


def _problem(B, cin, cout, Hs, Ws, with_res, relu):
    """Weights, input and the f64 / f32 references of relu?(bn(conv(up2(x))) (+ res))."""
    g = torch.Generator().manual_seed(cin + cout + Hs + Ws)
    conv = nn.Conv2d(cin, cout, 3, 1, 1, bias=True)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (3.0 * cin ** 0.5))
        conv.bias.copy_(0.1 * torch.randn(cout, generator=g))
    bn = _bn(cout, g)
    x = torch.relu(torch.randn(B, cin, Hs, Ws, generator=g))
    res = torch.randn(B, cout, 2 * Hs, 2 * Ws, generator=g) if with_res else None
    act = torch.relu if relu else (lambda t: t)
    with torch.no_grad():
        y32 = bn(conv(_up(x)))
        ref32 = act(y32 + res if with_res else y32)
        s64 = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        y64 = F.conv2d(_up(x.double()), conv.weight.double(), conv.bias.double(), padding=1)
        y64 = (y64 - bn.running_mean.double()[:, None, None]) * s64[:, None, None] + bn.bias.double()[:, None, None]
        ref64 = act(y64 + res.double() if with_res else y64)
    return conv, bn, x, res, ref32, ref64


def _run(dev, conv, bn, x, res, relu, ci, co, flags_up=True, xin=None):
    """One launch of krrn_conv3x3_wino4_x3_f32 into a sentinel-filled buffer: (status, whole buffer on
    the CPU). xin: the NHWC input Act (default: x at channel offset ci)."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, ptr
    B, cin, Hs, Ws = x.shape
    H, W = 2 * Hs, 2 * Ws
    cout = conv.out_channels
    xa = _nhwc(x, dev, cs=ops.pad4(cin) + ci + 4, co=ci) if xin is None else xin
    spec = ops.make_conv(conv, bn, dev, cin_p=ops.pad4(cin))
    U3 = ops.wino_weights_x3(ops.wino4_weights(conv, dev, cin_p=ops.pad4(cin)))
    ra = _nhwc(res, dev) if res is not None else None
    np_ = ops.pad4(cout)
    out = ops.new_act(B, H, W, cout, dev, cs=np_ + co + 4)
    out.t.fill_(7.0)
    st = _lib.lib().krrn_conv3x3_wino4_x3_f32(
        ptr(xa.t), xa.cs, xa.co, B, H, W, ops.pad4(cin), ptr(U3), np_, np_, ptr(spec.scale), ptr(spec.bias),
        ptr(ra.t) if ra else ptr(None), ra.cs if ra else 0, 0, ptr(out.t), out.cs, co,
        int(relu) | (2 if flags_up else 0), P(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, out.t.cpu()


def _check(t, co, cout, ref32, ref64):
    np_ = ops.pad4(cout)
    got = t[..., co:co + cout].permute(0, 3, 1, 2)
    err = float((got.double() - ref64).abs().max() / ref64.abs().max())
    print(f"fused: max|err| / max|ref64| = {err:.3e}")
    torch.testing.assert_close(got, ref32, **TOL)
    assert err <= 1e-5, err
    assert torch.all(t[..., :co] == 7.0) and torch.all(t[..., co + np_:] == 7.0)
    return err


# (B, cin, cout, Hs, Ws, input channel offset, output channel offset, residual, relu)
CASES = {
    # one block, one chunk (prologue-only transform, no ring reuse), window clipped on all four sides
    "one_block": (2, 8, 64, 3, 5, 0, 0, False, True),
    # two chunks, an 8-channel second n-block, odd source sizes
    "two_chunks": (3, 16, 72, 9, 17, 4, 4, True, True),
    # 130 px wide: one pixel column pair past a 128-px block; 22 rows: not a multiple of the block's 4;
    # 3 chunks (both ring slots reused), two full n-blocks; i1 == i0 at the last source row / column
    "block_edge": (2, 24, 128, 11, 65, 0, 0, True, False),
    # the workload's map
    "workload": (2, 128, 128, 60, 60, 0, 0, False, True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_wino4_up2(dev, name):
    """Fused upsample + conv vs the f64 interpolate + conv (max|err| <= 1e-5 max|ref|), vs the same in torch
    f32 (TOL), and the output slice's neighbours keep their fill."""
    from pose_estimation_amd import _lib
    B, cin, cout, Hs, Ws, ci, co, with_res, relu = CASES[name]
    conv, bn, x, res, ref32, ref64 = _problem(B, cin, cout, Hs, Ws, with_res, relu)
    st, t = _run(dev, conv, bn, x, res, relu, ci, co)
    _lib.check(st, "wino4 up2")
    _check(t, co, cout, ref32, ref64)


def test_wino4_up2_against_two_launches(dev):
    """Case two_chunks: the fused launch against krrn_resize_bilinear_f32 (align_corners) + the plain launch.
    Both are within 1e-5 max|ref| of the f64 reference, so they differ by at most twice that."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, ptr
    B, cin, cout, Hs, Ws, ci, co, with_res, relu = CASES["two_chunks"]
    conv, bn, x, res, ref32, ref64 = _problem(B, cin, cout, Hs, Ws, with_res, relu)
    st, tf = _run(dev, conv, bn, x, res, relu, ci, co)
    _lib.check(st, "wino4 up2")
    xa = _nhwc(x, dev, cs=ops.pad4(cin) + ci + 4, co=ci)
    up = ops.new_act(B, 2 * Hs, 2 * Ws, cin, dev, cs=ops.pad4(cin) + ci + 4).slice(ci, cin)
    _lib.check(_lib.lib().krrn_resize_bilinear_f32(
        ptr(xa.t), B, Hs, Ws, xa.cs, xa.co, ops.pad4(cin), ptr(up.t), 2 * Hs, 2 * Ws, up.cs, up.co, ptr(None), 0, 0,
        1, 0, P(torch.cuda.current_stream().cuda_stream)), "resize")
    st, t2 = _run(dev, conv, bn, x, res, relu, ci, co, flags_up=False, xin=up)
    _lib.check(st, "wino4")
    sl = slice(co, co + cout)
    gf, g2 = tf[..., sl].permute(0, 3, 1, 2).double(), t2[..., sl].permute(0, 3, 1, 2).double()
    m = float(ref64.abs().max())
    ef, e2, d = float((gf - ref64).abs().max()) / m, float((g2 - ref64).abs().max()) / m, float((gf - g2).abs().max()) / m
    print(f"fused err {ef:.3e}, two-launch err {e2:.3e}, fused - two-launch {d:.3e} (of max|ref64|)")
    assert ef <= 1e-5 and e2 <= 1e-5, (ef, e2)
    assert d <= 2e-5, d


@pytest.mark.parametrize("H,W", [(19, 34), (18, 33)])
def test_wino4_up2_odd_size_is_a_shape_error(dev, H, W):
    """Bit 1 with an odd H or W: KRRN_ESHAPE from both entry points, nothing written."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, ptr
    B, cin, cout = 1, 8, 64
    g = torch.Generator().manual_seed(H + W)
    conv = nn.Conv2d(cin, cout, 3, 1, 1, bias=False)
    x = _nhwc(torch.randn(B, cin, H, W, generator=g), dev)
    U3 = ops.wino_weights_x3(ops.wino4_weights(conv, dev, cin_p=cin))
    out = torch.full((B, H, W, cout), 7.0, device=dev)
    L = _lib.lib()
    s = P(torch.cuda.current_stream().cuda_stream)
    st = L.krrn_conv3x3_wino4_x3_f32(ptr(x.t), x.cs, 0, B, H, W, cin, ptr(U3), cout, cout, ptr(None), ptr(None),
                                     ptr(None), 0, 0, ptr(out), cout, 0, 3, s)
    assert st == -2  # KRRN_ESHAPE (include/krrn_hip.h)
    w1 = torch.zeros(4, cout, device=dev)
    part = torch.full((B * H * W * 4,), 7.0, device=dev)
    o2 = torch.full((B, 4, H, W), 7.0, device=dev)
    st2 = L.krrn_conv3x3_wino4_x3_head_f32(ptr(x.t), x.cs, 0, B, H, W, cin, ptr(U3), cout, ptr(None), ptr(None),
                                           ptr(None), 0, 0, 3, ptr(w1), ptr(None), 3, ptr(part), ptr(o2), 4, s)
    torch.cuda.synchronize()
    assert st2 == st
    assert torch.all(out == 7.0) and torch.all(part == 7.0) and torch.all(o2 == 7.0)


@pytest.mark.parametrize("cin,cout,Hs,Ws,co,p1,with_res", [(64, 72, 17, 19, 4, 4, True), (96, 132, 20, 18, 8, 1, True)])
def test_wino4_up2_head(dev, cin, cout, Hs, Ws, co, p1, with_res):
    """The head form on the half-resolution source: up2 -> conv + BN (+ residual) + ReLU -> a <= 4-output 1x1 +
    bias in one launch, vs torch f32 (TOL); the NCHW channels past p1 are not written."""
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, ptr
    g = torch.Generator().manual_seed(cin + 3 * cout + Hs + p1)
    B, H, W = 3, 2 * Hs, 2 * Ws
    conv = nn.Conv2d(cin, cout, 3, 1, 1, bias=False)
    final = nn.Conv2d(cout, p1, 1)
    with torch.no_grad():
        conv.weight.copy_(0.05 * torch.randn(conv.weight.shape, generator=g))
        final.weight.copy_(0.1 * torch.randn(final.weight.shape, generator=g))
        final.bias.copy_(0.1 * torch.randn(p1, generator=g))
    bn = _bn(cout, g)
    x = torch.randn(B, cin, Hs, Ws, generator=g)
    res = torch.randn(B, cout, H, W, generator=g) if with_res else None
    with torch.no_grad():
        h = bn(conv(_up(x)))
        ref = final(torch.relu(h + res if with_res else h))
    xa = _nhwc(x, dev, cs=ops.pad4(cin) + co + 4, co=co)
    spec = ops.make_conv(conv, bn, dev, cin_p=ops.pad4(cin))
    U3 = ops.wino_weights_x3(ops.wino4_weights(conv, dev, cin_p=ops.pad4(cin)))
    np_ = ops.pad4(cout)
    w1 = torch.zeros(4, np_, device=dev)
    w1[:p1, :cout] = final.weight.detach().reshape(p1, cout).to(dev)
    b1 = final.bias.detach().to(dev).contiguous()
    ra = _nhwc(res, dev) if with_res else None
    part = torch.full((((np_ + 63) // 64) * B * H * W * 4,), float("nan"), device=dev)
    out = torch.full((B, p1 + 1, H, W), -7.0, device=dev)
    _lib.check(_lib.lib().krrn_conv3x3_wino4_x3_head_f32(
        ptr(xa.t), xa.cs, xa.co, B, H, W, ops.pad4(cin), ptr(U3), np_, ptr(spec.scale), ptr(spec.bias),
        ptr(ra.t) if ra else ptr(None), ra.cs if ra else 0, 0, 1 | 2, ptr(w1), ptr(b1), p1, ptr(part), ptr(out),
        p1 + 1, P(torch.cuda.current_stream().cuda_stream)), "wino4 up2 head")
    torch.cuda.synchronize()
    got = out.cpu()
    torch.testing.assert_close(got[:, :p1], ref, **TOL)
    assert torch.all(got[:, p1] == -7.0)
