"""krrn_gcn_conv_f32 (Conv_layer, gcn3d.py:136-216) against a plain torch fp32 statement of the
same op. Neighbour lists: "local" ones (every neighbour within +-16 of the point's own index, as
pixel-ordered `choose` rows give) and fully random ones (the sampled levels), ragged n (not a
multiple of the block's 8 points), k = 10 / 7 / 16 (compile-time and runtime k paths). The second half
runs the same comparison through all three kernels (LDS-staged 3-D, generic LP = 32, generic LP = 128)
with and without Y: 9-D directions, C = 4 / 256 / 512, S above the staged kernel's bound, zero
directions, strided coordinate rows, and the output as a slice of a sentinel-filled buffer.
"""
import pytest
import torch

from pose_estimation_amd import _lib
from pose_estimation_amd.runtime import P, ptr
from tests.points_ref import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _torch_conv_layer(idx, v, dn, Y, S, C, bn_s, bn_b, relu):
    B, n, k = idx.shape
    bi = torch.arange(B)[:, None, None]
    d = v[bi, idx.long()] - v[:, :, None, :]                              # [B, n, k, 3]
    d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    theta = torch.relu(d @ dn)                                            # [B, n, k, S*C]
    sup = Y[bi, idx.long(), C:]                                           # [B, n, k, S*C]
    act = (theta * sup).max(dim=2).values.view(B, n, S, C).sum(dim=2)
    out = Y[:, :, :C] + act
    out = out * bn_s + bn_b
    return torch.relu(out) if relu else out


def _idx(B, n, k, mode, g):
    if mode == "local":
        w = 16
        off = torch.randint(-w, w + 1, (B, n, k), generator=g)
        base = torch.arange(n)[None, :, None]
        i = (base + off).clamp(0, n - 1)
        i = torch.where(i == base, (base + 1) % n, i)
    else:
        i = torch.randint(0, n, (B, n, k), generator=g)
    return i.to(torch.int32)


@pytest.mark.parametrize("B,n,k,mode", [(4, 1000, 10, "local"), (3, 250, 10, "local"), (2, 1000, 10, "random"),
                                        (2, 77, 7, "local"), (2, 300, 16, "local"), (1, 31, 10, "random")])
def test_gcn_conv_layer(dev, B, n, k, mode):
    S, C = 7, 128
    g = torch.Generator().manual_seed(n * 31 + k)
    idx = _idx(B, n, k, mode, g)
    v = torch.randn(B, n, 9, generator=g)                                 # fusion's [x y z nx ny nz r g b] rows
    dn = torch.randn(3, S * C, generator=g)
    dn = dn / dn.norm(dim=0, keepdim=True)
    Y = torch.randn(B, n, (S + 1) * C, generator=g)
    bn_s = 1 + 0.1 * torch.randn(C, generator=g)
    bn_b = 0.1 * torch.randn(C, generator=g)
    ref = _torch_conv_layer(idx, v[..., :3], dn, Y, S, C, bn_s, bn_b, True)
    L = _lib.lib()
    st = P(torch.cuda.current_stream().cuda_stream)
    d_idx, d_v, d_dn, d_Y = idx.to(dev), v.to(dev), dn.contiguous().to(dev), Y.to(dev)
    d_s, d_b = bn_s.to(dev), bn_b.to(dev)
    out = torch.full((B, n, C), float("nan"), device=dev)
    _lib.check(L.krrn_gcn_conv_f32(ptr(d_idx), n, k, ptr(d_v), n * 9, 9, 3, ptr(d_dn), S, C, ptr(d_Y), ptr(d_s),
                                   ptr(d_b), 1, ptr(out), n * C, C, B, st), "gcn conv")
    torch.cuda.synchronize()
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("B,n,k,has_y", [(4, 1000, 10, False), (2, 250, 8, True), (2, 77, 8, False),
                                         (3, 64, 10, True)])
def test_gcn_conv_surface_and_k8(dev, B, n, k, has_y):
    """Conv_surface (gcn3d.py:88-112: no Y, ReLU(max_k theta) summed over supports, no BN) and the
    k = 8 level-1 form of the test shapes, through the LDS-staged 3-D kernel."""
    S, C = 7, 128
    g = torch.Generator().manual_seed(n * 17 + k + int(has_y))
    idx = _idx(B, n, k, "local", g)
    v = torch.randn(B, n, 9, generator=g)
    dn = torch.randn(3, S * C, generator=g)
    dn = dn / dn.norm(dim=0, keepdim=True)
    bi = torch.arange(B)[:, None, None]
    if has_y:
        Y = torch.randn(B, n, (S + 1) * C, generator=g)
        ref = _torch_conv_layer(idx, v[..., :3], dn, Y, S, C, torch.ones(C), torch.zeros(C), False)
    else:
        Y = None
        d = v[bi, idx.long(), :3] - v[:, :, None, :3]
        d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        ref = torch.relu((d @ dn).max(dim=2).values).view(B, n, S, C).sum(dim=2)
    L = _lib.lib()
    st = P(torch.cuda.current_stream().cuda_stream)
    d_idx, d_v, d_dn = idx.to(dev), v.to(dev), dn.contiguous().to(dev)
    d_Y = Y.to(dev) if has_y else None
    out = torch.full((B, n, C), float("nan"), device=dev)
    _lib.check(L.krrn_gcn_conv_f32(ptr(d_idx), n, k, ptr(d_v), n * 9, 9, 3, ptr(d_dn), S, C, ptr(d_Y), P(0), P(0), 0,
                                   ptr(out), n * C, C, B, st), "gcn conv")
    torch.cuda.synchronize()
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------------
# The forms the cases above do not reach: 9-D directions (Conv_fuse_layer), the LP = 128 form
# (C >= 512), the generic kernel's channel loop (C = 256) and idle lanes (C = 4), S above the
# LDS-staged kernel's bound, run-time k, zero directions, strided v rows and an output slice of a
# wider sentinel-filled buffer (tests/points_ref.py's Guarded).
# ------------------------------------------------------------------------------------------------
def _torch_conv_surface(idx, v, dn, S, C, bn_s, bn_b, relu):
    B, n, k = idx.shape
    bi = torch.arange(B)[:, None, None]
    d = v[bi, idx.long()] - v[:, :, None, :]
    d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    out = torch.relu((d @ dn).max(dim=2).values).view(B, n, S, C).sum(dim=2)
    out = out * bn_s + bn_b
    return torch.relu(out) if relu else out


def _run_general(dev, idx, v, d, v_st, S, C, has_y, bn, relu, g):
    """Kernel output (guard-checked) and torch f32 reference for coordinates v [B][n][d] stored in rows
    of v_st floats; out is a C-wide slice at column 4 of rows C + 8 wide, batch stride with slack."""
    B, n, k = idx.shape
    dn = torch.randn(d, S * C, generator=g)
    dn = dn / dn.norm(dim=0, keepdim=True)
    Y = torch.randn(B, n, (S + 1) * C, generator=g) if has_y else None
    bn_s = 1 + 0.1 * torch.randn(C, generator=g) if bn else None
    bn_b = 0.1 * torch.randn(C, generator=g) if bn else None
    rs, rb = (bn_s, bn_b) if bn else (torch.ones(C), torch.zeros(C))
    if has_y:
        ref = _torch_conv_layer(idx, v, dn, Y, S, C, rs, rb, relu)
    else:
        ref = _torch_conv_surface(idx, v, dn, S, C, rs, rb, relu)
    slack = 5
    vbuf = torch.full((B, n * v_st + slack), float("nan"))
    vbuf[:, :n * v_st].view(B, n, v_st)[..., :d] = v
    if v_st > d:
        vbuf[:, :n * v_st].view(B, n, v_st)[..., d:] = 1e3  # the row's other columns must not be read
    out = Guarded(B, n, C, stride=C + 8, off=4, slack=16, device=dev)
    d_idx, d_v, d_dn = idx.to(dev), vbuf.to(dev), dn.contiguous().to(dev)
    d_Y = Y.to(dev) if has_y else None
    d_s, d_b = (bn_s.to(dev), bn_b.to(dev)) if bn else (None, None)
    _lib.call("krrn_gcn_conv_f32", ptr(d_idx), n, k, ptr(d_v), n * v_st + slack, v_st, d, ptr(d_dn), S, C, ptr(d_Y),
              ptr(d_s), ptr(d_b), int(relu), P(out.ptr_value()), out.bs, out.stride, B,
              P(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.result(), ref


def _check_general(dev, B, n, k, d, v_st, S, C, has_y, bn, relu, mode="random"):
    g = torch.Generator().manual_seed(((n * 31 + k) * 7 + C) * 3 + d + S)
    idx = _idx(B, n, k, mode, g)
    v = torch.randn(B, n, d, generator=g)
    got, ref = _run_general(dev, idx, v, d, v_st, S, C, has_y, bn, relu, g)
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("k", [1, 4, 7, 10, 16])  # 10 / 7 compile-time, the others run-time
@pytest.mark.parametrize("n", [1, 3, 62])  # odd n leaves half a block idle
def test_gcn_fuse_layer_9d_c512(dev, n, k):
    """Conv_fuse_layer (level 2): generic kernel, LP = 128, two points per block, with Y."""
    _check_general(dev, 2, n, k, 9, 9, 7, 512, True, bn=(k != 4), relu=(n != 3))


@pytest.mark.parametrize("k", [4, 10])
def test_gcn_fuse_layer_9d_c128(dev, k):
    """9-D directions through the generic kernel's LP = 32 form, with Y, ragged n."""
    _check_general(dev, 2, 77, k, 9, 12, 7, 128, True, bn=(k == 10), relu=True)


@pytest.mark.parametrize("has_y", [True, False], ids=["Y", "surface"])
@pytest.mark.parametrize("C", [4, 256, 512])
def test_gcn_generic_3d_channel_forms(dev, C, has_y):
    """d = 3 through the generic kernel: C = 4 (31 of 32 lanes without a channel), C = 256 (two trips of
    the channel loop, c += 4 LP), C = 512 (LP = 128), with and without Y; v rows of 3, 9 and 12 floats."""
    v_st = {4: 3, 256: 9, 512: 12}[C]
    _check_general(dev, 2, 77, 10, 3, v_st, 7, C, has_y, bn=has_y, relu=not has_y, mode="local")
    _check_general(dev, 2, 13, 5, 3, v_st, 7, C, has_y, bn=not has_y, relu=has_y)


@pytest.mark.parametrize("has_y", [True, False], ids=["Y", "surface"])
@pytest.mark.parametrize("S", [8, 9], ids=["S8-staged", "S9-generic"])
def test_gcn_support_bound(dev, S, has_y):
    """d = 3, C = 128, k = 10: S = 8 is the largest the LDS-staged kernel takes (kGcnSmax), S = 9 must go
    to the generic kernel; the same points and neighbour lists through both."""
    g = torch.Generator().manual_seed(99)
    idx = _idx(2, 77, 10, "local", g)
    v = torch.randn(2, 77, 3, generator=g)
    got, ref = _run_general(dev, idx, v, 3, 9, S, 128, has_y, True, True, g)
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("d,C,k", [(3, 128, 10), (3, 128, 8), (9, 512, 7), (3, 256, 5)],
                         ids=["staged-k10", "staged-k8", "generic-9d-LP128", "generic-3d-runtime-k"])
@pytest.mark.parametrize("has_y", [True, False], ids=["Y", "surface"])
def test_gcn_zero_direction(dev, d, C, k, has_y):
    """A neighbour equal to the point itself and a duplicated point: the zero direction takes the 1e-12
    clamp, so theta = 0 and nothing is NaN; a point whose every neighbour is itself has act = 0 exactly."""
    B, n, S = 2, 21, 7
    g = torch.Generator().manual_seed(d * 100 + C + k)
    idx = _idx(B, n, k, "random", g)
    idx[:, :, 0] = torch.arange(n, dtype=torch.int32)  # every point lists itself first
    idx[:, 5, :] = 5                                   # ... and point 5 only itself
    idx[:, 6, 1] = 7                                   # the duplicate of point 6
    v = torch.randn(B, n, d, generator=g)
    v[:, 7] = v[:, 6]
    got, ref = _run_general(dev, idx, v, d, 9 if d == 3 else 12, S, C, has_y, False, False, g)
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=2e-5)
    if not has_y:
        assert (got[:, 5] == 0).all()
