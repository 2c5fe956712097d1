"""The point branch's memory-bound kernels, each against its plain reference of tests/points_ref.py:
krrn_pool_max_f32, krrn_gather_rows_f32 (int32 / int64 index x float4 / scalar copies),
krrn_points_gather_f32, krrn_nchw_to_nhwc_f32, krrn_add_relu_f32 and the xyz half of
krrn_heads_select_f32 bit for bit against torch indexing in f32; krrn_gather2_add_f32,
krrn_tbase_tail_f32 and the normal half of krrn_heads_select_f32 against float64 within bounds counted
from their operations. Every output is a slice of a wider sentinel-filled buffer with guard rows
(points_ref.Guarded): the slice must equal the reference, everything outside it must stay untouched."""
import pytest
import torch

from pose_estimation_amd import _lib
from pose_estimation_amd.runtime import P, ptr
from tests import points_ref as R

pytestmark = pytest.mark.gpu


def _st():
    return P(torch.cuda.current_stream().cuda_stream)


def _gen(*key):
    seed = 0
    for x in key:
        seed = seed * 1009 + int(x)
    return torch.Generator().manual_seed(seed)


# ---- krrn_pool_max_f32 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 62, 250])
@pytest.mark.parametrize("C", [4, 128, 384])
@pytest.mark.parametrize("kk", [1, 4, 5])
def test_pool_max(dev, kk, C, nq):
    """Crop 0's features are all negative (a zero-seeded max would return 0), crop 1's mixed; row 0 of
    every crop repeats one neighbour. C = 128 reads a 128-wide slice at column 128 of 384-wide rows, as
    the fusion's per-branch pools do (f_st = 384, offset pointer)."""
    B, n = 2, 4 * nq + 3
    g = _gen(kk, C, nq)
    Fm = torch.randn(B, n, C, generator=g)
    Fm[0] = -Fm[0].abs() - 0.25
    nbr = torch.randint(0, n, (B, nq, kk), generator=g, dtype=torch.int32)
    nbr[:, 0] = n - 1
    f_st, f_off = (384, 128) if C == 128 else (C, 0)
    src = R.Guarded(B, n, C, stride=f_st, off=f_off, slack=12)
    src.fill(Fm)
    out = R.Guarded(B, nq, C, stride=C + 8, off=4, slack=20, device=dev)
    d_src, d_nbr = src.buf.to(dev), nbr.to(dev)
    _lib.call("krrn_pool_max_f32", ptr(d_nbr), nq, kk, P(d_src.data_ptr() + 4 * src.offset), src.bs, f_st, C,
              P(out.ptr_value()), out.bs, out.stride, B, _st())
    torch.cuda.synchronize()
    assert torch.equal(out.result(), R.pool_max_ref(Fm, nbr))


# ---- krrn_gather_rows_f32 ------------------------------------------------------------------------
# (id, idx64, idx shared (idx_bs = 0), width, src stride, src column offset, dst stride, dst column)
_GATHER = [
    ("i32-scalar-w3-src_st9-src+12B", 0, False, 3, 9, 2, 9, 3),  # (9 + 2) floats = 44 bytes = 12 mod 16
    ("i64-scalar-w9-src_st9-shared-idx", 1, True, 9, 9, 0, 12, 1),
    ("i32-scalar-w8-src+12B-falls-back", 0, False, 8, 12, 3, 16, 4),  # aligned strides, misaligned pointer
    ("i32-scalar-w8-dst_st9-falls-back", 0, True, 8, 8, 0, 9, 0),
    ("i64-scalar-w8-dst_st9-falls-back", 1, False, 8, 12, 4, 9, 1),
    ("i32-vec-w384-into-1280-at-512-shared-idx", 0, True, 384, 384, 0, 1280, 512),
    ("i32-vec-w384-into-1280-at-896", 0, False, 384, 388, 4, 1280, 896),
    ("i64-vec-w512-into-1280-at-512", 1, False, 512, 512, 0, 1280, 512),
    ("i64-vec-w384-into-1280-at-896-shared-idx", 1, True, 384, 768, 384, 1280, 896),
]


@pytest.mark.parametrize("case", _GATHER, ids=[c[0] for c in _GATHER])
def test_gather_rows(dev, case):
    name, idx64, shared, width, s_st, s_off, d_st, d_off = case
    B, n, nrows = 3, 37, 50
    g = _gen(width, d_st, idx64)
    vals = torch.randn(B, n, width, generator=g)
    idx = torch.randint(0, n, (1 if shared else B, nrows), generator=g, dtype=torch.int64 if idx64 else torch.int32)
    idx[:, :3] = torch.tensor([n - 1, 0, n - 1])
    src = R.Guarded(B, n, width, stride=s_st, off=s_off, slack=4 if width % 4 == 0 else 5)
    src.fill(vals)
    out = R.Guarded(B, nrows, width, stride=d_st, off=d_off, slack=4 if d_st % 4 == 0 else 7, device=dev)
    vec = width % 4 == 0 and s_st % 4 == 0 and d_st % 4 == 0 and s_off % 4 == 0 and d_off % 4 == 0
    assert vec == ("-vec-" in name)  # the float4 instance needs every stride, offset and pointer aligned
    d_src, d_idx = src.buf.to(dev), idx.to(dev)
    _lib.call("krrn_gather_rows_f32", ptr(d_idx), idx64, 0 if shared else nrows, nrows,
              P(d_src.data_ptr() + 4 * src.offset), src.bs, s_st, P(out.ptr_value()), out.bs, d_st, width, B, _st())
    torch.cuda.synchronize()
    assert torch.equal(out.result(), R.gather_rows_ref(vals, idx, B))


@pytest.mark.parametrize("width,d_st,d_off", [(1024, 1032, 4), (6, 7, 1)], ids=["vec", "scalar"])
def test_gather_rows_one_hot_column(dev, width, d_st, d_off):
    """The production one-hot form (krrn.py:132-138): idx64 = 1, idx_bs = 1, nrows = 1, src_bs = 0: crop b
    takes row cls[b] of one shared [ncls][width] table."""
    B, ncls = 5, 4
    g = _gen(width)
    table = torch.randn(1, ncls, width, generator=g)
    cls = torch.tensor([3, 0, 2, 2, 1], dtype=torch.int64)
    out = R.Guarded(B, 1, width, stride=d_st, off=d_off, slack=8 if d_st % 4 == 0 else 3, device=dev)
    d_t, d_cls = table.to(dev), cls.to(dev)
    _lib.call("krrn_gather_rows_f32", ptr(d_cls), 1, 1, 1, ptr(d_t), 0, width, P(out.ptr_value()), out.bs, d_st,
              width, B, _st())
    torch.cuda.synchronize()
    assert torch.equal(out.result(), R.gather_rows_ref(table, cls.view(B, 1), B))


# ---- krrn_gather2_add_f32 ------------------------------------------------------------------------
@pytest.mark.parametrize("bias2,relu", [(True, 1), (False, 0), (True, 0), (False, 1)],
                         ids=["bias2-relu", "plain", "bias2", "relu"])
@pytest.mark.parametrize("n", [1, 77, 1000])
@pytest.mark.parametrize("C", [4, 12, 256])
def test_gather2_add(dev, C, n, bias2, relu):
    """ia into the n / 16 level-2 rows, ib into the n / 4 level-1 rows, both tables slices of wider rows."""
    B, na, nb = 2, max(1, n // 16), max(1, n // 4)
    g = _gen(C, n, bias2, relu)
    A, Bm = torch.randn(B, na, C, generator=g), torch.randn(B, nb, C, generator=g)
    ia = torch.randint(0, na, (B, n), generator=g, dtype=torch.int32)
    ib = torch.randint(0, nb, (B, n), generator=g, dtype=torch.int32)
    ia[:, -1], ib[:, -1] = na - 1, nb - 1
    scale, bias = 1 + 0.2 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    b2 = torch.randn(B, C, generator=g) if bias2 else None
    ga, gb = R.Guarded(B, na, C, stride=C + 4, off=4, slack=8), R.Guarded(B, nb, C, stride=C + 8, off=0, slack=4)
    ga.fill(A)
    gb.fill(Bm)
    out = R.Guarded(B, n, C, stride=C + 12, off=8, slack=12, device=dev)
    d_a, d_b, d_ia, d_ib = ga.buf.to(dev), gb.buf.to(dev), ia.to(dev), ib.to(dev)
    d_s, d_c, d_b2 = scale.to(dev), bias.to(dev), (b2.to(dev) if bias2 else None)
    _lib.call("krrn_gather2_add_f32", ptr(d_ia), P(d_a.data_ptr() + 4 * ga.offset), ga.bs, ga.stride, ptr(d_ib),
              P(d_b.data_ptr() + 4 * gb.offset), gb.bs, gb.stride, n, C, ptr(d_s), ptr(d_c), ptr(d_b2), relu,
              P(out.ptr_value()), out.bs, out.stride, B, _st())
    torch.cuda.synchronize()
    ref, bound = R.gather2_add_ref(ia, A, ib, Bm, scale, bias, b2, relu)
    err = (out.result().double() - ref).abs()
    assert (err <= bound).all(), float((err / bound).max())


# ---- krrn_tbase_tail_f32 -------------------------------------------------------------------------
def _tail(dev, h, w4, b4, cloud, want_t_res):
    B, n, C = h.shape
    pred = R.Guarded(1, B, 3, device=dev)
    tres = R.Guarded(B, n, 3, device=dev) if want_t_res else None
    d_h, d_w, d_b, d_c = h.to(dev), w4.to(dev), b4.to(dev), cloud.to(dev)
    _lib.call("krrn_tbase_tail_f32", ptr(d_h), B, n, C, ptr(d_w), ptr(d_b), ptr(d_c), P(pred.ptr_value()),
              P(tres.ptr_value()) if want_t_res else P(0), _st())
    torch.cuda.synchronize()
    return pred.result()[0], (tres.result() if want_t_res else None)


# n: a partial 16-point wave group, exactly one 256-point pass, one point into the second, several passes;
# C / 4 < 4 leaves lanes of a point without a stripe, C / 4 = 3 is not a multiple of the 4 lanes
@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 1000])
@pytest.mark.parametrize("C", [4, 8, 12, 16, 256])
def test_tbase_tail(dev, C, n):
    B = 3
    g = _gen(C, n)
    h = torch.relu(torch.randn(B, n, C, generator=g))
    w4, b4 = torch.randn(3, C, generator=g) / C ** 0.5, 0.1 * torch.randn(3, generator=g)
    cloud = torch.tensor([0.02, -0.05, 0.9]) + 0.1 * torch.randn(B, n, 3, generator=g)
    t64, p64, t_bound, p_bound = R.tbase_tail_ref(h, w4, b4, cloud)
    pred, tres = _tail(dev, h, w4, b4, cloud, True)
    err_t = (tres.double() - t64).abs()
    assert (err_t <= t_bound).all(), float((err_t / t_bound).max())
    err_p = (pred.double() - p64).abs()
    assert (err_p <= p_bound).all(), float((err_p / p_bound).max())
    # a fixed summation order: t_res = NULL, a second run and a crop computed alone give the same bits
    pred2, none = _tail(dev, h, w4, b4, cloud, False)
    assert none is None and torch.equal(pred2, pred)
    pred3, tres3 = _tail(dev, h, w4, b4, cloud, True)
    assert torch.equal(pred3, pred) and torch.equal(tres3, tres)
    for b in range(B):
        pb, tb = _tail(dev, h[b:b + 1].contiguous(), w4, b4, cloud[b:b + 1].contiguous(), True)
        assert torch.equal(pb[0], pred[b]) and torch.equal(tb[0], tres[b])


# ---- krrn_heads_select_f32 -----------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 7), (17, 19)], ids=["5x7", "17x19-block-edge-inside-a-crop"])
def test_heads_select(dev, H, W):
    B, ncls, xyz_off = 3, 5, 7
    Cx, Cn = xyz_off + 3 * ncls + 2, 3 * ncls
    g = _gen(H, W)
    fx, fn = torch.randn(B, Cx, H, W, generator=g), torch.randn(B, Cn, H, W, generator=g)
    cls = torch.tensor([0, ncls - 1, 2], dtype=torch.int64)
    fn[0, 0:3, 0, 0] = 0.0                                   # an all-zero normal: exactly 0, not NaN
    fn[1, 3 * (ncls - 1):, 0, 1] = torch.tensor([1e-9, -1e-9, 1e-9])    # tiny but above the clamp: still unit length
    fn[2, 6:9, 1, 0] = torch.tensor([3e-13, 0.0, -4e-13])    # ||x|| = 5e-13 < 1e-12: divided by the clamp
    xyz, nml = R.Guarded(B, 3, H * W, device=dev), R.Guarded(B, 3, H * W, device=dev)
    d_fx, d_fn, d_cls = fx.to(dev), fn.to(dev), cls.to(dev)
    _lib.call("krrn_heads_select_f32", ptr(d_fx), Cx, xyz_off, ptr(d_fn), Cn, ptr(d_cls), P(xyz.ptr_value()),
              P(nml.ptr_value()), B, H, W, _st())
    torch.cuda.synchronize()
    ref_xyz, ref_n = R.heads_select_ref(fx, xyz_off, fn, cls)
    assert torch.equal(xyz.result(), ref_xyz.reshape(B, 3, H * W))
    got_n = nml.result().view(B, 3, H, W)
    # three products, two sums, a square root and a divide, each correctly rounded or contracted, on
    # components of magnitude <= 1
    assert ((got_n.double() - ref_n).abs() <= 8 * R.EPS32).all()
    assert (got_n[0, :, 0, 0] == 0).all()
    assert abs(float(got_n[1, :, 0, 1].double().norm()) - 1) <= 8 * R.EPS32
    assert torch.allclose(got_n[2, :, 1, 0].double(), torch.tensor([0.3, 0.0, -0.4], dtype=torch.float64), rtol=0,
                          atol=8 * R.EPS32)


# ---- krrn_points_gather_f32 ----------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 300])
def test_points_gather(dev, N):
    """choose holds pixel 0, pixel HW - 1, repeats (the loader wrap-pads short masks) and unsorted entries."""
    B, H, W = 3, 7, 9
    g = _gen(N)
    cloud = torch.randn(B, N, 3, generator=g)
    xyz, nml = torch.randn(B, 3, H, W, generator=g), torch.randn(B, 3, H, W, generator=g)
    choose = torch.randint(0, H * W, (B, N), generator=g, dtype=torch.int64)
    choose[:, 0] = torch.tensor([H * W - 1, 0, H * W - 1])
    if N > 1:
        choose[0, :40] = torch.arange(20).repeat(2)          # wrap padding
        choose[1, -3:] = torch.tensor([H * W - 1, 0, 0])
    p9 = R.Guarded(B, N, 9, device=dev)
    d_c, d_x, d_n, d_ch = cloud.to(dev), xyz.to(dev), nml.to(dev), choose.to(dev)
    _lib.call("krrn_points_gather_f32", ptr(d_c), ptr(d_x), ptr(d_n), ptr(d_ch), B, N, H, W, P(p9.ptr_value()), _st())
    torch.cuda.synchronize()
    assert torch.equal(p9.result(), R.points_gather_ref(cloud, xyz, nml, choose))


# ---- krrn_nchw_to_nhwc_f32 -----------------------------------------------------------------------
@pytest.mark.parametrize("C,o_cs,o_co", [(3, 4, 0), (5, 12, 4)], ids=["3-into-4-production", "5-into-12-at-4"])
def test_nchw_to_nhwc(dev, C, o_cs, o_co):
    B, H, W = 2, 7, 9
    x = torch.randn(B, C, H, W, generator=_gen(C))
    out = R.Guarded(1, B * H * W, C, stride=o_cs, off=o_co, device=dev)  # the pad channels stay sentinel
    d_x = x.to(dev)
    _lib.call("krrn_nchw_to_nhwc_f32", ptr(d_x), B, C, H, W, P(out.buf.data_ptr() + 4 * o_cs), o_cs, o_co, _st())
    torch.cuda.synchronize()
    assert torch.equal(out.result()[0], R.nchw_to_nhwc_ref(x).reshape(B * H * W, C))


# ---- krrn_add_relu_f32 ---------------------------------------------------------------------------
@pytest.mark.parametrize("has_b,relu", [(True, 1), (True, 0), (False, 0), (False, 1)],
                         ids=["add-relu", "add", "copy", "copy-relu"])
@pytest.mark.parametrize("npix", [1, 257])
@pytest.mark.parametrize("C", [4, 20, 128])
def test_add_relu(dev, C, npix, has_b, relu):
    """a, b and out with three different channel strides and offsets; one add and a max leave no
    contraction to differ by, so the result is torch's f32 bit for bit."""
    g = _gen(C, npix, has_b, relu)
    a, b = torch.randn(1, npix, C, generator=g), (torch.randn(1, npix, C, generator=g) if has_b else None)
    ga, gb = R.Guarded(1, npix, C, stride=C + 8, off=4), R.Guarded(1, npix, C, stride=C + 4, off=0)
    ga.fill(a)
    if has_b:
        gb.fill(b)
    out = R.Guarded(1, npix, C, stride=C + 12, off=8, device=dev)
    d_a, d_b = ga.buf.to(dev), gb.buf.to(dev)
    # the ABI takes base pointer + channel offset: the base is the first row after the guard row
    _lib.call("krrn_add_relu_f32", P(d_a.data_ptr() + 4 * ga.stride), ga.stride, ga.off,
              P(d_b.data_ptr() + 4 * gb.stride) if has_b else P(0), gb.stride, gb.off,
              P(out.buf.data_ptr() + 4 * out.stride), out.stride, out.off, npix, C, relu, _st())
    torch.cuda.synchronize()
    assert torch.equal(out.result(), R.add_relu_ref(a, b, relu))


@pytest.mark.parametrize("relu", [0, 1])
def test_add_relu_in_place(dev, relu):
    """out aliasing a with the same stride and offset: the HRNet fuse accumulator (`_fuse_output` adds the
    identity term into the running sum that already lives in `out`); the only aliasing a caller uses."""
    C, npix = 36, 257
    g = _gen(C, relu)
    a, b = torch.randn(1, npix, C, generator=g), torch.randn(1, npix, C, generator=g)
    acc = R.Guarded(1, npix, C, stride=C + 8, off=4, device=dev)
    acc.fill(a)
    d_b = b.to(dev)
    base = P(acc.buf.data_ptr() + 4 * acc.stride)
    _lib.call("krrn_add_relu_f32", base, acc.stride, acc.off, ptr(d_b), C, 0, base, acc.stride, acc.off, npix, C,
              relu, _st())
    torch.cuda.synchronize()
    assert torch.equal(acc.result(), R.add_relu_ref(a, b, relu))
