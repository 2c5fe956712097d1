"""Term census of every split-bf16 (x3) kernel: each is held bit for bit to the six-pair sum
hh + hm + mh + hl + lh + mm of tests/census_ref.py (identity epilogue: scale 1, bias 0, no residual,
no ReLU), on operands with one non-zero k per output, where that sum is one exact f32 and a lost,
doubled or mis-paired term pair gives another (tests/test_census_host.py proves both on the CPU).

Two launches per kernel: "a" (A one-hot: row / pixel m holds one census x at one k, the weights are
dense, census w times a power-of-two scale s(k) that differs within every k quad) and "w" (W one-hot:
column n holds one census w at one k, the activations are dense). Ragged M and N where the entry point
allows, K = at least two stages of the kernel's k-pipeline plus a tail. Outputs are NaN-filled first:
every owned element is then s(k) * S6 or exactly 0.

torch.equal is the assertion: bf16 x bf16 products are exact in f32 and every subset sum of a census
pair's six products is an f32 (census_ref.assert_partial_sums_f32), so no accumulation order rounds.

Head forms (krrn_conv3x3_wino_x3_head_f32, krrn_conv3x3_wino4_x3_head_f32) have no case of their own:
they instantiate the main-loop templates of the plain forms, wino_f23_x3_kernel<HEAD> and
wino_f43_x3_kernel<HP>, and differ only in the epilogue. The live forms run gemm_x3_kernel<GA> too but
skip row tiles, so each has a case."""
import ctypes

import pytest
import torch

import census_ref as cr
from pose_estimation_amd import _lib, ops
from pose_estimation_amd.runtime import ConvDesc, P, conv_desc, ptr

pytestmark = pytest.mark.gpu

NAN = float("nan")
KINDS = ["a", "w"]


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def _assert_census(got: torch.Tensor, A: torch.Tensor, W: torch.Tensor, what: str):
    """got [M, N] == the six-pair sum of A [M, K] and W [N, K], bit for bit; on a mismatch the first
    bad outputs are decoded into the multiplicities of (hh, hm, mh, hl, lh, mm) the kernel summed."""
    ref = cr.six_pair_product(A, W).float()
    got = got.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if torch.equal(got, ref):
        return

    def info(idx):
        m, n = idx
        p = (A[m] * W[n]).abs()
        k = int(p.argmax())
        return (k, float(A[m, k]), float(W[n, k]), 1.0) if float(p[k]) != 0.0 else None

    raise AssertionError(f"{what}: not the six-pair sum\n" + cr.describe_mismatch(got, ref, info))


def _assert_probes_every_k_position(A: torch.Tensor, W: torch.Tensor, period: int = 32):
    """The launch's non-zero products sit at every k position of a pipeline stage (k mod 32)."""
    k = torch.nonzero((A != 0).any(0) & (W != 0).any(0)).flatten()
    assert len(set((k % period).tolist())) == min(period, A.shape[1])


def _gemm_operands(kind, M, K, N, k0=0):
    return (cr.a_onehot_operands if kind == "a" else cr.w_onehot_operands)(M, K, N, k0)


# --------------------------------------------------------------------------------------------
# gemm_x3.hip: KC = 16 k per LDS chunk, loaded two chunks ahead; K = 160 = 10 chunks (K % 32 is
# the entry point's rule, N % 128 too: two column blocks; M = 200 = one full and one ragged row tile)
# --------------------------------------------------------------------------------------------

GM, GK, GN = 200, 160, 256


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("live", [False, True], ids=["plain", "live"])
def test_gemm_x3(dev, kind, live):
    """krrn_gemm_x3_f32 / krrn_gemm_x3_live_f32: two strided groups with their own one-hot positions;
    live = [200, 77] leaves group 1's second row tile (rows 128..) unwritten."""
    lda, ldo, batch = GK + 4, GN + 4, 2
    ops_g = [_gemm_operands(kind, GM, GK, GN, k0=37 * g) for g in range(batch)]
    W = ops_g[0][1]  # shared by the groups (a: the dense W does not depend on k0)
    ops_g = [(a, W) for a, _ in ops_g]
    A = torch.full((batch, GM, lda), 3.0)
    for g in range(batch):
        A[g, :, :GK] = ops_g[g][0]
    A = A.to(dev)
    w3 = ops.gemm_weights_x3(W.to(dev))
    out = torch.full((batch, GM, ldo), NAN, device=dev)
    L = _lib.lib()
    if live:
        lv = torch.tensor([GM, 77], dtype=torch.int32, device=dev)
        st = L.krrn_gemm_x3_live_f32(ptr(A), lda, GM, GK, GN, ptr(w3), P(0), P(0), 0, ptr(out), ldo, 0, batch,
                                     GM * lda, GM * ldo, 0, ptr(lv), _stream())
    else:
        st = L.krrn_gemm_x3_f32(ptr(A), lda, GM, GK, GN, ptr(w3), P(0), P(0), 0, ptr(out), ldo, 0, batch, GM * lda,
                                GM * ldo, 0, _stream())
    _lib.check(st, "gemm_x3")
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[:, :, GN:]).all(), "wrote past N"
    for g in range(batch):
        rows = 128 if (live and g == 1) else GM
        _assert_census(out[g, :rows, :GN], ops_g[g][0][:rows], W, f"gemm_x3 {kind} group {g}")
        assert torch.isnan(out[g, rows:, :GN]).all(), "a skipped row tile was written"
        _assert_probes_every_k_position(ops_g[g][0], W)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("live", [False, True], ids=["plain", "live"])
def test_gemm_x3_gather(dev, kind, live):
    """krrn_gemm_x3_gather_f32 / krrn_gemm_x3_gather_live_f32: h1 = ReLU(P1[ia] + P2[ib]) is the census
    operand (the ReLU is part of the op, so |x|: the even k of a row come from table 1, the odd k from
    table 2, both through shuffled row indices)."""
    B, npts = 2, GM
    g = torch.Generator().manual_seed(1)
    L = _lib.lib()
    H1, P1, P2, IA, IB = [], [], [], [], []
    W = _gemm_operands(kind, npts, GK, GN)[1]  # shared by the crops
    for b in range(B):
        A = _gemm_operands(kind, npts, GK, GN, k0=37 * b)[0].abs()
        even = (torch.arange(GK) % 2 == 0)[None, :]
        ia, ib = torch.randperm(npts, generator=g), torch.randperm(npts, generator=g)
        t1, t2 = torch.zeros(npts, GK), torch.zeros(npts, GK)
        t1[ia] = torch.where(even, A, torch.zeros(()))   # row ia[i] of table 1 serves point i
        t2[ib] = torch.where(even, torch.zeros(()), A)
        assert torch.equal((t1[ia] + t2[ib]).clamp_min(0), A)
        for lst, v in zip((H1, P1, P2, IA, IB), (A, t1, t2, ia, ib)):
            lst.append(v)
    P1d, P2d = torch.stack(P1).to(dev), torch.stack(P2).to(dev)
    iad, ibd = torch.stack(IA).int().to(dev), torch.stack(IB).int().to(dev)
    w3 = ops.gemm_weights_x3(W.to(dev))
    ldo = GN + 4
    out = torch.full((B * npts, ldo), NAN, device=dev)
    args = (ptr(iad), ptr(P1d), npts * GK, GK, ptr(ibd), ptr(P2d), npts * GK, GK, npts, B, GK, GN, ptr(w3), P(0),
            ptr(out), ldo, 0)
    if live:
        lv = torch.tensor([npts, 77], dtype=torch.int32, device=dev)
        st = L.krrn_gemm_x3_gather_live_f32(*args, ptr(lv), _stream())
    else:
        st = L.krrn_gemm_x3_gather_f32(*args, _stream())
    _lib.check(st, "gemm_x3_gather")
    torch.cuda.synchronize()
    out = out.cpu().view(B, npts, ldo)
    assert torch.isnan(out[:, :, GN:]).all(), "wrote past N"
    for b in range(B):
        rows = 128 if (live and b == 1) else npts
        _assert_census(out[b, :rows, :GN], H1[b][:rows], W, f"gemm_x3_gather {kind} crop {b}")
        assert torch.isnan(out[b, rows:, :GN]).all(), "a skipped row tile was written"


# --------------------------------------------------------------------------------------------
# gemm_panel.hip: the whole K (64 or 128 = 8 or 16 8-k groups) sits in registers; N = 96 = three
# 32-column tiles (csplit = 2: ragged column ranges), M = 200 = one full and one ragged 128-row panel
# --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,csplit", [(128, 1), (128, 2), (64, 2)])
def test_gemm_panel(dev, kind, K, csplit):
    M, N, lda, ldo = 200, 96, K + 4, 100
    A, W = _gemm_operands(kind, M, K, N, k0=5)
    Ad = torch.full((M, lda), 3.0)
    Ad[:, :K] = A
    Ad = Ad.to(dev)
    wp = ops.gemm_weights_panel(W.to(dev))
    out = torch.full((M, ldo), NAN, device=dev)
    _lib.check(_lib.lib().krrn_gemm_panel_x3_f32(ptr(Ad), lda, M, K, N, ptr(wp), P(0), P(0), 0, ptr(out), ldo, 0,
                                                 csplit, _stream()), "gemm_panel_x3")
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[:, N:]).all(), "wrote past N"
    _assert_census(out[:, :N], A, W, f"gemm_panel {kind} K={K} csplit={csplit}")
    _assert_probes_every_k_position(A, W)


def _panel_census_error(dev, kind, spoil):
    """The failure message of the panel census with `spoil` applied to the packed weights
    ([N/32][K/8][384] words: 64 lanes x [m0..m3 h0..h3], then 64 lanes x [l0 l1 | l2 l3])."""
    M, K, N = 200, 128, 96
    A, W = _gemm_operands(kind, M, K, N, k0=5)
    wp = ops.gemm_weights_panel(W.to(dev))
    spoil(wp)
    out = torch.full((M, N), NAN, device=dev)
    _lib.check(_lib.lib().krrn_gemm_panel_x3_f32(ptr(A.to(dev)), K, M, K, N, ptr(wp), P(0), P(0), 0, ptr(out), N, 0, 1,
                                                 _stream()), "gemm_panel_x3")
    torch.cuda.synchronize()
    with pytest.raises(AssertionError) as e:
        _assert_census(out, A, W, "spoiled")
    return str(e.value)


@pytest.mark.parametrize("kind", KINDS)
def test_census_sees_a_lost_term_and_a_wrong_k(dev, kind):
    """The census is not vacuous on the device: the same kernel on weights whose l plane is zeroed
    (the pair hl lost at every k) or whose l words are exchanged within each k quad (x_h meets the
    w_l of another k) misses the six-pair sum at every output, and the message decodes the first case."""
    def drop_l(wp):
        wp[:, :, 256:] = 0

    def swap_l(wp):
        lp = wp[:, :, 256:].view(wp.shape[0], wp.shape[1], 64, 2)
        lp.copy_(lp.flip(-1).clone())

    msg = _panel_census_error(dev, kind, drop_l)
    assert msg.splitlines()[1].startswith(f"{200 * 96} of {200 * 96} outputs differ"), msg
    assert "census (1, 1, 1, 0, 1, 1)" in msg, msg
    msg = _panel_census_error(dev, kind, swap_l)
    # w: the one-hot column's l lands on a k whose activation has another scale, or on none of its own
    assert msg.splitlines()[1].startswith(f"{200 * 96} of {200 * 96} outputs differ"), msg
    assert "census (1, 1, 1, 1, 1, 1)" not in msg, msg


# --------------------------------------------------------------------------------------------
# conv1x1_nchw.hip (x3): cin = 128 is the entry point's only K (8 k steps of 16); 72 weight rows =
# four full 16-channel tiles and a ragged fifth, 70 stored; HW = 125 (odd: ragged 16-pixel subtiles)
# --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_conv1x1_nchw_x3(dev, kind):
    B, HW, K, N, n_store, Cx, oc, cs, co = 2, 125, 128, 72, 70, 75, 3, 136, 4
    A, W = _gemm_operands(kind, B * HW, K, N, k0=11)
    x = torch.full((B * HW, cs), 3.0)
    x[:, co:co + K] = A
    x = x.to(dev)
    w3 = ops.quad_weights_x3(W.to(dev), N, K)
    scale, bias = torch.ones(N, device=dev), torch.zeros(N, device=dev)
    out = torch.full((B, Cx, HW), NAN, device=dev)
    _lib.check(_lib.lib().krrn_conv1x1_nchw_x3_f32(ptr(x), cs, co, B, HW, K, ptr(w3), N, n_store, ptr(scale),
                                                   ptr(bias), ptr(out), Cx, oc, _stream()), "conv1x1 nchw x3")
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[:, :oc]).all() and torch.isnan(out[:, oc + n_store:]).all()
    got = out[:, oc:oc + n_store].permute(0, 2, 1).reshape(B * HW, n_store)
    _assert_census(got, A, W[:n_store], f"conv1x1_nchw_x3 {kind}")
    _assert_probes_every_k_position(A, W)


# --------------------------------------------------------------------------------------------
# conv_gemm.hip (x3): 3x3 stride 1 on 4 x 9 x 11 pixels, 36 -> 72 channels: K = 324 = 20 k-tiles of 16
# and a tail of 4 (tile 2, the plans' X3_TILE) or 10 of 32 and the tail (tiles 7, 8); 36 channels are
# no multiple of either; M = 396 and N = 72 are ragged against every tile
# --------------------------------------------------------------------------------------------

CB, CH, CW, CCIN, CN = 4, 9, 11, 36, 72
TAPS3 = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]


def _conv_operands(kind):
    """(x NHWC, wt [N, 9 * cin], A = im2col(x)). a: non-zero pixels 3 apart in both directions (one
    per 3x3 window), one channel each: the one-hot k of an output pixel walks the taps with its position
    in the window and the channels with the window. w: dense pixels, one-hot weight columns."""
    if kind == "a":
        x, npix = cr.sparse_pixels(CB, CH, CW, CCIN, cr.grid_every(3, CH, lambda b: b),
                                   cr.grid_every(3, CW, lambda b: b // 2 + 1))
        assert npix >= CCIN
        wt = cr.dense_weights(CN, 9, CCIN)
    else:
        x = cr.dense_pixels(CB, CH, CW, CCIN)
        wt = cr.onehot_weights(CN, 9 * CCIN, stride=5, k0=2)
    return x, wt, cr.im2col(x, CH, CW, 1, TAPS3)


def _conv_spec(wt, dev):
    n = wt.shape[0]
    return ops.ConvSpec([wt.to(dev)], [TAPS3], [(0, 0)], torch.ones(n, device=dev), torch.zeros(n, device=dev), CCIN, n,
                        1, "conv", 3, 1, CCIN)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tile,splits", [(2, 1), (7, 1), (8, 4)], ids=["tile2", "tile7", "tile8_splitk4"])
def test_conv2d_x3(dev, kind, tile, splits):
    """krrn_conv2d_x3_f32; the split-K case sums each output's one non-zero slice with exact zeros."""
    x, wt, A = _conv_operands(kind)
    spec = _conv_spec(wt, dev)
    xa = ops.Act(x.to(dev), CB, CH, CW, CCIN, 0, CCIN)
    out = ops.new_act(CB, CH, CW, CN, dev, cs=CN + 4)
    out.t.fill_(NAN)
    ws = torch.full((splits * CB * CH * CW * CN,), NAN, device=dev) if splits > 1 else None
    ops.conv2d(xa, spec, out, tile=tile, splits=splits, ws=ws, x3=True)
    torch.cuda.synchronize()
    t = out.t.cpu()
    assert torch.isnan(t[..., CN:]).all(), "wrote past N"
    _assert_census(t[..., :CN].reshape(-1, CN), A, wt, f"conv2d_x3 {kind} tile {tile} splits {splits}")
    _assert_probes_every_k_position(A, wt)


@pytest.mark.parametrize("tile", [1, 8])
def test_conv2d_group_x3(dev, tile):
    """krrn_conv2d_group_x3_f32: one launch of four problems, both census launches in tap-major k
    order and in channel-chunk-major order (k_chunk = 12, weights through ops.kchunk_weights)."""
    keep, probs, outs, refs = [], [], [], []
    for kind in KINDS:
        x, wt, A = _conv_operands(kind)
        xd = x.to(dev)
        one, zero = torch.ones(CN, device=dev), torch.zeros(CN, device=dev)
        for kc in (0, 12):
            w = wt.to(dev)
            w3 = ops.conv_weights_x3(ops.kchunk_weights(w, 9, CCIN, kc) if kc else w)
            out = torch.full((CB, CH, CW, CN + 4), NAN, device=dev)
            keep += [xd, w3, one, zero]
            probs.append(conv_desc(x=ptr(xd), x_cs=CCIN, x_co=0, B=CB, Hi=CH, Wi=CW, cin_p=CCIN, Hg=CH, Wg=CW, in_s=1,
                                   taps=TAPS3, wt=ptr(w3), N=CN, n_store=CN, scale=ptr(one), bias=ptr(zero),
                                   out=ptr(out), out_cs=CN + 4, out_co=0, Ho=CH, Wo=CW, k_chunk=kc))
            outs.append(out)
            refs.append((A, wt, f"conv2d_group_x3 {kind} k_chunk {kc} tile {tile}"))
    arr = (ConvDesc * len(probs))(*probs)
    _lib.check(_lib.lib().krrn_conv2d_group_x3_f32(ctypes.cast(arr, P), len(probs), tile, _stream()), "conv group x3")
    torch.cuda.synchronize()
    for out, (A, wt, what) in zip(outs, refs):
        t = out.cpu()
        assert torch.isnan(t[..., CN:]).all(), "wrote past N"
        _assert_census(t[..., :CN].reshape(-1, CN), A, wt, what)


# --------------------------------------------------------------------------------------------
# convt.hip: 8 input channels per chunk through a 2-slot LDS buffer; cin = 24 = 3 chunks (whole chunks
# are the entry point's rule, N = 128 too); a 6 x 35 grid = two 4 x 32 block rows and columns, both ragged
# --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,op", [(4, 0), (3, 1)])
def test_convT_s2_x3(dev, kind, k, op):
    """krrn_convT_s2_x3_f32, all four parity classes: class (py, px) of a grid point is one conv over
    the class's taps (ops.make_convT), held to the six-pair sum of its own im2col operand and weights."""
    B, cin, Hi, Wi, N = 2, 24, 6, 35, 128
    convT = torch.nn.ConvTranspose2d(cin, N, k, 2, 1, output_padding=op, bias=False)
    wgt = torch.zeros(cin, N, k, k)
    if kind == "a":
        x, npix = cr.sparse_pixels(B, Hi, Wi, cin, cr.grid_every(3, Hi, lambda b: b), cr.grid_every(3, Wi, lambda b: b + 1))
        assert npix >= cin
        c, t = torch.meshgrid(torch.arange(cin), torch.arange(k * k), indexing="ij")
        s = cr.kscale(c, t).view(cin, 1, k, k)
        wgt = torch.tensor(cr.CENSUS_W)[torch.arange(N) % 3].view(1, N, 1, 1) * s
    else:
        x = cr.dense_pixels(B, Hi, Wi, cin)
        n = torch.arange(N)
        j = (n * 7 + 3) % (cin * k * k)
        wgt[j // (k * k), n, (j % (k * k)) // k, j % k] = torch.tensor(cr.CENSUS_W)[n % 3]
    with torch.no_grad():
        convT.weight.copy_(wgt)
    host = ops.make_convT(convT, None, "cpu")
    spec = ops.make_convT(convT, None, dev)
    U3, table = ops.convT_weights_x3(spec)
    Ho, Wo = 2 * Hi, 2 * Wi
    xd = torch.full((B, Hi, Wi, cin + 8), 3.0)
    xd[..., 4:4 + cin] = x
    xd = xd.to(dev)
    out = torch.full((B, Ho, Wo, N + 8), NAN, device=dev)
    _lib.check(_lib.lib().krrn_convT_s2_x3_f32(ptr(xd), cin + 8, 4, B, Hi, Wi, cin, table, ptr(U3), N, ptr(spec.scale),
                                               ptr(spec.bias), 0, ptr(out), N + 8, 4, Ho, Wo, _stream()), "convT_s2")
    torch.cuda.synchronize()
    t = out.cpu()
    assert torch.isnan(t[..., :4]).all() and torch.isnan(t[..., 4 + N:]).all()
    assert float(host.scale.min()) == 1.0 and float(host.scale.max()) == 1.0 and float(host.bias.abs().max()) == 0.0
    for (py, px), taps, w in zip(host.cls_off, host.taps, host.wt):
        A = cr.im2col(x, Hi, Wi, 1, taps)
        got = t[:, py::2, px::2, 4:4 + N].reshape(-1, N)
        _assert_census(got, A, w, f"convT_s2 {kind} k={k} class ({py}, {px})")


# --------------------------------------------------------------------------------------------
# winograd.hip / winograd4.hip: 8 input channels per chunk; F(2x2) through a 3-slot raw ring: cin = 52
# = 6 chunks and a 4-channel tail; F(4x4) through 2-slot rings: cin = 40 = 5 chunks (whole chunks are
# its entry point's rule). 72 output channels = one full and one ragged 64-channel block, each channel
# probing one transform position xi = n mod 16 (36). Maps ragged against the tiles and the blocks
# (F(2x2): 32 x 4 pixels per block, 7 x 37; F(4x4): 64 x 8, 14 x 67), border tiles included.
# --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,B,H,W,C", [(2, 4, 7, 37, 52), (4, 3, 14, 67, 40)], ids=["f2x2", "f4x4"])
def test_winograd_x3(dev, kind, m, B, H, W, C):
    """krrn_conv3x3_wino_x3_f32 / krrn_conv3x3_wino4_x3_f32 fed U in the transform domain, against
    census_ref.wino_six_pair (V = B^T d B exact, the six-pair sum over the channels, Y = A^T M A exact)."""
    N = 72
    x, npix = cr.wino_pixels(m, B, H, W, C, dense_c=(kind == "w"))
    assert npix >= C
    U = cr.wino_probe_weights(m, N, C, onehot=(kind == "w"))
    ref = cr.wino_six_pair(x, U, m).float()
    U3 = ops.wino_weights_x3(cr.wino_chunk_major(U).to(dev))
    cs, co = C + 8, 4
    xd = torch.full((B, H, W, cs), 3.0)
    xd[..., co:co + C] = x
    xd = xd.to(dev)
    one, zero = torch.ones(N, device=dev), torch.zeros(N, device=dev)
    out = torch.full((B, H, W, N + 4), NAN, device=dev)
    L = _lib.lib()
    fn = L.krrn_conv3x3_wino_x3_f32 if m == 2 else L.krrn_conv3x3_wino4_x3_f32
    _lib.check(fn(ptr(xd), cs, co, B, H, W, C, ptr(U3), N, N, ptr(one), ptr(zero), P(0), 0, 0, ptr(out), N + 4, 0, 0,
                  _stream()), "winograd x3")
    torch.cuda.synchronize()
    t = out.cpu()
    assert torch.isnan(t[..., N:]).all(), "wrote past N"
    got = t[..., :N]
    if torch.equal(got, ref):
        return
    nxi = (m + 2) ** 2

    def info(idx):  # (b, y, x, n): the expected value is +-2^p S6 of one census pair
        pair = cr.census_pair_of(float(ref[idx]))
        return None if pair is None else (f"xi {idx[3] % nxi}", *pair)

    raise AssertionError(f"winograd F({m}x{m}) {kind}: not the six-pair sum (indices are b, y, x, n; k is the "
                         f"transform position)\n" + cr.describe_mismatch(got, ref, info))
