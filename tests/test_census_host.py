"""The term census (tests/census_ref.py) on the CPU: the census values meet their conditions, the
six-pair reference on the sparse operands is f32-exact and tells every single-pair mutation apart
(so the bit-for-bit GPU assertions of tests/test_gpu_term_census.py would catch each of them), and
the host weight packers hand the kernels exactly the h, m, l terms of the split."""
import itertools

import numpy as np
import pytest
import torch

import census_ref as cr
from pose_estimation_amd import ops

CROSS = list(itertools.product(cr.CENSUS_X, cr.CENSUS_W))


@pytest.mark.parametrize("cond", cr.CONDITIONS, ids=lambda f: f.__name__)
def test_census_value_conditions(cond):
    """Every x meets every w in the launches (rows cycle over x, columns over w): all nine pairs."""
    assert len(cr.CENSUS_X) >= 3 and len(cr.CENSUS_W) >= 3
    assert min(cr.CENSUS_X) < 0 and min(cr.CENSUS_W) < 0, "sign handling of the low terms needs a negative x and w"
    for x, w in CROSS:
        cond(x, w)


def test_census_values_survive_power_of_two_scales():
    """s(k) * w splits into s(k) times the terms of w, so the conditions carry over to scaled weights."""
    for w in cr.CENSUS_W:
        for s in (1.0, 2.0, 4.0, 8.0, -0.25, 64.0):
            assert cr.terms(s * w) == tuple(s * t for t in cr.terms(w))


def test_kscale_differs_within_every_quad():
    s = cr.kscale(torch.arange(4096)).view(-1, 4)
    assert set(s.unique().tolist()) == {1.0, 2.0, 4.0, 8.0}
    assert all(len(set(q)) == 4 for q in s.tolist())


def test_decode_names_the_mutation():
    for x, w in CROSS:
        for mult in [(1,) * 6] + cr.mutations():
            v = float(np.dot(mult, cr.pair_products(x, w)[0])) * 4.0
            assert cr.decode(v, x, w, 4.0) == mult
        assert cr.decode(3.0 * cr.s6(x, w), x, w) is None
        assert cr.decode(float("nan"), x, w) is None


SHAPES = [(200, 160, 128), (77, 64, 96), (300, 324, 72)]


def _expected(kind, M, K, N):
    """The closed form of both launches: s(k) * S6(x, w) at each output's only non-zero k."""
    S = torch.tensor([[cr.s6(x, w) for w in cr.CENSUS_W] for x in cr.CENSUS_X], dtype=torch.float64)
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    if kind == "a":
        k = (m % K).expand(M, N)
        return cr.kscale(k).double() * S[m % 3, n % 3]
    k = (n % K).expand(M, N)
    return cr.kscale(k).double() * S[(m + k) % 3, n % 3]


@pytest.mark.parametrize("kind", ["a", "w"])
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_six_pair_product_exact_and_mutations_differ(kind, M, K, N):
    A, W = (cr.a_onehot_operands if kind == "a" else cr.w_onehot_operands)(M, K, N)
    ref = cr.six_pair_product(A, W)  # asserts f32-exactness
    assert torch.equal(ref, _expected(kind, M, K, N))
    assert bool((ref != 0).all()), "every output of a GEMM launch holds one census product"
    # dropping ml + lm + ll costs less than half an ulp: S6 is the f32 nearest the true product
    true = A.double() @ W.double().t()
    assert torch.equal(true.float(), ref.float())
    muts = cr.mutations()
    assert len(muts) == 12 and len(set(muts)) == 12 and (1,) * 6 not in muts
    for mult in muts:
        mut = cr.six_pair_product(A, W, mult=mult, exact=False)
        # different in f64, and still different once a kernel has rounded its sum to f32
        assert bool((mut != ref).all()), mult
        assert bool((mut.float() != ref.float()).all()), mult


def test_six_pair_product_through_a_conv():
    """The same reference with a convolution as the bilinear op (what the conv tests use)."""
    import torch.nn.functional as F
    x = torch.zeros(2, 8, 9, 11)
    for b, (yy, xx) in itertools.product(range(2), itertools.product(range(1, 9, 3), range(1, 11, 3))):
        x[b, (yy + xx + b) % 8, yy, xx] = cr.CENSUS_X[(yy + xx) % 3]
    w = torch.tensor(cr.CENSUS_W)[torch.arange(12) % 3].view(12, 1, 1, 1) * cr.kscale(torch.arange(72)).view(1, 8, 3, 3)
    ref = cr.six_pair_product(x, w.contiguous(), op=lambda a, b: F.conv2d(a, b, padding=1))
    assert ref.shape == (2, 12, 9, 11) and bool((ref != 0).all())
    for mult in cr.mutations():
        mut = cr.six_pair_product(x, w.contiguous(), op=lambda a, b: F.conv2d(a, b, padding=1), mult=mult, exact=False)
        assert bool((mut.float() != ref.float()).all()), mult


def test_im2col_is_the_conv():
    """census_ref.im2col restates krrn_conv2d_f32's A operand: im2col(x) @ W^T is the conv."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 7, 9, 8, generator=g)
    w = torch.randn(12, 8, 3, 3, generator=g)
    taps = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]
    for s, (Hg, Wg) in ((1, (7, 9)), (2, (4, 5))):
        A = cr.im2col(x, Hg, Wg, s, taps)
        wt = w.permute(0, 2, 3, 1).reshape(12, 72)  # k = tap * cin + c
        ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), stride=s, padding=1)
        got = (A.double() @ wt.double().t()).view(2, Hg, Wg, 12).permute(0, 3, 1, 2)
        assert float((got - ref).abs().max()) < 1e-12


@pytest.mark.parametrize("m", [2, 4])
def test_wino_reference_is_the_conv(m):
    """census_ref.wino_six_pair with U = G g G^T (ops.wino_weights / wino4_weights, so their xi
    order, chunk layout and transform matrices) is the 3x3 conv at f32 accuracy, ragged tiles included."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(m)
    conv = torch.nn.Conv2d(12, 8, 3, 1, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / 10)
    x = torch.randn(2, 9, 11, 12, generator=g)
    Uc = (ops.wino_weights if m == 2 else ops.wino4_weights)(conv, "cpu")
    U = cr.wino_from_chunk_major(Uc, 12)
    assert torch.equal(cr.wino_chunk_major(U), Uc)
    got = cr.wino_six_pair(x, U, m, exact=False).permute(0, 3, 1, 2)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), conv.weight.detach().double(), padding=1)
    assert float((got - ref).abs().max()) <= 2e-6 * float(ref.abs().max())


@pytest.mark.parametrize("onehot", [False, True], ids=["a_onehot", "w_onehot"])
@pytest.mark.parametrize("m,B,H,W,C", [(2, 4, 7, 37, 52), (4, 3, 14, 67, 40)])
def test_wino_census_exact_and_mutations_differ(m, B, H, W, C, onehot):
    N = 72
    x, npix = cr.wino_pixels(m, B, H, W, C, dense_c=onehot)
    assert npix >= C, "every input channel carries a probe"
    U = cr.wino_probe_weights(m, N, C, onehot)
    ref = cr.wino_six_pair(x, U, m)  # asserts V, M and Y are f32-exact
    live = ref != 0
    assert bool(live.any(dim=(0, 1, 2)).all()), "every output channel (transform position) sees a product"
    assert int(live.sum()) >= B * H * W
    for mult in cr.mutations():
        mut = cr.wino_six_pair(x, U, m, mult=mult, exact=False)
        assert bool((mut.float() != ref.float())[live].all()), mult
        assert bool((mut == 0)[~live].all())


# --------------------------------------------------------------------------------------------
# Packers conserve terms
# --------------------------------------------------------------------------------------------

def _words(t: torch.Tensor) -> np.ndarray:
    """The non-zero bf16 words of a packed tensor (bf16 or int32 storage), sorted."""
    t = t.detach().cpu().contiguous()
    w = t.view(torch.int16).reshape(-1).numpy().view(np.uint16)
    return np.sort(w[(w & 0x7FFF) != 0])


def _planes(wt: torch.Tensor, mult=(1, 1, 1)) -> np.ndarray:
    h, m, l = ops.split_bf16x3(wt)
    return np.sort(np.concatenate([_words(p) for p, c in zip((h, m, l), mult) for _ in range(c)]))


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(*shape, generator=g) * torch.pow(2.0, torch.randint(-6, 3, shape, generator=g).float())
    assert int((w == 0).sum()) == 0
    return w


def _conserved(packed, wt, mult=(1, 1, 1)):
    got, want = _words(packed), _planes(wt, mult)
    assert got.shape == want.shape and bool((got == want).all()), (got.size, want.size)


def test_conv_weights_x3_conserves_terms():
    wt = _rand(72, 324, seed=1)
    p = ops.conv_weights_x3(wt)
    assert p.dtype == torch.bfloat16 and p.numel() == 72 * 324 * 4  # m h l + 4 zeros per 4 k
    _conserved(p, wt)


def test_gemm_weights_x3_conserves_terms():
    """h twice per element: once beside l (quad 0) and once beside m (quad 1)."""
    wt = _rand(128, 160, seed=2)
    p = ops.gemm_weights_x3(wt)
    assert p.numel() * 2 == 128 * 160 * 4
    _conserved(p, wt, mult=(2, 1, 1))


def test_gemm_weights_panel_conserves_terms():
    wt = _rand(96, 128, seed=3)
    p = ops.gemm_weights_panel(wt)
    assert p.numel() * 2 == 96 * 128 * 3
    _conserved(p, wt)


@pytest.mark.parametrize("N,K,kq_mult", [(72, 128, 4), (40, 100, 4), (50, 36, 2)])
def test_quad_weights_x3_conserves_terms(N, K, kq_mult):
    wt = _rand(N, K, seed=4)
    p = ops.quad_weights_x3(wt, N, K, kq_mult)
    n16, kqp = (N + 15) // 16 * 16, -(-(K // 4) // kq_mult) * kq_mult
    assert p.numel() * 2 == n16 * kqp * 4 * 3
    _conserved(p, wt)


@pytest.mark.parametrize("nxi", [16, 36])
def test_wino_weights_x3_conserves_terms(nxi):
    U = _rand(5, nxi, 72, 8, seed=nxi)
    p = ops.wino_weights_x3(U)
    assert p.dtype == torch.bfloat16 and p.numel() == U.numel() * 3
    _conserved(p, U)


@pytest.mark.parametrize("k,op", [(4, 0), (3, 1), (2, 0)])
def test_convT_weights_x3_conserves_terms(k, op):
    """Each class's taps once; a class's missing taps are zero words."""
    cin, cout = 24, 128
    convT = torch.nn.ConvTranspose2d(cin, cout, k, 2, 1, output_padding=op, bias=False)
    with torch.no_grad():
        convT.weight.copy_(_rand(cin, cout, k, k, seed=k))
    spec = ops.make_convT(convT, None, "cpu")
    U3, table = ops.convT_weights_x3(spec)
    assert U3.numel() == (cin // 8) * 16 * cout * 8 * 3
    assert [table[5 * c] for c in range(4)] == [len(t) for t in spec.taps]
    # the four classes' taps partition the k x k kernel: every weight once
    assert sum(len(t) for t in spec.taps) == k * k
    _conserved(U3, convT.weight.detach())
