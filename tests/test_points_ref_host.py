"""The references of tests/points_ref.py against what they restate, on the CPU: the kNN reference (a)
against the committed lattice fixture and the oracle's get_neighbor_index / get_nearest_index; the
pool_max reference against the oracle's Pool_layer; the tbase_tail and gather2_add references against
the oracle's TBase tail and conv1 over the concat on a tiny random model (f64 against f32 rounding);
and reference (a) against the float64 check (b) on every kNN input of the GPU test's case table."""
import os

import numpy as np
import pytest
import torch

from oracle import krrn_oracle as O
from tests import points_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_knn_ref_reproduces_lattice_fixture():
    g = np.load(os.path.join(GOLD, "knn_lattice.npz"))
    v, v9 = torch.from_numpy(g["v"]), torch.from_numpy(g["v9"])
    assert np.array_equal(R.knn_ref(v, v, 10, 1, 0).numpy(), g["idx_k10"])
    assert np.array_equal(R.knn_ref(v, v, 4, 1, 0).numpy(), g["idx_k4"])
    assert np.array_equal(R.knn_ref(v9, v9, 7, 1, 0).numpy(), g["idx9_k7"])
    assert np.array_equal(R.knn_ref(v, v[:, ::4].contiguous(), 1, 0, 1)[..., 0].numpy(), g["nearest"])


@pytest.mark.parametrize("family", ["random", "lattice", "cloud", "dup"])
@pytest.mark.parametrize("d", [3, 9])
def test_knn_ref_is_the_oracle(family, d):
    gen = torch.Generator().manual_seed(d)
    v = R.knn_points(family, 2, 90, d, gen)
    rows = torch.randperm(90, generator=gen)[:22]
    for k in (1, 4, 10):
        assert torch.equal(R.knn_ref(v, v, k, 1, 0), O.get_neighbor_index(v, k))
        assert torch.equal(R.knn_ref(v, v, k, 1, 0, qidx=rows), O.get_neighbor_index(v, k, rows=rows))
    src = v[:, rows].contiguous()
    assert torch.equal(R.knn_ref(v, src, 1, 0, 1), O.get_nearest_index(v, src))


def test_knn_ref_same_points_returns_ascending():
    v = R.knn_points("same", 2, 20, 3, torch.Generator().manual_seed(0))
    assert torch.equal(R.knn_ref(v, v, 6, 1, 0), torch.arange(1, 7).expand(2, 20, 6))


def test_knn_check_rejects_a_wrong_neighbour():
    gen = torch.Generator().manual_seed(5)
    v = R.knn_points("cloud", 1, 50, 3, gen)
    idx = R.knn_ref(v, v, 5, 0, 0)
    R.knn_check_f64(v, v, idx, 5)
    far = ((v[0, :1] - v[0]) ** 2).sum(-1).argmax()
    bad = idx.clone()
    bad[0, 0, 4] = far
    with pytest.raises(AssertionError, match="rounding slack"):
        R.knn_check_f64(v, v, bad, 5)
    bad = idx.clone()
    bad[0, 0, 4] = bad[0, 0, 3]
    with pytest.raises(AssertionError, match="repeats"):
        R.knn_check_f64(v, v, bad, 5)


@pytest.mark.parametrize("case", R.KNN_CASES, ids=[c[0] for c in R.KNN_CASES])
def test_knn_ref_meets_f64_check(case):
    """Reference (a) on the inputs of every GPU case: within the rounding bound of the float64 brute
    force, and the id's lane form / chunk count is the one the dispatch rule gives."""
    name, d, B, nq, nc, k, drop, mode, family, layout = case
    _, qidx, q, c = R.knn_case_inputs(case)
    assert q.shape == (B, nq, d) and c.shape[1:] == (nc, d)
    assert name.startswith(f"l{R.knn_lanes(B, nq, nc)}-d{d}-")
    assert ("chunk" in name) == (nc > 1024)
    K = k + drop
    ks = next(s for s in (1, 2, 5, 8, 11, 16) if K <= s)
    assert f"-KS{ks}-K{K}-" in name
    full = R.knn_ref(q, c, K, 0, mode)
    assert torch.equal(full[..., drop:], R.knn_ref(q, c, k, drop, mode))
    used = R.knn_check_f64(q, c, full, K)
    print(f"{name}: {100 * used:.1f} % of the slack used")
    if family == "same":
        assert torch.equal(full, torch.arange(K).expand(B, nq, K))


def test_knn_case_table_covers_every_path():
    seen = {(R.knn_lanes(c[2], c[3], c[4]), c[1], next(s for s in (1, 2, 5, 8, 11, 16) if c[5] + c[6] <= s))
            for c in R.KNN_CASES}
    assert seen == {(lanes, d, ks) for lanes in (4, 16) for d in (3, 9) for ks in (1, 2, 5, 8, 11, 16)}
    for lanes in (4, 16):
        assert any(R.knn_lanes(c[2], c[3], c[4]) == lanes and c[4] > 1024 for c in R.KNN_CASES)
    assert {c[5] + c[6] for c in R.KNN_CASES} >= {1, 2, 3, 5, 6, 8, 9, 11, 12, 16}
    assert {c[9] for c in R.KNN_CASES} == {"dense", "shared", "strided"}


def test_pool_max_ref_is_pool_layer():
    gen = torch.Generator().manual_seed(1)
    B, n, C = 2, 40, 12
    v = torch.randn(B, n, 3, generator=gen)
    fm = -torch.rand(B, n, C, generator=gen) - 0.5  # all negative: a zero-seeded max would differ
    perm = torch.randperm(n, generator=gen)
    nbr = torch.randint(0, n, (B, n // 4, 4), generator=gen)
    nbr[:, 0] = 7  # a repeated neighbour
    _, pooled, _ = O.Pool_layer()(v, fm, perm=perm, idx_override=nbr)
    assert torch.equal(R.pool_max_ref(fm, nbr), pooled)


def _tiny_tbase(f, gen):
    net = O.TBase(f).eval()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.5 / max(1, p.shape[1] if p.dim() > 1 else 1)) ** 0.5)
        for bn in (net.bn1, net.bn2, net.bn3):
            bn.weight.copy_(1 + 0.2 * torch.randn(bn.weight.shape, generator=gen))
            bn.bias.copy_(0.1 * torch.randn(bn.bias.shape, generator=gen))
            bn.running_mean.copy_(0.1 * torch.randn(bn.bias.shape, generator=gen))
            bn.running_var.copy_(0.5 + torch.rand(bn.bias.shape, generator=gen))
    return net


def test_tbase_tail_ref_is_the_oracle_tail():
    gen = torch.Generator().manual_seed(2)
    B, n, f = 3, 37, 24
    net = _tiny_tbase(f, gen)
    x = torch.randn(B, f, n, generator=gen)
    cloud = torch.tensor([0.02, -0.05, 0.9]) + 0.1 * torch.randn(B, n, 3, generator=gen)
    with torch.no_grad():
        h = torch.relu(net.bn1(net.conv1(x)))
        h = torch.relu(net.bn2(net.conv2(h)))
        h = torch.relu(net.bn3(net.conv3(h)))                             # [B][256][n]
        t_res = net(x)                                                    # TBase.forward: conv4's first three rows
        pred_t = (cloud + t_res.permute(0, 2, 1)).mean(dim=1)             # krrn.py:153
    t, pred, t_bound, p_bound = R.tbase_tail_ref(h.permute(0, 2, 1).contiguous(), net.conv4.weight[:3, :, 0].detach(),
                                                 net.conv4.bias[:3].detach(), cloud)
    # the oracle's f32 sums carry the same operation counts the bounds are written for
    assert ((t - t_res.permute(0, 2, 1).double()).abs() <= t_bound).all()
    assert ((pred - pred_t.double()).abs() <= p_bound + n * R.EPS32 * (cloud.double().abs() + t.abs()).mean(dim=1)).all()
    assert float(t_bound.max()) < 1e-4 and float(p_bound.max()) < 1e-4


def test_gather2_add_ref_is_conv1_on_the_concat():
    """krrn.py:132-141 with fusion.py:234-238: conv1 + bn1 + ReLU over [fm_5[nn2] | feat_1[nn1] | feat_2[nn1]
    | one-hot] equals the two gathered row tables plus the per-crop one-hot column."""
    gen = torch.Generator().manual_seed(3)
    B, n, n1, n2, c5, c1, c2, ncls = 2, 32, 8, 2, 8, 6, 6, 3
    net = _tiny_tbase(c5 + c1 + c2 + ncls, gen)
    fm5, feat1, feat2 = (torch.randn(B, m, c, generator=gen) for m, c in ((n2, c5), (n1, c1), (n1, c2)))
    nn2 = torch.randint(0, n2, (B, n), generator=gen)
    nn1 = torch.randint(0, n1, (B, n), generator=gen)
    cls = torch.tensor([2, 0])
    bi = torch.arange(B)[:, None]
    one_hot = torch.zeros(B, ncls).scatter_(1, cls.view(-1, 1), 1)
    feat = torch.cat([fm5[bi, nn2], feat1[bi, nn1], feat2[bi, nn1], one_hot[:, None].repeat(1, n, 1)], 2)
    with torch.no_grad():
        want = torch.relu(net.bn1(net.conv1(feat.permute(0, 2, 1)))).permute(0, 2, 1)   # [B][n][1024]
    W = net.conv1.weight[:, :, 0].detach().double()
    s = (net.bn1.weight / torch.sqrt(net.bn1.running_var + net.bn1.eps)).detach().double()
    bias = s * (net.conv1.bias.detach().double() - net.bn1.running_mean.double()) + net.bn1.bias.detach().double()
    A = fm5.double() @ W[:, :c5].t()
    Bm = torch.cat([feat1, feat2], 2).double() @ W[:, c5:c5 + c1 + c2].t()
    bias2 = s * W[:, c5 + c1 + c2:][:, cls].t()                            # [B][1024], pre-scaled
    out, _ = R.gather2_add_ref(nn2, A, nn1, Bm, s, bias, bias2, True)
    torch.testing.assert_close(out.float(), want, rtol=1e-5, atol=1e-5)
    assert float(want.max()) > 0.5 and (want == 0).any()


def test_guarded_buffer_finds_stray_writes():
    gd = R.Guarded(2, 3, 4, stride=8, off=4, slack=8)
    vals = torch.arange(24.).view(2, 3, 4)
    gd.fill(vals)
    assert torch.equal(gd.result(), vals)
    assert gd.buf.numel() == 16 + 2 * 32 and gd.offset == 12
    gd.buf[gd.offset + 4] = 0.0  # one past the first row's slice
    with pytest.raises(AssertionError, match="outside the slice"):
        gd.result()
    gi = R.Guarded(1, 2, 3, dtype=torch.int32)
    with pytest.raises(AssertionError, match="left inside"):
        gi.result()
