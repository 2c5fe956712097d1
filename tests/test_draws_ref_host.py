"""tests/draws_ref.py pinned on the CPU: the mixer against splitmix64's published outputs, the draws'
distributions by chi-square over a fixed range of seeds (deterministic; the GPU tests then hold the kernels to
the restatement bit for bit, which carries the distribution over), and the two tie fixtures of the radix
select that tests/test_gpu_inputs.py relies on."""
import math

import numpy as np
import pytest

from tests import draws_ref as D


def chi2_quantile(df: int, tail: float = 1e-6) -> float:
    """The 1 - tail quantile of chi-square(df): scipy.stats.chi2.ppf where scipy imports, else the
    Wilson-Hilferty cube-root normal approximation df * (1 - 2/(9 df) + z sqrt(2/(9 df)))^3 with z the normal
    quantile (4.753424 for 1 - 1e-6). At df = 15 / 63 the two differ by under 2 %."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - tail, df))
    except ImportError:
        assert tail == 1e-6
        z = 4.753424308822899
        return df * (1.0 - 2.0 / (9 * df) + z * math.sqrt(2.0 / (9 * df))) ** 3


def test_wilson_hilferty_is_close_to_the_exact_quantile():
    # chi2.ppf(1 - 1e-6, 15) = 56.493, chi2.ppf(1 - 1e-6, 63) = 131.370 (scipy 1.15); Wilson-Hilferty gives
    # 57.358 and 131.745: either form is within 1 of the exact value
    assert abs(chi2_quantile(15) - 56.493) < 1.0
    assert abs(chi2_quantile(63) - 131.370) < 1.0


def test_mix64_is_splitmix64():
    """The first three outputs of splitmix64 seeded with 0 (state += gamma, then the finaliser)."""
    g = D.GOLDEN
    assert D.mix64(0) == 0xE220A8397B1DCDAF
    assert D.mix64(g) == 0x6E789E6AA1B965F4
    assert D.mix64((2 * g) & D.M64) == 0x06C45D188009454F
    arr = np.array([0, g, (2 * g) & D.M64], dtype=np.uint64)
    assert [int(v) for v in D.mix64(arr)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert D.mix32(g) == 0x6E789E6A and int(D.mix32(arr)[2]) == 0x06C45D18


def test_scalar_and_array_forms_agree():
    for seed, stream, row in [(0, 0, 0), (-1, 5, 3), (123, 2 ** 32 - 1, 0), (-(2 ** 63), 7, 2 ** 32 - 1)]:
        i = np.arange(40, dtype=np.uint64)
        assert [D.rand32(seed, stream, row, int(j)) for j in i] == D.rand32(seed, stream, row, i).tolist()
    k = D.choose_keys(-7, 65534, 2, 30)
    assert k.tolist() == [D.mix32((D.choose_base(-7, 65534, 2) + r) & D.M64) for r in range(30)]


def test_seed_bits_and_advance():
    assert D.u64(-1) == 2 ** 64 - 1 and D.u64(-(2 ** 63)) == 2 ** 63
    assert D.advance(-1) == 0 and D.advance(2 ** 63 - 1) == -(2 ** 63) and D.advance(41, 3) == 44
    # a negative seed is its own stream of draws, not the draws of its magnitude
    assert not np.array_equal(D.randperm(-1, 0, 0, 64, 64), D.randperm(1, 0, 0, 64, 64))


@pytest.mark.parametrize("n,k", [(1, 1), (2, 2), (64, 64), (65, 10), (1025, 1), (4096, 4096)])
def test_randperm_is_a_prefix_of_a_permutation(n, k):
    p = D.randperm(123, 5, 1, n, n)
    assert sorted(p.tolist()) == list(range(n))
    assert np.array_equal(D.randperm(123, 5, 1, n, k), p[:k])
    r = D.rand32(123, 5, 1, np.arange(n, dtype=np.uint64))[p]
    assert all(r[i] < r[i + 1] or (r[i] == r[i + 1] and p[i] < p[i + 1]) for i in range(n - 1))


def test_ransac_subsets_known_structure():
    s = D.ransac_subsets(-1, 6, 2, 50, 5).reshape(-1, 5)
    assert all(sorted(r.tolist()) == [0, 1, 2, 3, 4] for r in s)  # P = 5: the loop must reject its way through
    s = D.ransac_subsets(9, 6, 3, 40, 256).reshape(-1, 5)
    assert all(len(set(r.tolist())) == 5 for r in s) and s.min() >= 0 and s.max() < 256
    # row e = b*H + h: the batch's second crop continues the first's rows
    assert np.array_equal(D.ransac_subsets(9, 6, 1, 120, 256).reshape(-1, 5), s)
    # the first index is the first draw, the counter starting at 0
    assert int(s[7, 0]) == (D.rand32(9, 6, 7, 0) * 256) >> 32


def test_choose_forms():
    m = np.zeros((4, 4), bool)
    m[1, 1] = m[2, 3] = m[3, 0] = True
    assert D.choose(m, 7).tolist() == [5, 11, 12, 5, 11, 12, 5]
    assert D.choose(m, 3).tolist() == [5, 11, 12]
    assert D.choose(np.zeros((4, 4), bool), 5).tolist() == [0] * 5
    full = np.ones((6, 6), bool)
    ch = D.choose(full, 10, seed=3, stream_id=2, crop=1)
    keys = D.choose_keys(3, 2, 1, 36)
    assert np.all(np.diff(ch) > 0) and keys[ch].max() <= np.delete(keys, ch).min()
    with pytest.raises(ValueError):
        D.choose_base(0, 65535, 0)
    with pytest.raises(ValueError):
        D.choose_base(0, -1, 0)


def test_choose_stream_ids_do_not_alias_inside_the_range():
    """(stream_id + 1) << 48 keeps 16 bits: 0 .. 65534 give 65535 distinct non-zero terms (65535 would give 0,
    the base of no stream term at all, and 65536 the term of 0: hence the range)."""
    terms = {((s + 1) << 48) & D.M64 for s in range(D.CHOOSE_STREAM_MAX + 1)}
    assert len(terms) == 65535 and 0 not in terms
    assert ((65535 + 1) << 48) & D.M64 == 0 and ((65536 + 1) << 48) & D.M64 == (1 << 48)


SEEDS = range(3200)


def _pearson(obs, expect):
    return float(((obs - expect) ** 2 / expect).sum())


def test_randperm_slot0_is_uniform():
    """The index in slot 0 of randperm(n = 16) over seeds 0..3199: 16 cells of expectation 200, Pearson's
    statistic against chi-square with 15 degrees of freedom, bounded by its 1 - 1e-6 quantile."""
    obs = np.bincount([int(D.randperm(s, 0, 0, 16, 1)[0]) for s in SEEDS], minlength=16)
    x2 = _pearson(obs, len(SEEDS) / 16)
    print("randperm slot 0: chi2 =", x2, "bound", chi2_quantile(15))
    assert x2 < chi2_quantile(15)


def test_ransac_first_index_is_uniform():
    """The first index of ransac_subsets(P = 16) over seeds 0..3199 (B = H = 1): 16 cells, 15 degrees of freedom."""
    obs = np.bincount([int(D.ransac_subsets(s, 1, 1, 1, 16)[0, 0, 0]) for s in SEEDS], minlength=16)
    x2 = _pearson(obs, len(SEEDS) / 16)
    print("subsets first index: chi2 =", x2, "bound", chi2_quantile(15))
    assert x2 < chi2_quantile(15)


def test_choose_subset_inclusion_is_uniform():
    """Per-rank inclusion counts of choose_subset(count = 64, N = 16) over seeds 0..3199. A uniform N-subset of
    M ranks includes each with p = N/M, and two ranks' indicators have covariance -p(1-p)/(M-1), so over T
    draws the counts' covariance is T p(1-p) M/(M-1) (I - J/M): sum (O - Tp)^2 / (T p (1-p) M/(M-1)) is
    chi-square with M - 1 = 63 degrees of freedom (the counts sum to T N exactly, which takes one)."""
    M, N, T = 64, 16, len(SEEDS)
    obs = np.zeros(M)
    for s in SEEDS:
        obs[D.choose_subset(s, 0, 0, M, N)] += 1
    p = N / M
    assert obs.sum() == T * N
    x2 = float(((obs - T * p) ** 2).sum() / (T * p * (1 - p) * M / (M - 1)))
    print("choose inclusion: chi2 =", x2, "bound", chi2_quantile(63))
    assert x2 < chi2_quantile(63)


TIES = [  # (seed, stream_id, crop, sorted positions of the two equal keys, their ranks), count = 9000
    (185, 0, 0, (790, 791), (1814, 6064)),
    (59, 0, 1, (4834, 4835), (607, 3670)),
]
TIE_COUNT = 9000


@pytest.mark.parametrize("seed,sid,crop,pos,ranks", TIES)
def test_tie_fixtures(seed, sid, crop, pos, ranks):
    """Two of the 9000 keys are equal and sit at the stated neighbouring positions of the (key, rank) order;
    no other two keys are equal, so N = pos[1] takes exactly the lower rank of the pair."""
    keys = D.choose_keys(seed, sid, crop, TIE_COUNT)
    order = np.lexsort((np.arange(TIE_COUNT), keys))
    assert keys[ranks[0]] == keys[ranks[1]] and ranks[0] < ranks[1]
    assert (int(order[pos[0]]), int(order[pos[1]])) == ranks
    ks = keys[order]
    assert np.nonzero(ks[1:] == ks[:-1])[0].tolist() == [pos[0]]
    lo = set(D.choose_subset(seed, sid, crop, TIE_COUNT, pos[1]).tolist())
    assert ranks[0] in lo and ranks[1] not in lo
    both = set(D.choose_subset(seed, sid, crop, TIE_COUNT, pos[1] + 1).tolist())
    assert ranks[0] in both and ranks[1] in both
    none = set(D.choose_subset(seed, sid, crop, TIE_COUNT, pos[1] - 1).tolist())
    assert ranks[0] not in none and ranks[1] not in none
