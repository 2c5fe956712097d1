"""tests/pairs_ref.py (the reference the GPU test holds krrn_pair_compact_i32 to) on hand-made cases."""
import torch

from pairs_ref import pair_compact_ref


def test_hand_made_crop():
    # keys with n2 = 4: (2,1)=9 (0,3)=3 (2,1)=9 (1,0)=4 (0,3)=3 -> distinct 3, 4, 9
    ia = torch.tensor([[2, 0, 2, 1, 0]])
    ib = torch.tensor([[1, 3, 1, 0, 3]])
    cnt, pa, pb, slot = pair_compact_ref(ia, ib, 3, 4)
    assert cnt.tolist() == [3]
    assert pa.tolist() == [[0, 1, 2, 0, 0]]  # entries 3, 4 repeat entry 0 = (0, 3)
    assert pb.tolist() == [[3, 0, 1, 3, 3]]
    assert slot.tolist() == [[2, 0, 2, 1, 0]]
    assert cnt.dtype == pa.dtype == pb.dtype == slot.dtype == torch.int32


def test_one_pair_and_all_distinct():
    ia = torch.tensor([[4, 4, 4], [2, 1, 0]])
    ib = torch.tensor([[1, 1, 1], [0, 0, 0]])
    cnt, pa, pb, slot = pair_compact_ref(ia, ib, 5, 2)
    assert cnt.tolist() == [1, 3]
    assert pa.tolist() == [[4, 4, 4], [0, 1, 2]] and pb.tolist() == [[1, 1, 1], [0, 0, 0]]
    assert slot.tolist() == [[0, 0, 0], [2, 1, 0]]


def test_rows_rebuild_the_pairs():
    """(pa, pb)[slot[i]] is point i's pair; the keys of the first cnt entries ascend strictly."""
    g = torch.Generator().manual_seed(0)
    n1, n2 = 7, 5
    ia = torch.randint(0, n1, (3, 40), generator=g)
    ib = torch.randint(0, n2, (3, 40), generator=g)
    cnt, pa, pb, slot = pair_compact_ref(ia, ib, n1, n2)
    for b in range(3):
        s = slot[b].long()
        assert torch.equal(pa[b][s].long(), ia[b]) and torch.equal(pb[b][s].long(), ib[b])
        c = int(cnt[b])
        keys = pa[b, :c].long() * n2 + pb[b, :c]
        assert bool((keys[1:] > keys[:-1]).all()) and int(slot[b].max()) == c - 1
        assert bool((pa[b, c:] == pa[b, 0]).all()) and bool((pb[b, c:] == pb[b, 0]).all())
