"""Plain statement of krrn_pair_compact_i32 (include/krrn_hip.h): the distinct (ia, ib) pairs of every
crop in ascending key order (key = ia * n2 + ib), each point's rank among them, and the padding rule
(entries past cnt repeat entry 0). Test infrastructure: torch.unique on the CPU, one crop at a time."""
import torch


def pair_compact_ref(ia: torch.Tensor, ib: torch.Tensor, n1: int, n2: int):
    """ia, ib: integer [B, npts] with values < n1 / < n2. Returns (cnt [B], pa [B, npts], pb [B, npts],
    slot [B, npts]) as int32."""
    ia, ib = ia.cpu().long(), ib.cpu().long()
    assert ia.shape == ib.shape and ia.dim() == 2
    assert int(ia.min()) >= 0 and int(ia.max()) < n1 and int(ib.min()) >= 0 and int(ib.max()) < n2
    B, npts = ia.shape
    cnt = torch.zeros(B, dtype=torch.int32)
    pa = torch.zeros(B, npts, dtype=torch.int32)
    pb = torch.zeros(B, npts, dtype=torch.int32)
    slot = torch.zeros(B, npts, dtype=torch.int32)
    for b in range(B):
        keys, inv = torch.unique(ia[b] * n2 + ib[b], sorted=True, return_inverse=True)
        c = keys.numel()
        cnt[b] = c
        pa[b, :c] = (keys // n2).int()
        pb[b, :c] = (keys % n2).int()
        pa[b, c:] = pa[b, 0]
        pb[b, c:] = pb[b, 0]
        slot[b] = inv.int()
    return cnt, pa, pb, slot
