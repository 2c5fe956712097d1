"""Lane layout of v_mfma_f32_4x4x1_16b_f32 on the hardware (krrn_mfma4x4_probe_f32: one wave, one MFMA)
against a plain loop. conv_small's ragged channel tail relies on it: sixteen independent 4x4x1 blocks,
block b = lanes 4b .. 4b+3; row i of the first operand from lane 4b + i, column j of the second from
lane 4b + j; lane l's result register i = row i, column l % 4 of block l / 4."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _probe(dev, a, b, c):
    from pose_estimation_amd import _lib
    from pose_estimation_amd.runtime import P, ptr
    ad, bd, cd = a.to(dev).contiguous(), b.to(dev).contiguous(), c.to(dev).contiguous()
    d = torch.full((64, 4), float("nan"), device=dev)
    _lib.check(_lib.lib().krrn_mfma4x4_probe_f32(ptr(ad), ptr(bd), ptr(cd), ptr(d),
                                                 P(torch.cuda.current_stream().cuda_stream)), "mfma4x4 probe")
    torch.cuda.synchronize()
    return d.cpu()


def _loop(a, b, c):
    d = torch.empty(64, 4)
    for blk in range(16):
        for i in range(4):        # row: first operand, result register
            for j in range(4):    # column: second operand, result lane
                d[4 * blk + j, i] = c[4 * blk + j, i] + a[4 * blk + i] * b[4 * blk + j]
    return d


def test_mfma4x4_lane_layout(dev):
    lanes = torch.arange(64, dtype=torch.float32)
    one, zero = torch.ones(64), torch.zeros(64, 4)
    # rows alone (second operand 1): register i of lane l is the first operand of lane 4 (l / 4) + i
    da = _probe(dev, 1 + lanes, one, zero)
    assert torch.equal(da, _loop(1 + lanes, one, zero))
    assert torch.equal(da, (1 + 4 * (lanes[:, None] // 4) + torch.arange(4.0)[None, :]))
    # columns alone (first operand 1): every register of lane l is lane l's own second operand
    db = _probe(dev, one, 1 + lanes, zero)
    assert torch.equal(db, (1 + lanes)[:, None].expand(64, 4))
    # both, on top of an index-coded accumulator (small integers: every product and sum is exact)
    a, b = 1 + lanes, 67 + 3 * lanes
    c = (1000 * (1 + lanes))[:, None] + 7 * torch.arange(4.0)[None, :]
    assert torch.equal(_probe(dev, a, b, c), _loop(a, b, c))


def test_mfma4x4_blocks_are_independent(dev):
    """A NaN in one block's operands stays in that block's 4 lanes."""
    a, b = torch.ones(64), torch.ones(64)
    a[4 * 5 + 2] = float("nan")
    d = _probe(dev, a, b, torch.zeros(64, 4))
    bad = torch.isnan(d)
    want = torch.zeros(64, 4, dtype=torch.bool)
    want[20:24, 2] = True  # block 5, row 2, every column
    assert torch.equal(bad, want)
    assert torch.equal(d[~bad], torch.ones(int((~bad).sum())))
