"""hrnet._Builder.small_problem's mfma_flops states what krrn_conv_small_f32 issues: 16 rows per full
16-channel tile, 4 for a one-quad tail when a wave runs at least 8 K steps, 16 for a longer or short-K
(padded) one, nothing for tile slots past N (no GPU needed)."""
import pytest
import torch
import torch.nn as nn

from pose_estimation_amd import ops
from pose_estimation_amd.hrnet import _Builder


def _issued_rows(np_, ksteps, ks):
    full, rem = divmod(np_, 16)
    steps_per_wave = -(-ksteps // ks)
    return 16 * full + {0: 0, 4: 4 if steps_per_wave >= 8 else 16, 8: 16, 12: 16}[rem]


@pytest.mark.parametrize("np_,ksteps,ks,rows", [
    (4, 12, 1, 4), (8, 12, 1, 16), (12, 12, 1, 16), (16, 12, 1, 16), (20, 12, 1, 20), (36, 21, 2, 36), (44, 21, 1, 48),
    (72, 41, 4, 80), (144, 81, 4, 144),
    # short reductions keep the padded tile: 5 steps over 4 waves, 8 steps (the threshold), 7, 29 and 28 over 4
    (36, 5, 4, 48), (20, 8, 1, 20), (20, 7, 1, 32), (36, 29, 4, 36), (36, 28, 4, 48)])
def test_small_conv_rows(np_, ksteps, ks, rows):
    assert ops.small_conv_rows(np_, ksteps, ks) == rows == _issued_rows(np_, ksteps, ks)


@pytest.mark.parametrize("c,side,k,st", [(18, 30, 3, 1), (36, 15, 3, 1), (72, 8, 3, 1), (144, 4, 3, 1),
                                         (72, 8, 1, 1), (36, 15, 3, 2)])
def test_small_problem_mfma_flops(c, side, k, st):
    """The four W18 branch shapes (N = 20, 36, 72, 144 after pad4), a 1x1 and a stride-2 conv."""
    B = 2
    cout = {(72, 1, 1): 36, (36, 3, 2): 72}.get((c, k, st), c)
    conv = nn.Conv2d(c, cout, k, st, (k - 1) // 2, bias=False)
    spec = ops.make_conv(conv, nn.BatchNorm2d(cout).eval(), torch.device("cpu"), cin_p=ops.pad4(c))
    x = ops.new_act(B, side, side, c, "cpu")
    Ho, Wo = ops.conv_out_hw(spec, side, side)
    out = ops.new_act(B, Ho, Wo, cout, "cpu")
    p = _Builder.small_problem(x, spec, out, None, True)
    np_ = ops.pad4(cout)
    assert p["N"] == np_ and p["M"] == B * Ho * Wo
    ksteps = (k * k * ops.pad4(c) // 4 + 3) // 4      # 16-wide K steps, each 4 MFMAs deep per tile
    assert p["mfma_flops"] == 2.0 * 16 * ksteps * _issued_rows(np_, ksteps, p["ks"]) * p["M"]
    assert p["flops"] == 2.0 * c * cout * k * k * p["M"]
    assert p["mfma_flops"] >= 2.0 * ops.pad4(c) * np_ * k * k * p["M"]  # never below the padded problem
