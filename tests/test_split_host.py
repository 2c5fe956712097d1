"""The device split (csrc/krrn_split.h) and the host split (ops.split_bf16x3) are one contract (CPU only).

Activations are split in the kernels by krrn_split3 / krrn_split3_pair, weights on the host by
ops.split_bf16x3; a disagreement between the two would leave a conv slightly wrong and still inside
the 1e-3 parity tolerances. The header also compiles as plain host C++, so a small program
(tests/split_host_main.cpp) runs it on the CPU and this test holds it to the host split bit for bit,
and both to x = h + m + l exactly, with no exception allowed.

Range: |x| in [2^-100, 2^100] or zero. Near FLT_MAX h rounds to infinity (l is then a NaN) and for
f32 denormals the three terms do not hold x exactly; neither occurs in weights or activations."""
import os
import subprocess

import numpy as np
import pytest
import torch

from pose_estimation_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
N_RANDOM = 60000


def _inputs() -> torch.Tensor:
    g = torch.Generator().manual_seed(20)
    x = torch.randn(N_RANDOM, generator=g, dtype=torch.float64)
    x = x * torch.pow(2.0, torch.randint(-40, 41, (N_RANDOM,), generator=g).double())
    ties = [1 + 2.0**-8, -(1 + 2.0**-8), 1 + 3 * 2.0**-8, -(1 + 3 * 2.0**-8), 1 + 2.0**-8 + 2.0**-16,
            1 + 2.0**-8 + 2.0**-23, 1 + 2.0**-8 - 2.0**-23, 1 + 2.0**-16, 1 + 2.0**-23, 0.0, -0.0, 1.0, -1.0,
            2.0**-100, -(2.0**-100), 2.0**100, -(2.0**100), 2.0**100 * (1 - 2.0**-24), 2.0**-100 * (1 + 2.0**-23)]
    x = torch.cat([x, torch.tensor(ties, dtype=torch.float64)])
    xf = x.float()
    assert torch.equal(xf.double()[N_RANDOM:], x[N_RANDOM:])  # the edge values are f32 numbers
    a = xf.abs()
    assert bool(((a == 0) | ((a >= 2.0**-100) & (a <= 2.0**100))).all())
    pad = (-xf.numel()) % 4
    return torch.cat([xf, torch.ones(pad)])


@pytest.fixture(scope="module")
def device_split(tmp_path_factory):
    """x and the six uint16 planes (split3 h m l, split3_pair h m l) the host build of the header gives."""
    tmp = tmp_path_factory.mktemp("split_host")
    exe = str(tmp / "split_host")
    subprocess.check_call([CLANG, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "pose_estimation_amd", "csrc"),
                           os.path.join(ROOT, "tests", "split_host_main.cpp"), "-o", exe])
    x = _inputs()
    x.numpy().tofile(str(tmp / "x.f32"))
    subprocess.check_call([exe, str(tmp / "x.f32"), str(tmp / "out.u16")])
    out = np.fromfile(str(tmp / "out.u16"), dtype=np.uint16)
    assert out.size == 6 * x.numel()
    return x, torch.from_numpy(out.view(np.int16)).view(torch.bfloat16).view(6, x.numel())


pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="no ROCm clang++")


@pytest.mark.parametrize("form", ["split3", "split3_pair"])
def test_device_split_equals_host_split(device_split, form):
    x, planes = device_split
    got = planes[:3] if form == "split3" else planes[3:]
    for name, g, r in zip("hml", got, ops.split_bf16x3(x)):
        bad = g.view(torch.int16) != r.view(torch.int16)
        assert int(bad.sum()) == 0, (form, name, int(bad.sum()), x[bad][:5].tolist())


@pytest.mark.parametrize("form", ["split3", "split3_pair"])
def test_device_split_is_exact(device_split, form):
    x, planes = device_split
    h, m, l = planes[:3] if form == "split3" else planes[3:]
    s = h.double() + m.double() + l.double()
    bad = s != x.double()
    assert int(bad.sum()) == 0, (form, int(bad.sum()), x[bad][:5].tolist())
