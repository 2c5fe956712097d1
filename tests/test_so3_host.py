"""csrc/krrn_so3.h on the CPU: the log map that starts BPnP's Levenberg-Marquardt from the RANSAC
rotation, over f32-rounded rotations at the angles where a log map goes wrong (CPU only).

The header compiles as plain host C++, so a small program (tests/so3_host_main.cpp) runs it over
so3_ref.rotation_set(): 0, 1e-7, 1e-4, 1e-2, 0.5, 2 and pi - {1, 1e-1, 1e-2, 1e-3, 3e-4, 1e-4, 1e-5,
1e-7, 0} about 24 random and the three coordinate axes, both signs, plus the three exact 180-degree
diagonal matrices. Measure (so3_ref.rebuild_error): max entry |exp([w]x) - R| with the returned w
rounded to f32 and R the f64 value of the f32 input.

Bound: 4 x the largest such error of so3_ref.log_ref (Shepperd's quaternion, f64) over the same
set. Measured on the CPU: log_ref 1.248e-7 (the input's own f32 rounding plus that of an output vector
of length pi), so the bound is 4.99e-7; the header 1.248e-7 (the same matrix, at pi - 3e-4); the parent
commit's function (so3_ref.log_parent, and the C++ itself before the change) 2.0: a rotation rebuilt
the wrong way round from pi - 1e-3 on (0.075 there, 1.2 at pi - 1e-4), and w = 0 at pi exactly."""
import os
import subprocess

import numpy as np
import pytest

import so3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="no ROCm clang++")


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """(R f32, angle, the header's w f64, the reference's error per matrix)."""
    tmp = tmp_path_factory.mktemp("so3_host")
    exe = str(tmp / "so3_host")
    subprocess.check_call([CLANG, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "pose_estimation_amd", "csrc"),
                           os.path.join(ROOT, "tests", "so3_host_main.cpp"), "-o", exe])
    R, ang = so3_ref.rotation_set()
    R.tofile(str(tmp / "R.f32"))
    subprocess.check_call([exe, str(tmp / "R.f32"), str(tmp / "w.f64")])
    w = np.fromfile(str(tmp / "w.f64"), dtype=np.float64).reshape(-1, 3)
    assert w.shape == (len(R), 3)
    return R, ang, w, so3_ref.rebuild_error(so3_ref.log_ref(R), R)


def test_reference_log_is_tight(case):
    """The bound's own basis: the reference rebuilds every matrix to f32 rounding (a loose reference
    would make 4 x its error a loose bound)."""
    R, ang, _, ref_err = case
    assert ref_err.max() < 3e-7, (ref_err.max(), ang[ref_err.argmax()])


def test_reference_log_equals_scipy(case):
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    R = case[0]
    got = so3_ref.rebuild_error(Rotation.from_matrix(R.astype(np.float64)).as_rotvec(), R)
    assert got.max() < 3e-7, got.max()


def test_rot_log_rebuilds_rotation(case):
    R, ang, w, ref_err = case
    err = so3_ref.rebuild_error(w, R)
    print(f"rot_log max rebuild error {err.max():.3e} at angle {ang[err.argmax()]!r}; reference {ref_err.max():.3e}")
    assert np.isfinite(w).all()
    assert err.max() <= 4 * ref_err.max(), (err.max(), ang[err.argmax()], ref_err.max())
    assert (np.linalg.norm(w, axis=1) <= np.pi + 1e-12).all()


def test_set_tells_parent_function_apart(case):
    """The same set under the former rule (angle and branch from acos of the trace alone) misses the
    bound by orders of magnitude: the set reaches the angles where that rule breaks."""
    R, ang, _, ref_err = case
    err = so3_ref.rebuild_error(so3_ref.log_parent(R), R)
    assert err.max() > 1000 * 4 * ref_err.max(), err.max()
    near_pi = np.pi - ang < 0.05
    assert err[~near_pi].max() < 1e-4  # and it was right away from pi: only that neighbourhood moved
