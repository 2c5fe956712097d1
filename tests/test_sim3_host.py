"""csrc/krrn_umeyama.h on the CPU: umeyama_solve, the one-sided Jacobi SVD with the signed third singular
value that decides every Umeyama hypothesis, every refit and every ICP update, over covariances at the
places where a 3x3 SVD goes wrong (CPU only).

The header compiles as plain host C++, so a small program (tests/sim3_host_main.cpp, built with ROCm's
clang++ -O2 -ffp-contract=off as the kernels are) runs it over covariance_set(): PER_KIND seeded
covariances U diag(d) V^T of each kind in KINDS (generic, reflections, exact rank 2 of either
orientation, repeated leading / trailing values, a trailing pair equal and opposite, isotropic, scaled by
1e-12 and 1e+6, 1 : 1e-3 : 1e-9, a leading pair of 1e-13) and the FIXED list (identity, diag(1, 1, -1),
diag(-1, -1, 1), a cyclic permutation, diag(2, 1, 0), diag(2, -1, 0), and the two rank-deficient ones: the
zero matrix and diag(1, 0, 0)), each with its own centroids and source variance.

Measures, none of which depends on which of several optimal rotations is returned (d: numpy's singular
values with the reference's sign rule on the third):
    orth   max |R R^T - I|
    det    |det R - 1|
    trace  |tr(R^T Cov) - (d1 + d2 + d3)| / d1     (R attains the maximum of tr(R^T Cov) over SO(3))
    scale  |s varP - (d1 + d2 + d3)| / d1
Bound: each at most 4 x the largest value the numpy solution (solve_ref, the lines of
umeyama_ref.umeyama on a covariance) shows over the same set. Measured on the CPU:
    numpy   orth 2.22e-15  det 2.66e-15  trace 1.81e-15  scale 6.58e-16
    header  orth 1.55e-15  det 1.78e-15  trace 2.19e-15  scale 2.19e-15
so nothing needed fixing. R entry by entry against umeyama_ref.umeyama only for the kinds whose optimum
is unique (the True entries of KINDS and FIXED), within R_BOUND_EPS * eps * d1 / (d2 + d3): the rotation is the
polar factor of Cov,
whose first-order sensitivity to a perturbation E of Cov is |E| / (d2 + d3) (the smallest sum of two signed
singular values); either SVD is backward stable, |E| <= c eps d1 with c a small multiple of the dimension,
and two solutions are compared, so 64 eps d1 / (d2 + d3) leaves c = 32 for a 3x3 problem. Measured: at most
0.68 of that bound. t against mT - s R mS from the header's own s and R: the three products and sums of
its last line, 8 eps (|mT| + 3 |s| |mS|).

The zero matrix and diag(1, 0, 0) have no second direction: the header returns NaN for s, R and t (ICP's
DEGENERATE and Umeyama's zero count rest on that; the header's comment says so), and the driver built once
more with -fsanitize=address,undefined runs over the same file and exits clean."""
import os
import subprocess

import numpy as np
import pytest

import umeyama_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="no ROCm clang++")

PER_KIND = 300
EPS = np.finfo(np.float64).eps
R_BOUND_EPS = 64.0
# kind -> is the optimal rotation unique (Cov of rank >= 2 and d2 + d3 > 0 with the signed d3)
KINDS = {
    "generic": True, "reflection": True, "rank2": True, "rank2_reflected": True, "equal_leading": True,
    "equal_trailing": True, "trailing_opposite": False, "isotropic": True, "isotropic_reflected": False,
    "scaled_1e-12": True, "scaled_1e+6": True, "ratio_1_1e-3_1e-9": True, "leading_pair_1e-13": True,
}
FIXED = [
    ("identity", np.eye(3), True),
    ("diag(1,1,-1)", np.diag([1.0, 1.0, -1.0]), False),
    ("diag(-1,-1,1)", np.diag([-1.0, -1.0, 1.0]), True),
    ("cyclic", np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), True),
    ("diag(2,1,0)", np.diag([2.0, 1.0, 0.0]), True),
    ("diag(2,-1,0)", np.diag([2.0, -1.0, 0.0]), True),
    ("zero", np.zeros((3, 3)), None),          # None: rank below 2, no rotation
    ("diag(1,0,0)", np.diag([1.0, 0.0, 0.0]), None),
]
# eight points with mean 0 and S^T S = 2 I exactly: T = 4 S Cov^T has the covariance Cov bit for bit
S8 = np.concatenate([np.eye(3), -np.eye(3), np.zeros((2, 3))])


def _orth(rng, det):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) * det < 0:
        q[:, 2] = -q[:, 2]
    return q


def _cov(rng, kind):
    """One covariance of the kind: U diag(d) V^T with det(U) det(V) = sign."""
    sign = -1.0 if kind in ("reflection", "trailing_opposite", "isotropic_reflected") else 1.0
    if kind.startswith("rank2"):
        while True:  # small integers: the products and sums are exact, so the rank is exactly 2
            a, b, c, d = rng.integers(-8, 9, size=(4, 3)).astype(np.float64)
            C = np.outer(a, b) + np.outer(c, d)
            sv = np.linalg.svd(C, compute_uv=False)
            if sv[1] > 0.05 * sv[0]:
                return C @ np.diag([1.0, 1.0, -1.0]) if kind == "rank2_reflected" else C
    u = np.sort(rng.uniform(0.05, 1.0, 3))[::-1]
    d = {
        "generic": u, "reflection": u,
        "equal_leading": np.array([u[0], u[0], u[2]]),
        "equal_trailing": np.array([u[0], u[2], u[2]]),
        "trailing_opposite": np.array([u[0], u[2], u[2]]),
        "isotropic": np.array([u[0]] * 3), "isotropic_reflected": np.array([u[0]] * 3),
        "scaled_1e-12": 1e-12 * u, "scaled_1e+6": 1e6 * u,
        "ratio_1_1e-3_1e-9": u[0] * np.array([1.0, 1e-3, 1e-9]),
        "leading_pair_1e-13": np.array([1e-13, 1e-13, 1e-13 * u[2]]),
    }[kind]
    return _orth(rng, 1.0) @ np.diag(d) @ _orth(rng, sign).T


def covariance_set():
    """(names, unique flags (None: rank below 2), records [n, 16] = mS, mT, Cov, varP)."""
    names, unique, rec = [], [], []
    for k, kind in enumerate(KINDS):
        rng = np.random.default_rng(4100 + k)
        for _ in range(PER_KIND):
            names.append(kind)
            unique.append(KINDS[kind])
            rec.append(np.concatenate([rng.normal(scale=0.05, size=3), rng.normal(size=3) * [0.1, 0.1, 1.0],
                                       _cov(rng, kind).ravel(), [rng.uniform(1e-3, 2.0)]]))
    rng = np.random.default_rng(4099)
    for name, C, uq in FIXED:
        names.append(name)
        unique.append(uq)
        rec.append(np.concatenate([rng.normal(scale=0.05, size=3), rng.normal(size=3), C.ravel(), [0.75]]))
    return names, unique, np.array(rec)


def solve_ref(rec):
    """umeyama_ref.umeyama's lines on a record's covariance: (s, R, t, signed d)."""
    mS, mT, cov, varP = rec[:3], rec[3:6], rec[6:15].reshape(3, 3), rec[15]
    U, D, Vh = np.linalg.svd(cov, full_matrices=True)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0.0:
        D[-1] = -D[-1]
        U[:, -1] = -U[:, -1]
    R = U @ Vh
    s = 1 / varP * np.sum(D)
    return s, R, mT - mS.dot(s * R.T), D


def measures(s, R, rec, d):
    cov, varP = rec[6:15].reshape(3, 3), rec[15]
    return dict(orth=np.abs(R @ R.T - np.eye(3)).max(), det=abs(np.linalg.det(R) - 1.0),
                trace=abs(np.trace(R.T @ cov) - d.sum()) / d[0], scale=abs(s * varP - d.sum()) / d[0])


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sim3_host")
    names, unique, rec = covariance_set()
    rec.tofile(str(tmp / "rec.f64"))
    base = [CLANG, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "pose_estimation_amd", "csrc"),
            os.path.join(ROOT, "tests", "sim3_host_main.cpp")]
    exe = str(tmp / "sim3_host")
    subprocess.check_call(base + ["-o", exe])
    subprocess.check_call([exe, str(tmp / "rec.f64"), str(tmp / "out.f64")])
    out = np.fromfile(str(tmp / "out.f64"), dtype=np.float64).reshape(-1, 13)
    assert out.shape[0] == len(rec)
    ref = [solve_ref(r) for r in rec]
    full = np.array([u is not None for u in unique])
    worst = {"ref": {}, "hdr": {}}
    for i in np.nonzero(full)[0]:
        for who, (s, R) in (("ref", ref[i][:2]), ("hdr", (out[i, 0], out[i, 1:10].reshape(3, 3)))):
            for k, v in measures(s, R, rec[i], ref[i][3]).items():
                if not v <= worst[who].get(k, (-1.0, ""))[0]:  # (a NaN takes the place and fails the bound)
                    worst[who][k] = (v, names[i])
    return dict(tmp=tmp, base=base, names=names, unique=unique, rec=rec, out=out, ref=ref, worst=worst)


def test_set_holds_every_kind(case):
    names, rec = case["names"], case["rec"]
    assert len(rec) == PER_KIND * len(KINDS) + len(FIXED) and PER_KIND >= 200
    sv = np.linalg.svd(rec[:, 6:15].reshape(-1, 3, 3), compute_uv=False)
    det = np.linalg.det(rec[:, 6:15].reshape(-1, 3, 3))
    k = lambda name: np.array([n == name for n in names])  # noqa: E731
    assert (det[k("reflection")] < 0).all() and (det[k("generic")] > 0).all()
    assert (sv[k("rank2") | k("rank2_reflected"), 2] <= 1e-14 * sv[k("rank2") | k("rank2_reflected"), 0]).all()
    assert (np.abs(sv[k("equal_leading"), 0] - sv[k("equal_leading"), 1]) <= 4 * EPS).all()
    for name in ("equal_trailing", "trailing_opposite"):
        assert (np.abs(sv[k(name), 1] - sv[k(name), 2]) <= 4 * EPS).all()
    assert (det[k("trailing_opposite")] < 0).all() and (det[k("isotropic_reflected")] < 0).all()
    assert (sv[k("isotropic"), 0] - sv[k("isotropic"), 2] <= 4 * EPS).all()
    assert sv[k("scaled_1e-12"), 0].max() < 1e-12 and sv[k("scaled_1e+6"), 0].min() > 1e4
    r = sv[k("ratio_1_1e-3_1e-9")]
    assert np.allclose(r[:, 1] / r[:, 0], 1e-3, rtol=1e-6) and np.allclose(r[:, 2] / r[:, 0], 1e-9, rtol=1e-4)
    assert np.allclose(sv[k("leading_pair_1e-13"), :2], 1e-13, rtol=1e-9)


def test_reference_is_tight(case):
    """The bound's own basis: the numpy solution meets every measure to rounding (a loose reference would
    make 4 x its error a loose bound)."""
    w = case["worst"]["ref"]
    print("numpy  ", "  ".join(f"{k} {v[0]:.2e} ({v[1]})" for k, v in w.items()))
    assert all(v[0] < 1e-14 for v in w.values()), w


def test_reference_is_umeyama_ref_on_points(case):
    """solve_ref is umeyama_ref.umeyama: on eight points whose covariance is the record's bit for bit, the
    same scale and rotation (the same LAPACK call on the same matrix)."""
    for i in range(0, len(case["rec"]), 97):
        if case["unique"][i] is None:
            continue
        C = case["rec"][i, 6:15].reshape(3, 3)
        s, R, t, _ = ur.umeyama(S8, 4.0 * S8 @ C.T)
        assert np.array_equal(R, case["ref"][i][1]), case["names"][i]
        assert abs(s * 0.75 - case["ref"][i][3].sum()) <= 4 * EPS * case["ref"][i][3][0]


def test_umeyama_solve_meets_the_measures(case):
    ref, hdr = case["worst"]["ref"], case["worst"]["hdr"]
    print("numpy  ", "  ".join(f"{k} {v[0]:.2e} ({v[1]})" for k, v in ref.items()))
    print("header ", "  ".join(f"{k} {v[0]:.2e} ({v[1]})" for k, v in hdr.items()))
    full = np.array([u is not None for u in case["unique"]])
    assert np.isfinite(case["out"][full]).all()
    for k in ("orth", "det", "trace", "scale"):
        assert hdr[k][0] <= 4 * ref[k][0], (k, hdr[k], ref[k])


def test_unique_rotations_equal_umeyama_ref(case):
    worst = 0.0
    n = 0
    for i, uq in enumerate(case["unique"]):
        if not uq:
            continue
        C = case["rec"][i, 6:15].reshape(3, 3)
        _, Rr, _, _ = ur.umeyama(S8, 4.0 * S8 @ C.T)
        d = case["ref"][i][3]
        bound = R_BOUND_EPS * EPS * d[0] / (d[1] + d[2])
        err = np.abs(case["out"][i, 1:10].reshape(3, 3) - Rr).max()
        worst = max(worst, err / bound)
        n += 1
        assert err <= bound, (case["names"][i], err, bound)
    print(f"{n} unique optima: worst |R - R_ref| / bound {worst:.3f}")
    assert n >= PER_KIND * 10


def test_translation_is_consistent(case):
    for i, uq in enumerate(case["unique"]):
        if uq is None:
            continue
        rec, o = case["rec"][i], case["out"][i]
        s, R, t = o[0], o[1:10].reshape(3, 3), o[10:13]
        lim = 8 * EPS * (np.abs(rec[3:6]).max() + 3 * abs(s) * np.abs(rec[:3]).max())
        assert np.abs(t - (rec[3:6] - s * R @ rec[:3])).max() <= lim, case["names"][i]


def test_rank_deficient_covariances_are_non_finite(case):
    """No second direction: NaN throughout, which is what ICP's DEGENERATE and a zero Umeyama count test for."""
    idx = [i for i, u in enumerate(case["unique"]) if u is None]
    assert [case["names"][i] for i in idx] == ["zero", "diag(1,0,0)"]
    for i in idx:
        assert np.isnan(case["out"][i]).all(), case["names"][i]  # s, every entry of R, t
        assert ur_kabsch_is_none(case["rec"][i, 6:15].reshape(3, 3))


def ur_kabsch_is_none(C):
    """icp_ref.kabsch's own test of the same covariance (second singular value 0)."""
    D = np.linalg.svd(C, compute_uv=False)
    return not (np.isfinite(D).all() and D[1] > 0.0)


def test_sanitized_driver_exits_clean(case):
    """The stand-alone driver under AddressSanitizer and UBSan over the same file, the rank-deficient records
    included: exit status 0, no report, the same bytes out."""
    tmp = case["tmp"]
    exe = str(tmp / "sim3_host_san")
    subprocess.check_call(case["base"] + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe])
    p = subprocess.run([exe, str(tmp / "rec.f64"), str(tmp / "out_san.f64")], capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
    got = np.fromfile(str(tmp / "out_san.f64"), dtype=np.float64).reshape(-1, 13)
    assert np.array_equal(got, case["out"], equal_nan=True)
