"""Builds tests/golden/umeyama_scenes.npz by RUNNING the reference's own
lib/transform/umeyama.py:estimateSimilarityTransform (pure numpy) on synthetic 3D-3D scenes and
recording its inputs, the samples it drew and its results (recorded data only, no reference text).
Run where the reference is checked out (it is not on the GPU box):

    python tests/golden/make_umeyama_golden.py /path/to/pose_estimation

Per scene: np.random.seed(k); estimateSimilarityTransform(src, dst); np.random.seed(k) again and
np.random.randint(N, size=5) replayed 128 times = the subsets the reference drew (it draws nothing
else). Scenes: LineMOD extent / lfborder of tests/test_gpu_pnp._scene, a random pose, ~0.9 m depth.
A seed is kept only if the conditions of tests/umeyama_ref.py hold (every sampled scale finite and
positive, sigma ratios, threshold and early-stop margins) and the restatement fed the replayed
subsets reproduces the reference within 1e-12; otherwise the next seed is tried.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import umeyama_ref as ur  # noqa: E402

if len(sys.argv) < 2:
    raise SystemExit(__doc__)
sys.path.insert(0, sys.argv[1])
from lib.transform.umeyama import estimateSimilarityTransform  # noqa: E402

EXT = np.array([0.067, 0.1276, 0.1175])
LFB = np.array([-0.0335, -0.0638, -0.0587])
H = 128

# name: (N, outlier fraction, noise [m], planar, scale, extra check on the restatement's result)
SCENES = {
    "exact": (64, 0.0, 0.0, False, 1.0, lambda r, sub: r["stop"] == 1),
    "tail": (257, 0.3, 1e-3, False, 1.0, lambda r, sub: any(len(set(row)) < 5 for row in sub.tolist())),
    "long": (500, 0.5, 2e-3, False, 1.0, lambda r, sub: r["stop"] >= 100),
    "planar": (300, 0.2, 1e-3, True, 1.0, lambda r, sub: True),
    "scaled": (333, 0.2, 1e-3, False, 1.7, lambda r, sub: True),
    "fail": (1000, 0.92, 2e-3, False, 1.0, lambda r, sub: r["failed"]),
}


def rodrigues(v):
    th = np.linalg.norm(v)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_scene(rng, N, out_frac, noise, planar, scale):
    u = rng.random((N, 3)).astype(np.float32)
    if planar:
        u[:, 2] = np.float32(0.5)
    src = (u.astype(np.float64) * EXT + LFB).astype(np.float32)
    R = rodrigues(rng.normal(size=3))
    t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.1)])
    dst = scale * src.astype(np.float64) @ R.T + t
    if noise:
        dst += rng.normal(scale=noise, size=dst.shape)
    out = rng.random(N) < out_frac
    dst[out] = t + rng.uniform(-0.15, 0.15, size=(int(out.sum()), 3))
    return src, dst.astype(np.float32)


def record(name, spec):
    N, out_frac, noise, planar, scale, extra = spec
    for k in range(1000):
        rng = np.random.default_rng([k, sum(map(ord, name))])
        src, dst = make_scene(rng, N, out_frac, noise, planar, scale)
        np.random.seed(k)
        with contextlib.redirect_stdout(io.StringIO()):
            s, R, t, _ = estimateSimilarityTransform(src, dst)
        np.random.seed(k)
        sub = np.stack([np.random.randint(N, size=5) for _ in range(H)]).astype(np.int32)
        res = ur.ransac(src, dst, sub)
        try:
            ur.check_conditions(res)
            assert extra(res, sub)
            assert res["failed"] == (s is None)
            if s is not None:
                assert abs(res["scale"] - s) <= 1e-12 and np.abs(res["R"] - R).max() <= 1e-12
                assert np.abs(res["t"] - t).max() <= 1e-12
        except AssertionError:
            continue
        m = res["margins"]
        print(f"{name}: seed {k}, N {N}, stop {res['stop']}, best {res['best_hyp']} ({res['inliers']} inliers), "
              f"margins thr {m['thr']:.2e} sigma {m['sigma']:.3f} refit sigma {m['refit_sigma']:.3f} "
              f"stop {m['stop']:.2e}")
        failed = s is None
        return dict(src=src, dst=dst, subsets=sub, failed=np.array(failed),
                    scale=np.array(1.0 if failed else s, np.float64),
                    R=np.eye(3) if failed else np.asarray(R, np.float64),
                    t=np.zeros(3) if failed else np.asarray(t, np.float64))
    raise SystemExit(f"no seed satisfies the conditions for scene {name}")


arrays = {}
for name, spec in SCENES.items():
    for key, v in record(name, spec).items():
        arrays[f"{name}_{key}"] = v
arrays["names"] = np.array(list(SCENES))
out = os.path.join(HERE, "umeyama_scenes.npz")
np.savez_compressed(out, **arrays)
print(out, os.path.getsize(out), "bytes")
