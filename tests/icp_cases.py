"""Edge cases of the ICP refinement kernel (test infrastructure: pinned on the CPU by
tests/test_solver_cases_host.py, run on the GPU by tests/test_gpu_icp_edges.py).

One row of ICP_EDGE_CASES is one launch of krrn_icp_refine_f32 at B = 1 (BATCH is one launch of six). The rows sit
where csrc/icp.hip takes another path: every case of the switch over slots = cdiv(N, 512) and both sides of every
slot boundary, the remainder of the model loop's unroll by 4, every stop (STARVED in pass 0 and after an update,
CONVERGED by tolerance and by fixed point, MAX_ITER, DEGENERATE in pass 0 three ways and after an update) and
non-finite points on either side. Scenes are icp_ref.make_scene's with M = 67 and max_dist 0.02 unless the row
says otherwise.

Seeds are part of the table: test_solver_cases_host.py asserts with the numpy restatement alone that each row shows
what `expect` names and meets icp_ref.check_conditions."""
import functools
from collections import namedtuple

import numpy as np

import icp_ref as ir

Case = namedtuple("Case", "id N M seed gen edit max_dist kw expect")


def _case(id, N, M=67, seed=None, gen=None, edit=None, max_dist=ir.MAX_DIST, kw=None, **expect):
    return Case(id, N, M, 7000 + N if seed is None else seed, gen or {}, edit, max_dist, kw or {}, expect)


STARVED_SCENE = dict(seed=5080, gen=dict(out_frac=0.3, rot_deg=12.0, dt=0.01), max_dist=0.01)
CLOUD_NAN, CLOUD_INF, CLOUD_NINF = 5, 100, 200   # cloud points the `cloud_nonfinite` edit spoils
CLUSTER_A, CLUSTER_B = 4, 60                      # the `cluster` edit: spread cloud points, identical cloud points
MODEL_NAN = 10                                    # model point the `model_nan` edit spoils

ICP_EDGE_CASES = [
    # every case of the slot switch and both sides of every boundary (seeds 7000 + N)
    _case("n3", 3, kw=dict(min_pairs=3)),
    _case("n511", 511), _case("n512", 512), _case("n513", 513), _case("n1024", 1024), _case("n1025", 1025),
    _case("n1537", 1537), _case("n2049", 2049), _case("n2561", 2561), _case("n3073", 3073), _case("n3585", 3585),
    _case("n4096", 4096),
    # the model loop's unroll-by-4 remainder; the cloud is drawn from the whole model. One model point has no
    # second direction (DEGENERATE); two span a line only (a rank-1 covariance up to rounding, which no
    # restatement can follow), so that row scores the start pose alone
    _case("m1_degenerate", 64, 1, seed=7101, gen=dict(half=False), status=ir.DEGENERATE, passes=1),
    _case("m2_score_only", 64, 2, seed=7102, gen=dict(half=False), kw=dict(max_iter=0), status=ir.MAX_ITER_HIT, passes=1),
    _case("m3", 64, 3, seed=7103, gen=dict(half=False, rot_deg=2.0, dt=0.002), status=ir.CONVERGED, pairs=64),
    _case("m4", 64, 4, seed=7104, gen=dict(half=False, rot_deg=2.0, dt=0.002), status=ir.CONVERGED, pairs=64),
    _case("m5", 64, 5, seed=7105, gen=dict(half=False, rot_deg=2.0, dt=0.002), status=ir.CONVERGED, pairs=64),
    # stops
    _case("starved_after_update", 257, 65, kw=dict(min_pairs=52), status=ir.STARVED, passes=2, pairs=50, **STARVED_SCENE),
    # K = 52, 50, 48 in passes 0, 1, 2: min_pairs 51 still starves in pass 1, min_pairs 50 is the first that goes
    # on from there (the test is K < min_pairs) and starves one pass later
    _case("min_pairs_51", 257, 65, kw=dict(min_pairs=51), status=ir.STARVED, passes=2, pairs=50, **STARVED_SCENE),
    _case("min_pairs_50_continues", 257, 65, kw=dict(min_pairs=50), status=ir.STARVED, passes=3, pairs=48, **STARVED_SCENE),
    _case("max_iter_1", 257, 65, seed=7201, kw=dict(max_iter=1), status=ir.MAX_ITER_HIT, passes=2),
    _case("max_iter_2_n4096_m4096", 4096, 4096, seed=7202, kw=dict(max_iter=2), status=ir.MAX_ITER_HIT, passes=3),
    _case("tol0_fixed_point", 257, 65, seed=7203, kw=dict(max_iter=64, tol=0.0), status=ir.CONVERGED),
    _case("degenerate_identical_cloud", 130, seed=7301, gen=dict(noise=0.0, rot_deg=1.0, dt=0.001), edit="identical_cloud",
          status=ir.DEGENERATE, passes=1),
    _case("degenerate_x_axis", 100, 33, seed=7302, edit="x_axis", status=ir.DEGENERATE, passes=1),
    # DEGENERATE after an update: the pose handed back is the one from before the failed update, not the input
    _case("degenerate_after_update", CLUSTER_A + CLUSTER_B, 12, seed=7611, edit="cluster", status=ir.DEGENERATE, passes=2,
          pairs=CLUSTER_B),
    # inputs
    _case("cloud_nan_inf", 257, 65, seed=7401, edit="cloud_nonfinite"),
    _case("model_nan", 257, 65, seed=7402, edit="model_nan"),
    _case("max_dist_inf", 300, 65, seed=7403, gen=dict(out_frac=0.2), max_dist=np.inf, pairs=300),
    _case("max_dist_0", 257, 65, seed=7404, max_dist=0.0, status=ir.STARVED, passes=1, pairs=0),
]
CASES = {c.id: c for c in ICP_EDGE_CASES}
assert len(CASES) == len(ICP_EDGE_CASES)
SLOT_ROWS = [c.id for c in ICP_EDGE_CASES[:12]]
NULL_NN = "n513"  # the two-slot row that is also launched without nn_idx

# one launch, six crops of N = 257 / M = 65 with their own max_dist: (seed, generator arguments, edit, max_dist)
BATCH_KW = dict(max_iter=6)
BATCH = [
    (7501, dict(noise=0.0, rot_deg=1.0, dt=0.001), None, 0.02),       # CONVERGED
    (7502, dict(out_frac=0.2), None, 0.02),                           # MAX_ITER
    (7503, dict(shift=1.0), None, 0.02),                              # STARVED in pass 0
    (7504, dict(noise=0.0, rot_deg=1.0, dt=0.001), "identical_cloud", 0.02),   # DEGENERATE
    (7505, dict(rot_deg=2.0), None, 0.012),
    (5080, STARVED_SCENE["gen"], None, 0.01),
]


def _edit(sc, edit, seed):
    cloud, model = sc["cloud"].copy(), sc["model"].copy()
    if edit == "identical_cloud":
        cloud[:] = cloud[0]
    elif edit == "cloud_nonfinite":
        cloud[CLOUD_NAN, 1] = np.nan
        cloud[CLOUD_INF, 0] = np.inf
        cloud[CLOUD_NINF, 2] = -np.inf
    elif edit == "model_nan":
        model[MODEL_NAN, 0] = np.nan
    elif edit == "x_axis":
        # model and cloud on the x axis, the pose a shift along it: every covariance entry but [0][0] is an exact 0
        rng = np.random.default_rng(int(sc["t0"].view(np.uint32)[0]))
        N, M = cloud.shape[0], model.shape[0]
        model = np.zeros((M, 3), np.float32)
        model[:, 0] = np.linspace(-0.06, 0.06, M, dtype=np.float32)
        cloud = np.zeros((N, 3), np.float32)
        cloud[:, 0] = model[rng.integers(M, size=N), 0].astype(np.float64) + 0.05 + rng.normal(scale=2e-4, size=N)
        sc["R0"] = np.eye(3, dtype=np.float32)
        sc["t0"] = np.array([0.0505, 0.0, 0.0], np.float32)
    elif edit == "cluster":
        # CLUSTER_B identical cloud points half of max_dist from model point 0 along d, CLUSTER_A points just inside
        # max_dist of model points 1.. on the other side: the first update follows the cluster, the spread points fall
        # out of reach, and the pairs that are left (one cloud point, one model point) have a covariance of exact zeros
        rng = np.random.default_rng(seed + 1)
        Mo, R0, t0 = model.astype(np.float64), sc["R0"].astype(np.float64), sc["t0"].astype(np.float64)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        q = np.concatenate([Mo[1:1 + CLUSTER_A] - 0.99 * ir.MAX_DIST * d,
                            np.repeat(Mo[:1] + 0.5 * ir.MAX_DIST * d, CLUSTER_B, 0)])
        cloud = (q @ R0.T + t0).astype(np.float32)
        cloud[CLUSTER_A:] = cloud[CLUSTER_A]
    else:
        assert edit is None, edit
    sc["cloud"], sc["model"] = cloud, model
    return sc


def _scene(seed, N, M, gen, edit):
    sc = _edit(ir.make_scene(seed, N, M, **gen), edit, seed)
    for v in sc.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sc


@functools.lru_cache(maxsize=None)
def build(case_id):
    """The row's scene (read-only: shared between tests): R0, t0, cloud, model f32, and the row's own max_dist / kw."""
    c = CASES[case_id]
    sc = _scene(c.seed, c.N, c.M, c.gen, c.edit)
    sc["max_dist"], sc["kw"] = c.max_dist, dict(c.kw)
    return sc


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """icp_ref.icp of the row, computed once per process (callers do not modify it)."""
    sc = build(case_id)
    return ir.icp(sc["R0"], sc["t0"], sc["cloud"], sc["model"], sc["max_dist"], **sc["kw"])


@functools.lru_cache(maxsize=None)
def batch():
    """(scenes, max_dist f32 [6], references) of BATCH."""
    scs = [_scene(seed, 257, 65, gen, edit) for seed, gen, edit, _ in BATCH]
    md = np.array([m for *_, m in BATCH], np.float32)
    refs = [ir.icp(s["R0"], s["t0"], s["cloud"], s["model"], m, **BATCH_KW) for s, m in zip(scs, md)]
    return scs, md, refs
