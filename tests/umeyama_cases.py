"""Edge cases of the Umeyama-RANSAC kernels and of krrn_model_points_f32 (test infrastructure: pinned on the CPU
by tests/test_solver_cases_host.py, run on the GPU by tests/test_gpu_umeyama_edges.py).

One row of UMEYAMA_EDGE_CASES is one launch of krrn_umeyama_ransac_f32. The rows sit where csrc/umeyama.hip takes
another path: N around the 64-lane scoring stride and the 256-thread staging loop, H around the 16 hypotheses of a
wave and the 64 of a block, N = 4096 / H = 8192 (128 KiB of dynamic LDS in the refit kernel); at the selection's own
edges (conf 0 / 0.5 / 0.99 / 1, a better hypothesis after the stop, a tie, the stop at i = 63 / 64 / 65, min_ratio
equal to the best ratio and one ulp above, every count 0, inlier_frac other than 0.1); and at inputs that leave the
sound path (indices outside [0, N), repeated indices, NaN / Inf points, a planar object). Scenes are LineMOD-sized
(`synth`) with 30 % outliers and 1 mm noise unless the row says otherwise.

Seeds are part of the table: test_solver_cases_host.py asserts with the numpy restatement alone that each row shows
the condition its id names and meets umeyama_ref.check_conditions."""
import functools
from collections import namedtuple

import numpy as np

import umeyama_ref as ur

EXT = np.array([0.067, 0.1276, 0.1175])
LFB = np.array([-0.0335, -0.0638, -0.0587])
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
FAR = np.array([3.0, -2.0, 5.0], np.float32)  # where the host test puts a non-finite dst point to make it an outlier

# id, N, H, builder name and its arguments, the launch's inlier_frac / conf / min_ratio, the rows of `subsets`
# named as ill-conditioned (at most two in the whole table), allow: hypotheses without a scale are expected
Case = namedtuple("Case", "id N H builder args inlier_frac conf min_ratio ill allow")


def _case(id, N, H, builder="plain", args=None, inlier_frac=ur.INLIER_FRAC, conf=ur.CONFIDENCE, min_ratio=ur.MIN_RATIO,
          ill=(), allow=False):
    return Case(id, N, H, builder, args or {}, inlier_frac, conf, min_ratio, tuple(ill), allow)


def _rodrigues(v):
    th = np.linalg.norm(v)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def synth(seed, N, out_frac=0.3, noise=1e-3, planar=False):
    """LineMOD-sized model points under a random pose at about 0.9 m -> (src f32, dst f32, outlier mask)."""
    rng = np.random.default_rng(seed)
    u = rng.random((N, 3)).astype(np.float32)
    if planar:
        u[:, 2] = np.float32(0.5)
    src = (u.astype(np.float64) * EXT + LFB).astype(np.float32)
    R = _rodrigues(rng.normal(size=3))
    t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.1)])
    dst = src.astype(np.float64) @ R.T + t
    if noise:
        dst += rng.normal(scale=noise, size=dst.shape)
    out = rng.random(N) < out_frac
    dst[out] = t + rng.uniform(-0.15, 0.15, size=(int(out.sum()), 3))
    return src, dst.astype(np.float32), out


def draw_subsets(rng, pool, H):
    """H rows of five distinct indices out of `pool`."""
    pool = np.asarray(pool)
    sub = pool[rng.integers(len(pool), size=(H, 5))]
    while True:
        bad = np.array([len(set(r)) < 5 for r in sub.tolist()])
        if not bad.any():
            return sub.astype(np.int32)
        sub[bad] = pool[rng.integers(len(pool), size=(int(bad.sum()), 5))]


SEL_N, SEL_H, SEL_LATE = 200, 130, 100  # the selection scene; SEL_LATE: where its best hypothesis sits
SEL_SEED = 8100


@functools.lru_cache(maxsize=None)
def _selection_scene():
    """N = 200 with 4 mm noise (so that sound samples spread over many counts) and H = 130 rows arranged from a
    seeded pool by their counts: rows 0 and 1 poor (0 < count < 0.1 N), the single best row of the pool at SEL_LATE,
    and before it only rows of at most 0.95 of its count, one of at least half of it among the first eight."""
    src, dst, out = synth(SEL_SEED, SEL_N, noise=4e-3)
    rng = np.random.default_rng(SEL_SEED)
    pool = np.concatenate([draw_subsets(rng, np.arange(SEL_N), 600), draw_subsets(rng, np.nonzero(~out)[0], 600)])
    cnt = ur.ransac(src, dst, pool, conf=1.0)["counts"]
    order = np.argsort(-cnt, kind="stable")
    best = order[0]
    poor = [i for i in range(len(pool)) if 0 < cnt[i] < 0.1 * SEL_N][:2]
    mid = [i for i in range(len(pool)) if 0.1 * SEL_N <= cnt[i] <= 0.95 * cnt[best]]
    lead = [i for i in mid if cnt[i] >= 0.5 * cnt[best]][0]
    rest = [i for i in mid if i != lead]
    rows = poor + rest[:4] + [lead] + rest[4:SEL_LATE - 3] + [best] + rest[SEL_LATE - 3:SEL_H - 4]
    assert len(rows) == SEL_H and rows[SEL_LATE] == best and len(set(rows)) == SEL_H
    return src, dst, pool[rows]


def _b_plain(c, seed, out_frac=0.3, noise=1e-3, planar=False, pool="all", best_at=None):
    src, dst, out = synth(seed, c.N, out_frac, noise, planar)
    rng = np.random.default_rng(seed + 1)
    sub = np.arange(5, dtype=np.int32)[None] if c.N == 5 else \
        draw_subsets(rng, np.arange(c.N) if pool == "all" else np.nonzero(~out)[0], c.H)
    if best_at is not None:  # one row of the largest count goes to row best_at, the others that reach it are replaced
        cnt = ur.ransac(src, dst, sub, c.inlier_frac, 1.0)["counts"]
        top = np.nonzero(cnt == cnt.max())[0]
        sub[top[1:]] = sub[int(np.argmin(cnt))]
        sub[[top[0], best_at]] = sub[[best_at, top[0]]]
    return dict(src=src[None], dst=dst[None], subsets=sub[None])


def _b_selection(c, tie=None):
    src, dst, sub = _selection_scene()
    sub = sub.copy()
    if tie is not None:  # the best row once more, earlier: two identical rows tie at the maximum
        sub[tie] = sub[SEL_LATE]
    return dict(src=src[None], dst=dst[None], subsets=sub[None])


def _b_all_identical(c, seed):
    src, dst, _ = synth(seed, c.N)
    sub = np.repeat(np.random.default_rng(seed).integers(c.N, size=(c.H, 1)), 5, axis=1).astype(np.int32)
    return dict(src=src[None], dst=dst[None], subsets=sub[None])


def _b_indices(c, seed):
    """Rows 0..3 hold one index outside [0, N) each, row 4 all four; `clamped` is what the kernel must make of them."""
    d = _b_plain(c, seed)
    sub = d["subsets"].astype(np.int64)
    for r, v in enumerate((-1, c.N, INT_MAX, INT_MIN)):
        sub[0, r, r] = v
    sub[0, 4, :4] = (-1, c.N, INT_MAX, INT_MIN)
    d["subsets"] = sub.astype(np.int32)
    d["clamped"] = np.clip(sub, 0, c.N - 1).astype(np.int32)
    return d


def _b_repeats(c, seed, rows):
    """`rows`: {row: five indices into the row's own first two samples} (repeated indices)."""
    d = _b_plain(c, seed)
    for r, pat in rows.items():
        d["subsets"][0, r] = d["subsets"][0, r][list(pat)]
    return d


NONFINITE_POINT = 17   # the point the src_nan / dst_nan_inf builders spoil
DST_ROWS_HOLDING = (0, 5, 16, 40)  # rows of dst_nan_inf made to sample the spoiled point


def _b_src_nan(c, seed):
    d = _b_plain(c, seed)
    d["src"][0, NONFINITE_POINT, 1] = np.nan
    return d


def _b_dst_nan_inf(c, seed):
    d = _b_plain(c, seed)
    d["dst"][0, NONFINITE_POINT] = (np.nan, np.inf, 0.9)
    sub = d["subsets"][0]
    for r in range(c.H):  # only DST_ROWS_HOLDING sample the point
        sub[r][sub[r] == NONFINITE_POINT] = (NONFINITE_POINT + 1 + r) % c.N
    for r in DST_ROWS_HOLDING:
        sub[r, r % 5] = NONFINITE_POINT
    assert all(len(set(r)) == 5 for r in sub.tolist())
    return d


def _b_batch_nan_middle(c, seed):
    a, b, e = _b_plain(c, seed), _b_src_nan(c, seed + 10), _b_plain(c, seed + 20, planar=True)
    return {k: np.concatenate([a[k], b[k], e[k]]) for k in ("src", "dst", "subsets")}


BUILDERS = dict(plain=_b_plain, selection=_b_selection, all_identical=_b_all_identical, indices=_b_indices,
                repeats=_b_repeats, src_nan=_b_src_nan, dst_nan_inf=_b_dst_nan_inf, batch_nan_middle=_b_batch_nan_middle)

SIZES = [(5, 1), (63, 15), (64, 16), (65, 17), (255, 63), (256, 64), (257, 65), (1000, 130)]
BIG, BIG_BEST = "n4096_h8192_conf1", 8100
OPTIONAL = "n257_h65"     # the row also launched without best_hyp, without inlier_mask and without both
INDICES = "indices_outside_0_n"
BATCH = "batch_nan_crop_in_the_middle"
ILL = "ill_two_distinct_points"
STOPS = (63, 64, 65)

UMEYAMA_EDGE_CASES = [
    _case("n5_h1", 5, 1, args=dict(seed=8005, out_frac=0.0))] + [
    _case(f"n{N}_h{H}", N, H, args=dict(seed=8000 + N)) for N, H in SIZES[1:]] + [
    # conf = 1: the scan reads all 8192 counts; the samples are drawn from the inliers, the best one is put near the end
    _case(BIG, 4096, 8192, args=dict(seed=8096, pool="inliers", best_at=BIG_BEST), conf=1.0),
    # the selection loop on one scene (conf and min_ratio tuned rows get their value from `tuned`)
    _case("sel_conf0_stops_at_1_and_fails", SEL_N, SEL_H, "selection", conf=0.0),
    _case("sel_conf05", SEL_N, SEL_H, "selection", conf=0.5),
    _case("sel_conf099_better_after_stop", SEL_N, SEL_H, "selection", conf=0.99),
    _case("sel_conf1_finds_the_late_best", SEL_N, SEL_H, "selection", conf=1.0),
    _case("sel_tie_lower_index_wins", SEL_N, SEL_H, "selection", dict(tie=40), conf=1.0),
    _case("stop_at_63", SEL_N, SEL_H, "selection", conf="stop:63"),
    _case("stop_at_64", SEL_N, SEL_H, "selection", conf="stop:64"),
    _case("stop_at_65", SEL_N, SEL_H, "selection", conf="stop:65"),
    _case("min_ratio_equal_best", 257, 65, args=dict(seed=8257), min_ratio="best"),
    _case("min_ratio_next_above_best", 257, 65, args=dict(seed=8257), min_ratio="best+ulp"),
    _case("min_ratio_0_all_counts_0", 100, 20, "all_identical", dict(seed=8300), min_ratio=0.0, allow=True),
    _case("inlier_frac_005", 257, 65, args=dict(seed=8257), inlier_frac=0.05),
    _case("inlier_frac_03", 257, 65, args=dict(seed=8257), inlier_frac=0.3),
    # inputs
    _case(INDICES, 300, 33, "indices", dict(seed=8400)),
    _case("five_identical_indices", 257, 17, "repeats", dict(seed=8401, rows={3: (0, 0, 0, 0, 0)}), allow=True),
    _case("src_nan_fails", 257, 65, "src_nan", dict(seed=8402), allow=True),
    _case("dst_nan_inf_point", 257, 65, "dst_nan_inf", dict(seed=8403), allow=True),
    _case("planar_object", 257, 65, args=dict(seed=8404, planar=True)),
    _case(BATCH, 257, 65, "batch_nan_middle", dict(seed=8405), allow=True),
    # the two ill-conditioned rows of the table: samples of two distinct points (a rank-1 covariance up to rounding)
    _case(ILL, 257, 33, "repeats", dict(seed=8406, rows={2: (0, 1, 0, 1, 0), 20: (2, 2, 2, 3, 3)}), ill=(2, 20)),
]
CASES = {c.id: c for c in UMEYAMA_EDGE_CASES}
assert len(CASES) == len(UMEYAMA_EDGE_CASES)
assert sum(len(c.ill) for c in UMEYAMA_EDGE_CASES) <= 2


@functools.lru_cache(maxsize=None)
def build(case_id):
    """The row's arrays (shared between tests: callers do not modify them): src / dst f32 [B, N, 3], subsets i32
    [B, H, 5] (`clamped` beside it where the row passes indices outside [0, N)) and the launch's inlier_frac, conf,
    min_ratio as f64 values."""
    c = CASES[case_id]
    d = BUILDERS[c.builder](c, **c.args)
    assert d["src"].shape[1:] == (c.N, 3) and d["subsets"].shape[1:] == (c.H, 5)
    conf, min_ratio = c.conf, c.min_ratio
    if isinstance(conf, str) or isinstance(min_ratio, str):
        base = ur.ransac(d["src"][0], d["dst"][0], d["subsets"][0], c.inlier_frac, 1.0, 0.0)
        if isinstance(conf, str):  # half way between the stop expression at i - 1 and at i
            i = int(conf.split(":")[1])
            run = np.maximum.accumulate(base["counts"]) / c.N
            e = [1 - (1 - run[k] ** 5) ** k for k in (i - 1, i)]
            conf = 0.5 * (e[0] + e[1])
        if isinstance(min_ratio, str):
            ratio = base["inliers"] / c.N
            min_ratio = ratio if min_ratio == "best" else np.nextafter(ratio, 2.0)
    d.update(inlier_frac=float(c.inlier_frac), conf=float(conf), min_ratio=float(min_ratio))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """umeyama_ref.ransac of every crop of a row on the clamped subsets (computed once per process; the per-hypothesis
    masks are dropped)."""
    c, d = CASES[case_id], build(case_id)
    sub = d.get("clamped", d["subsets"])
    refs = []
    for b in range(d["src"].shape[0]):
        r = ur.ransac(d["src"][b], d["dst"][b], sub[b], d["inlier_frac"], d["conf"], d["min_ratio"], ill=c.ill)
        r.pop("masks")
        refs.append(r)
    return refs


# ---- krrn_model_points_f32 ----------------------------------------------------------------------------------------

MODEL_POINT_ROWS = [(1, 1), (3, 85), (1, 255), (2, 128), (1, 256), (1, 257)]  # (B, N): B N = 1, 255, 256, 257
MP_HW = 7 * 9


def model_points_case(B, N):
    """xyz f32 [B, 3, HW], choose i64 [B, N] (0, HW - 1, HW, -1 and 2^40 among the pixels wherever N has room),
    extent / lfborder f64 [B, 3] (each crop its own), and the expected out f32 [B, N, 3]: the f64 product rounded to
    f32, NaN exactly at the pixels outside the map."""
    rng = np.random.default_rng(8500 + 10 * B + N)
    xyz = rng.random((B, 3, MP_HW)).astype(np.float32)
    choose = rng.integers(MP_HW, size=(B, N)).astype(np.int64)
    edge = [MP_HW - 1, 0, MP_HW, -1, 2 ** 40]
    for b in range(B):
        at = rng.permutation(N)[:len(edge)]
        choose[b, at] = edge[:len(at)]
    ext = EXT * (1.0 + 0.1 * rng.random((B, 3)))
    lfb = LFB * (1.0 + 0.1 * rng.random((B, 3)))
    ok = (choose >= 0) & (choose < MP_HW)
    pix = np.where(ok, choose, 0)
    val = np.take_along_axis(xyz, np.broadcast_to(pix[:, None, :], (B, 3, N)), 2).transpose(0, 2, 1)
    out = (val.astype(np.float64) * ext[:, None, :] + lfb[:, None, :]).astype(np.float32)
    out[~ok] = np.nan
    return dict(xyz=xyz, choose=choose, extent=ext, lfborder=lfb, out=out, outside=~ok)
