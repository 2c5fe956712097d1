"""Edge cases of the PnP-RANSAC kernels (test infrastructure: pinned on the CPU by
tests/test_pnp_cases_host.py, run on the GPU by tests/test_gpu_pnp_edges.py).

One row of PNP_EDGE_CASES is one launch of krrn_pnp_ransac_f32. The rows sit at the sizes where
csrc/pnp.hip takes another path: P around the 16-lane scoring stride and the 64-lane inlier ballot,
P = 5 and P = 1024 (kPnpMaxP), H with a ragged last block of four hypotheses, H across the 64-count
chunks of the selection scan, H = 4095; at the selection's own edges (ties, a best count of exactly 5,
a maximum of exactly 4, conf 0 and 1, thr other than 1); and at inputs that take EPnP's rank-deficient
branches (collinear / coplanar / repeated subsets, NaN / Inf correspondences). Every crop has its own
K4, extent and lfborder, a non-square map, N > P chosen pixels and a non-identity `sel`, so an index
taken from the wrong crop or the wrong table cannot go unnoticed.

Seeds are part of the table: test_pnp_cases_host.py asserts with the C oracle alone that each row
shows the condition its id names."""
import functools
from collections import namedtuple

import numpy as np

from oracle import pnp as opnp

K4_LINEMOD = np.array([572.4114, 573.57043, 325.2611, 242.04899], np.float64)
FRAME_WH = (640.0, 480.0)
# (extent, lfborder) in metres of LineMOD objects 1, 6 and 11: size / min of configs/models_info.yaml
OBJECTS = [
    (np.array([0.0758686, 0.0775992, 0.091769]), np.array([-0.0379343, -0.0387996, -0.0458845])),
    (np.array([0.0670107, 0.127633, 0.1174566]), np.array([-0.0335054, -0.0638165, -0.0587283])),
    (np.array([0.0367211, 0.077866, 0.1728158]), np.array([-0.0183605, -0.038933, -0.0864079])),
]
MAP_FILL = 9.0  # value of every map pixel that is not chosen (a normalised coordinate lies in [0, 1])
PIX_FILL = -1000.0  # x / y of every chosen pixel that `sel` leaves out

Case = namedtuple("Case", "id B P H N kinds subsets thr conf seed")

CLEAN = ("clean",)
PLANAR = ("planar",)
PURE_NOISE = ("pure_noise",)
NONFINITE = ("nonfinite",)
DEGENERATE = ("degenerate",)


def noisy(outlier_frac, noise_px):
    return ("noisy", outlier_frac, noise_px)


def _case(id, B, P, H, kinds, seed, N=None, subsets="random", thr=1.0, conf=0.9999):
    assert len(kinds) == B
    return Case(id, B, P, H, P + 13 if N is None else N, tuple(kinds), subsets, thr, conf, seed)


# the sel-space positions the `degenerate` kind fills, and the explicit subsets over them (sound subsets
# between the degenerate ones)
DEG_COLLINEAR = [0, 1, 2, 3, 4]
DEG_COPLANAR = [5, 6, 7, 8, 9]
DEG_COINCIDENT = [10, 11]
DEG_NAN = [12, 13]
DEG_INF = [14]
DEG_SUBSETS = [
    [20, 31, 42, 53, 64],
    DEG_COLLINEAR,
    [7, 7, 7, 7, 7],
    [21, 32, 43, 54, 65],
    DEG_COPLANAR,
    [10, 11, 10, 11, 10],
    [12, 22, 33, 44, 55],   # holds a NaN point
    [23, 14, 34, 45, 56],   # holds the Inf pixel
    [24, 35, 46, 57, 68],
    [76, 75, 74, 73, 72],
    [25, 25, 36, 47, 58],   # one repeated index among sound points
]
DEG_UNSOUND = [2, 5, 6, 7, 10]  # rows of DEG_SUBSETS that must score < 5 (repeated index, NaN, Inf)

MIXED = "mixed_b5_p100_h37"
NULL_MASK = "p65_h2"

PNP_EDGE_CASES = [
    # minimal P: the subset is all the points, the refit runs on exactly 5 inliers
    _case("p5_h1_clean", 2, 5, 1, [CLEAN, CLEAN], 1),
    _case("p5_h3_clean", 2, 5, 3, [CLEAN, CLEAN], 2),
    # tails of the 16-lane scoring loop and of the 64-lane ballot, H mod 4 = 1, 2, 3 and H = 1
    _case("p6_h2", 2, 6, 2, [noisy(0.0, 0.3), CLEAN], 3),
    _case("p15_h3", 2, 15, 3, [noisy(0.1, 0.1), noisy(0.0, 0.2)], 4),
    _case("p16_h5", 2, 16, 5, [noisy(0.1, 0.3), CLEAN], 5),
    _case("p17_h63", 2, 17, 63, [noisy(0.2, 0.3), noisy(0.3, 0.1)], 6),
    _case("p63_h65", 2, 63, 65, [noisy(0.3, 0.4), noisy(0.1, 0.2)], 7),
    _case("p64_h1", 2, 64, 1, [noisy(0.1, 0.1), CLEAN], 8),
    _case("p65_h2", 2, 65, 2, [noisy(0.0, 0.4), CLEAN], 9),
    _case("p129_h5", 2, 129, 5, [noisy(0.1, 0.4), CLEAN], 10),
    # maximal P (the refine kernel's LDS extents); the first is also the cut-off row of condition (a)
    _case("p1000_h101_cutoff", 1, 1000, 101, [noisy(0.3, 0.4)], 105),
    _case("p1024_h65_full_sel", 1, 1024, 65, [noisy(0.3, 0.4)], 12, N=1024),
    # the selection scan across its 64-count chunks (condition (b))
    _case("scan_h129_stop_in_chunk1", 1, 100, 129, [noisy(0.42, 0.4)], 103),
    _case("scan_h130_best_in_chunk1", 1, 150, 130, [noisy(0.6, 0.3)], 100),
    _case("scan_h258_best_past_192", 1, 333, 258, [noisy(0.68, 0.3)], 102),
    _case("scan_h65_tail_count", 2, 40, 65, [noisy(0.6, 0.3), noisy(0.5, 0.3)], 16),
    # maximal H
    _case("h4095_p64", 1, 64, 4095, [noisy(0.7, 0.2)], 101),
    # ties at the best count: the first must win
    _case("tie_p6_h9", 1, 6, 9, [noisy(0.0, 0.3)], 18),
    _case("tie_p16_h63", 1, 16, 63, [noisy(0.3, 0.2)], 19),
    # the selection threshold cnt > max(best, 4)
    _case("max_count_exactly_4", 1, 12, 7, [noisy(0.75, 0.0)], 981),
    _case("max_count_exactly_5", 1, 8, 20, [noisy(0.4, 0.0)], 112),
    # every point an inlier, P not a multiple of 64
    _case("all_inliers_p65", 1, 65, 3, [CLEAN], 22),
    _case("all_inliers_p129", 1, 129, 6, [CLEAN], 23),
    # planar object at a ragged P (pinv3 drops a singular value in every solve)
    _case("planar_p77_h10", 2, 77, 10, [PLANAR, PLANAR], 24),
    # rank-deficient and non-finite subsets, given explicitly
    _case("degenerate_p77", 1, 77, len(DEG_SUBSETS), [DEGENERATE], 25, subsets="degenerate"),
    # conf and thr
    _case("conf0_p200_h50", 1, 200, 50, [noisy(0.3, 0.4)], 26, conf=0.0),
    _case("conf05_p200_h50", 1, 200, 50, [noisy(0.3, 0.4)], 26, conf=0.5),
    _case("conf1_p200_h50", 1, 200, 50, [noisy(0.3, 0.4)], 26, conf=1.0),
    _case("thr025_p200_h50", 1, 200, 50, [noisy(0.3, 0.4)], 27, thr=0.25),
    _case("thr3_p200_h50", 1, 200, 50, [noisy(0.3, 0.4)], 27, thr=3.0),
    # per-crop parameters: five kinds, five K4 / extent / lfborder, one launch
    _case(MIXED, 5, 100, 37, [CLEAN, noisy(0.5, 0.5), PLANAR, PURE_NOISE, NONFINITE], 101),
]
CASES = {c.id: c for c in PNP_EDGE_CASES}
assert len(CASES) == len(PNP_EDGE_CASES)


def map_shape(N):
    """(Hm, Wm), Hm != Wm, Hm * Wm >= N."""
    Wm = int(np.sqrt(N)) + 3
    Hm = -(-N // Wm) + 1
    return (Hm + 1 if Hm == Wm else Hm), Wm


def make_crop(spec, seed):
    """One crop's host arrays. spec = (kind tuple, P, N); the random stream is `seed` alone.

    Returns a dict: xyz f32 [3, Hm, Wm], choose i64 [N], x_map / y_map f32 [N], sel i32 [P], K4 f32 [4],
    extent / lfborder f64 [3], R_gt / t_gt, and `nonfinite`: the sel-space positions of the NaN / Inf points."""
    kind, P, N = spec
    name = kind[0]
    rng = np.random.default_rng(seed)
    Hm, Wm = map_shape(N)
    HW = Hm * Wm
    ext, lfb = OBJECTS[seed % len(OBJECTS)]  # consecutive crops of a row: different objects
    K4 = K4_LINEMOD * (1.0 + rng.uniform(-0.1, 0.1, 4))
    R = opnp.rotation_from_axis_angle(rng.normal(size=3))
    t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.1)])
    # chosen pixels: distinct, the first and the last pixel of the map among them
    choose = np.concatenate([[0, HW - 1], 1 + rng.choice(HW - 2, N - 2, replace=False)])
    rng.shuffle(choose)
    # sel: a non-identity draw from N that keeps the choose slots of pixel 0 and pixel HW - 1
    while True:
        sel = rng.permutation(N)[:P]
        if not np.array_equal(sel, np.arange(P)):
            break
    ends = [int(np.nonzero(choose == pix)[0][0]) for pix in (0, HW - 1)]
    for slot in ends:
        if slot not in sel:
            sel[[i for i in range(P) if sel[i] not in ends][1]] = slot
    assert len(set(sel.tolist())) == P
    u = rng.random((N, 3))
    if name == "planar":
        u[:, 2] = 0.5
    if name == "degenerate":
        s = sel
        steps = np.array([[0.0], [0.25], [0.5], [0.75], [1.0]])
        u[s[DEG_COLLINEAR]] = np.array([0.125, 0.25, 0.5]) + steps * [0.5, 0.25, 0.125]
        u[s[DEG_COPLANAR], 2] = 0.3
        u[s[DEG_COINCIDENT[1]]] = u[s[DEG_COINCIDENT[0]]]
    u32 = u.astype(np.float32)  # the normalised coordinate the network would predict
    pw = u32.astype(np.float64) * ext + lfb
    pc = pw @ R.T + t
    img = np.stack([K4[0] * pc[:, 0] / pc[:, 2] + K4[2], K4[1] * pc[:, 1] / pc[:, 2] + K4[3]], 1)
    nonfinite = {"nan": [], "inf": []}
    if name == "noisy":
        _, outlier_frac, noise_px = kind
        if noise_px:
            img += rng.normal(scale=noise_px, size=img.shape)
        out = rng.random(N) < outlier_frac
        img[out] += rng.uniform(-20, 20, size=(int(out.sum()), 2))
    elif name == "pure_noise":
        img = rng.random((N, 2)) * FRAME_WH
    elif name in ("nonfinite", "degenerate"):
        img += rng.normal(scale=0.2, size=img.shape)
        if name == "degenerate":
            img[sel[DEG_COINCIDENT[1]]] = img[sel[DEG_COINCIDENT[0]]]
            nonfinite = {"nan": list(DEG_NAN), "inf": list(DEG_INF)}
        else:
            out = rng.random(N) < 0.2
            img[out] += rng.uniform(-20, 20, size=(int(out.sum()), 2))
            nonfinite = {"nan": [P // 3, P // 2], "inf": [(2 * P) // 3]}
    else:
        assert name in ("clean", "planar"), name
    xyz = np.full((3, HW), MAP_FILL, np.float32)
    xyz[:, choose] = u32.T
    x_map = np.full(N, PIX_FILL, np.float32)
    y_map = np.full(N, PIX_FILL, np.float32)
    x_map[sel] = img[sel, 0]
    y_map[sel] = img[sel, 1]
    xyz[0, choose[sel[nonfinite["nan"][:1]]]] = np.nan
    xyz[2, choose[sel[nonfinite["nan"][1:]]]] = np.nan
    x_map[sel[nonfinite["inf"]]] = np.inf
    return dict(xyz=xyz.reshape(3, Hm, Wm), choose=choose.astype(np.int64), x_map=x_map, y_map=y_map,
                sel=sel.astype(np.int32), K4=K4.astype(np.float32), extent=ext.copy(), lfborder=lfb.copy(),
                R_gt=R, t_gt=t, nonfinite=nonfinite, kind=kind)


def correspondences(crop):
    """(obj f32 [P, 3], img f32 [P, 2]) as the kernel forms them (csrc/pnp.hip load_corr): the f64 product
    xyz * extent + lfborder rounded to f32, the pixels of the selected slots."""
    s = crop["sel"].astype(np.int64)
    pix = crop["choose"][s]
    flat = crop["xyz"].reshape(3, -1)
    with np.errstate(invalid="ignore"):
        obj = (flat[:, pix].astype(np.float64).T * crop["extent"] + crop["lfborder"]).astype(np.float32)
    return obj, np.stack([crop["x_map"][s], crop["y_map"][s]], 1)


@functools.lru_cache(maxsize=None)
def build(case_id):
    """(crops, subsets i32 [B, H, 5]) of a row; crop b's stream is seed * 100 + b, the subsets' seed * 100 + 99."""
    c = CASES[case_id]
    crops = [make_crop((c.kinds[b], c.P, c.N), c.seed * 100 + b) for b in range(c.B)]
    if c.subsets == "degenerate":
        subsets = np.tile(np.array(DEG_SUBSETS, np.int32), (c.B, 1, 1))
    else:
        rng = np.random.default_rng(c.seed * 100 + 99)
        subsets = np.stack([np.stack([rng.permutation(c.P)[:5] for _ in range(c.H)]) for _ in range(c.B)]).astype(np.int32)
    assert subsets.shape == (c.B, c.H, 5)
    return crops, subsets


def oracle_crop(obj, img, K4, subsets, thr, conf):
    """The C oracle on one crop: every hypothesis and the RANSAC result."""
    hR, ht, hcnt = opnp.pnp_hypotheses(obj, img, K4, subsets, thr)
    R, t, cnt, mask, best_h = opnp.pnp_ransac(obj, img, K4, subsets, thr, conf)
    return dict(hyp_R=hR, hyp_t=ht, hyp_cnt=hcnt, R=R, t=t, cnt=cnt, mask=mask, best_h=best_h)


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """oracle_crop of every crop of a row (computed once per process; callers do not modify it)."""
    c = CASES[case_id]
    crops, subsets = build(case_id)
    return [oracle_crop(*correspondences(crops[b]), crops[b]["K4"], subsets[b], c.thr, c.conf) for b in range(c.B)]


def update_niters(conf, ep, model_points, max_iters):
    """cv::RANSACUpdateNumIters (ptsetreg.cpp)."""
    conf, ep = min(max(conf, 0.0), 1.0), min(max(ep, 0.0), 1.0)
    num = max(1.0 - conf, np.finfo(np.float64).tiny)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < np.finfo(np.float64).tiny:
        return 0
    num, denom = np.log(num), np.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else int(np.rint(num / denom))


def cv2_scan(cnts, P, conf=np.float32(0.9999)):
    """ptsetreg.cpp's RANSAC loop over already-scored hypotheses: (selected index, final niters)."""
    best, best_cnt, niters, h = -1, 0, len(cnts), 0
    while h < niters:
        c = int(cnts[h])
        if c > max(best_cnt, 4):
            best, best_cnt = h, c
            niters = update_niters(float(conf), (P - c) / P, 5, niters)
        h += 1
    return best, niters


def cv2_select(cnts, P, conf=np.float32(0.9999)):
    """The selected index of cv2_scan."""
    return cv2_scan(cnts, P, conf)[0]
