"""numpy f64 restatement of lib/transform/umeyama.py's estimateSimilarityTransform with explicit
subsets (test infrastructure, like tests/parity.py), and the conditioning checks under which a
bit-different f64 evaluation (the HIP kernel's) must reach the same discrete decisions.

    res = ransac(src, dst, subsets, inlier_frac, conf, min_ratio)   # src / dst [N, 3] (f32 or f64), subsets [H, 5]
    select(counts, N, conf, min_ratio)    # the selection loop alone, on any counts
    res['counts']   [H] inlier count of every hypothesis (all H are scored, as the kernel does)
    res['best_hyp'] selected hypothesis (-1 on failure), res['inliers'] its count (0 on failure)
    res['stop']     the iteration after which the reference's loop stopped
    res['scale'], res['R'], res['t']      the refit (1, I, 0 on failure), res['failed']
    res['margins']  dict of the condition figures; check_conditions(res) asserts the limits
"""
import numpy as np

INLIER_FRAC = 0.1
CONFIDENCE = 0.99
MIN_RATIO = 0.1

# limits of the generator / test conditions
MIN_SIGMA_RATIO = 1e-3      # s2 / s1 of every sampled covariance and of the refit covariance
MIN_THR_MARGIN = 1e-7       # |residual - threshold| / threshold over every (hypothesis, point)
MIN_STOP_MARGIN = 1e-9      # |early-stop expression - confidence| at every iteration


def umeyama(S, T):
    """estimateSimilarityUmeyama (:67-98) on S, T [n, 3] f64 -> scale, R, t, singular values of Cov."""
    n = S.shape[0]
    mS, mT = S.mean(0), T.mean(0)
    Sc, Tc = S - mS, T - mT
    cov = Tc.T @ Sc / n
    U, D, Vh = np.linalg.svd(cov, full_matrices=True)
    sig = D.copy()
    if np.linalg.det(U) * np.linalg.det(Vh) < 0.0:
        D[-1] = -D[-1]
        U[:, -1] = -U[:, -1]
    R = U @ Vh
    varP = np.var(S, axis=0).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = 1 / varP * np.sum(D)
        t = mT - mS.dot(scale * R.T)
    return scale, R, t, sig


def select(counts, N, conf=CONFIDENCE, min_ratio=MIN_RATIO):
    """The reference's loop (:31-52) over already-scored hypotheses, as the kernel runs it: a strictly larger
    count becomes the best, the loop stops after iteration i once 1 - (1 - best^5)^i > conf, and the crop fails
    when no hypothesis has a positive count (the kernel's best_h >= 0, whatever min_ratio is) or best < min_ratio.
    -> dict(best_hyp (-1 on failure), inliers (0 on failure), stop, failed, stop_margin).

    stop_margin is the smallest |e - conf| over the iterations whose comparison e > conf rounding could decide.
    It leaves out exactly those decided without rounding: conf >= 1 (e <= 1 always: the loop never stops), and
    i = 0 or a best count of 0, where e = 1 - 1 is exactly 0 (never above a conf >= 0)."""
    counts = np.asarray(counts)
    H = counts.shape[0]
    best, best_cnt, best_h, stop, stop_margin = 0.0, 0, -1, H - 1, np.inf
    for i in range(H):
        if counts[i] > best_cnt:
            best_cnt, best_h = int(counts[i]), i
            best = counts[i] / N
        e = 1 - (1 - best ** 5) ** i
        if not (conf >= 1.0 or i == 0 or best_cnt == 0):
            stop_margin = min(stop_margin, abs(e - conf))
        if e > conf:
            stop = i
            break
    failed = best_h < 0 or best < min_ratio
    return dict(best_hyp=-1 if failed else int(best_h), inliers=0 if failed else best_cnt, stop=stop, failed=bool(failed),
                stop_margin=stop_margin)


def ransac(src, dst, subsets, inlier_frac=INLIER_FRAC, conf=CONFIDENCE, min_ratio=MIN_RATIO, ill=()):
    """`ill`: hypothesis rows named as ill-conditioned (a sample of rank 1 up to rounding). They are scored like
    any other, but their counts mean nothing and they are left out of the margins."""
    S = np.asarray(src, np.float64)
    T = np.asarray(dst, np.float64)
    subsets = np.asarray(subsets).reshape(-1, 5)
    N, H = S.shape[0], subsets.shape[0]
    with np.errstate(invalid="ignore"):
        inlier_t = inlier_frac * 2 * np.amax(np.linalg.norm(S - S.mean(0), axis=1))
    counts = np.zeros(H, np.int64)
    masks = np.zeros((H, N), bool)
    thr_margin, sig_ratio, all_finite = np.inf, np.inf, True
    for h in range(H):
        ids = subsets[h]
        # a non-finite coordinate in the sample (or in src at all: the threshold is NaN): no scale, count 0
        # (numpy's SVD raises on NaN; the kernel's gives a NaN scale)
        if not (np.isfinite(inlier_t) and np.isfinite(S[ids]).all() and np.isfinite(T[ids]).all()):
            all_finite = False
            continue
        with np.errstate(all="ignore"):
            s, R, t, sig = umeyama(S[ids], T[ids])
        ok = np.isfinite(s) and s > 0
        all_finite &= bool(ok)
        if not ok:
            continue
        with np.errstate(invalid="ignore"):
            res = np.linalg.norm(T - (S @ (s * R).T + t), axis=1)  # NaN / inf for a non-finite point: no inlier
            thr = s * inlier_t
            masks[h] = res < thr
        counts[h] = masks[h].sum()
        if h in ill:
            continue
        sig_ratio = min(sig_ratio, sig[1] / sig[0])
        fin = np.isfinite(res)
        if fin.any():
            thr_margin = min(thr_margin, np.abs(res[fin] - thr).min() / thr)
    sel = select(counts, N, conf, min_ratio)
    out = dict(counts=counts, stop=sel["stop"], failed=sel["failed"], inlier_t=inlier_t, masks=masks,
               margins=dict(thr=thr_margin, sigma=sig_ratio, stop=sel["stop_margin"], finite=all_finite,
                            refit_sigma=np.inf))
    if sel["failed"]:
        out.update(best_hyp=-1, inliers=0, scale=1.0, R=np.eye(3), t=np.zeros(3), mask=np.zeros(N, bool))
        return out
    m = masks[sel["best_hyp"]]
    s, R, t, sig = umeyama(S[m], T[m])
    out["margins"]["refit_sigma"] = sig[1] / sig[0]
    out.update(best_hyp=sel["best_hyp"], inliers=sel["inliers"], scale=float(s), R=R, t=t, mask=m)
    return out


def check_conditions(res, allow_degenerate=False):
    """The conditions under which counts / selection are decided with room to spare. With
    allow_degenerate, hypotheses without a finite positive scale (all-duplicate samples) are let
    through: such rows count 0 on both sides by definition; every other row is held to the limits."""
    m = res["margins"]
    if not allow_degenerate:
        assert m["finite"], "a sampled hypothesis has no finite positive scale"
    assert m["sigma"] >= MIN_SIGMA_RATIO, m["sigma"]
    assert m["thr"] >= MIN_THR_MARGIN, m["thr"]
    assert m["stop"] >= MIN_STOP_MARGIN, m["stop"]
    assert m["refit_sigma"] >= MIN_SIGMA_RATIO, m["refit_sigma"]
