"""numpy f64 restatement of lib/transform/umeyama.py's estimateSimilarityTransform with explicit
subsets (test infrastructure, like tests/parity.py), and the conditioning checks under which a
bit-different f64 evaluation (the HIP kernel's) must reach the same discrete decisions.

    res = ransac(src, dst, subsets)       # src / dst [N, 3] (f32 or f64), subsets [H, 5]
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


def ransac(src, dst, subsets, inlier_frac=INLIER_FRAC, conf=CONFIDENCE, min_ratio=MIN_RATIO):
    S = np.asarray(src, np.float64)
    T = np.asarray(dst, np.float64)
    subsets = np.asarray(subsets).reshape(-1, 5)
    N, H = S.shape[0], subsets.shape[0]
    inlier_t = inlier_frac * 2 * np.amax(np.linalg.norm(S - S.mean(0), axis=1))
    counts = np.zeros(H, np.int64)
    masks = np.zeros((H, N), bool)
    thr_margin, sig_ratio, all_finite = np.inf, np.inf, True
    for h in range(H):
        ids = subsets[h]
        with np.errstate(all="ignore"):
            s, R, t, sig = umeyama(S[ids], T[ids])
        ok = np.isfinite(s) and s > 0
        all_finite &= bool(ok)
        if not ok:
            continue
        sig_ratio = min(sig_ratio, sig[1] / sig[0])
        res = np.linalg.norm(T - (S @ (s * R).T + t), axis=1)
        thr = s * inlier_t
        masks[h] = res < thr
        counts[h] = masks[h].sum()
        thr_margin = min(thr_margin, np.abs(res - thr).min() / thr)
    best, best_h, stop, stop_margin = 0.0, -1, H - 1, np.inf
    for i in range(H):
        ratio = counts[i] / N
        if ratio > best:
            best, best_h = ratio, i
        e = 1 - (1 - best ** 5) ** i
        stop_margin = min(stop_margin, abs(e - conf))
        if e > conf:
            stop = i
            break
    failed = best < min_ratio
    out = dict(counts=counts, stop=stop, failed=bool(failed), inlier_t=inlier_t,
               margins=dict(thr=thr_margin, sigma=sig_ratio, stop=stop_margin, finite=all_finite, refit_sigma=np.inf))
    if failed:
        out.update(best_hyp=-1, inliers=0, scale=1.0, R=np.eye(3), t=np.zeros(3), mask=np.zeros(N, bool))
        return out
    m = masks[best_h]
    s, R, t, sig = umeyama(S[m], T[m])
    out["margins"]["refit_sigma"] = sig[1] / sig[0]
    out.update(best_hyp=int(best_h), inliers=int(counts[best_h]), scale=float(s), R=R, t=t, mask=m)
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
