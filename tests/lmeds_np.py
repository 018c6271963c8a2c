"""NumPy restatement of the least-median-of-squares filter of the tracker's matches (xk_trk_fundamental_lmeds),
on top of fundamental_np: its sampler, seven-point solver, error and float32 handling.  What it adds is the definition:

  median    of a candidate: 0.5 (e[(n-1)//2] + e[n//2]) of its ascending errors, a NaN error counting as +inf; a candidate
            whose median is not finite is not a candidate
  winner    smallest median, then the lowest hypothesis, then the lowest candidate
  scale     sigma = 2.5 * 1.4826 * (1.0 + 5.0 / (n - 7)) * sqrt(med_min), at least 0.001, evaluated in this order
  inlier    error <= sigma * sigma

n < 8 keeps nothing.  For 8 <= n <= 13 both middle errors belong to the seven sample points, every median is round-off and the
selection arbitrary: such n are not compared against the device."""
import numpy as np

import fundamental_np as fnp


def median(e):
    """0.5 (e[(n-1)//2] + e[n//2]) of the ascending errors; NaN counts as +inf."""
    e = np.sort(np.where(np.isnan(e), np.inf, np.asarray(e, np.float64)))
    n = len(e)
    with np.errstate(all="ignore"):
        return 0.5 * (e[(n - 1) // 2] + e[n // 2])


def sigma_of(med, n):
    return max(2.5 * 1.4826 * (1.0 + 5.0 / (n - 7)) * float(np.sqrt(np.float64(med))), 0.001)


def lmeds(prev_xy, cur_xy, K, n_hyp=1024, seed=0):
    """prev_xy / cur_xy: undistorted pixels (they pass through float32 here) -> dict(mask, F [3,3], n_inliers, winner, median,
    sigma, kept [n_hyp] bool, cands [list of [m,3,3]], medians [n_hyp,3] (+inf: no candidate), gap, margin).
    gap: the relative distance between the smallest and the second smallest per-hypothesis median; margin: min |d / sigma^2 - 1|
    over the pairs under the winner."""
    P1, P2 = fnp.through_float(prev_xy), fnp.through_float(cur_xy)
    n = len(P1)
    out = dict(mask=np.zeros(n, np.uint8), F=np.zeros((3, 3)), n_inliers=0, winner=-1, median=0.0, sigma=0.0,
               kept=np.zeros(n_hyp, bool), cands=[], medians=np.full((n_hyp, 3), np.inf), gap=np.inf, margin=np.inf)
    if n < 8:
        return out
    c1, c2 = fnp.condition(P1, K), fnp.condition(P2, K)
    best = None
    for h in range(n_hyp):
        s = fnp.sample(seed, h, n)
        sol = fnp.solve7(c1[s], c2[s], K)
        out["kept"][h] = fnp.is_kept(sol, K)
        out["cands"].append(sol["cands"])
        for c, F in enumerate(sol["cands"]):
            m = median(fnp.error(F, P1, P2))
            out["medians"][h, c] = m if np.isfinite(m) else np.inf
            if np.isfinite(m) and (best is None or m < best[0]):      # (ascending h, then c: a tie keeps the earlier one)
                best = (m, h, F)
    if best is None:
        return out
    per_h = np.sort(out["medians"].min(axis=1))
    if len(per_h) > 1 and np.isfinite(per_h[1]):
        out["gap"] = float((per_h[1] - per_h[0]) / per_h[1]) if per_h[1] > 0 else 0.0
    med, w, F = best
    sig = sigma_of(med, n)
    d = fnp.error(F, P1, P2)
    mask = d <= sig * sig
    with np.errstate(all="ignore"):
        mg = np.abs(d / (sig * sig) - 1.0)
    out.update(mask=mask.astype(np.uint8), F=F, n_inliers=int(mask.sum()), winner=w, median=float(med), sigma=sig,
               margin=float(np.nanmin(mg)))
    return out


def filter_matches(prev_dist_xy, cur_dist_xy, K, s, n_hyp=1024, seed=0):
    """tracker.cpp:233-293 under outlier_method = cv::LMEDS: undistort both lists, LMedS on their float casts, keep the masked pairs."""
    up, uc = fnp.undistort(prev_dist_xy, K, s), fnp.undistort(cur_dist_xy, K, s)
    r = lmeds(up, uc, K, n_hyp, seed)
    keep = np.flatnonzero(r["mask"]).astype(np.int32)
    r.update(keep_idx=keep, prev_xy=up[keep], cur_xy=uc[keep])
    return r
