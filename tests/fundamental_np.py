"""NumPy restatement of the fundamental-matrix RANSAC filter of the tracker's matches (xk_trk_*), written
independently of the device code: null space by numpy.linalg.svd, the cubic's coefficients by interpolating four
determinants, its roots by numpy.roots.  Same sampler, same error, same score rule, same selection key, same float32
handling as the device -- so masks can be compared bit for bit on scenes whose margin is not at round-off, and candidates
hypothesis by hypothesis.

Convention: p1 = previous, p2 = current, p2^T F p1 = 0.  The solve runs on conditioned coordinates x = (u - cx)/fx,
y = (v - cy)/fy, the score on pixels; K = (fx, fy, cx, cy).

The degenerate rules (all coefficients below the floor: the basis itself; a leading coefficient below it: F1 - F2 and the
deflated polynomial) are restated too, but they name the BASIS of the null space, and an SVD basis is not the Householder
basis: a hypothesis that takes one of them, or comes within two decades of the floor, is reported as not `kept`."""
import numpy as np

_M64 = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15
COEF_FLOOR = 1e-12                      # XK_FUND_COEF_FLOOR
K_DEFAULT = (458.654, 457.296, 367.215, 248.375)
WIDTH, HEIGHT = 752, 480


def _mix(z):
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample(seed, h, n):
    """The seven distinct point indices of hypothesis h (synth.SplitMix value i = mix(seed + (i+1) golden), i = 7h+k)."""
    picks = []
    for k in range(7):
        z = _mix((seed & _M64) + (7 * h + k + 1) * _GOLD)
        r = ((z >> 32) * (n - k)) >> 32
        for p in sorted(picks):
            if r >= p:
                r += 1
        picks.append(int(r))
    return picks


def through_float(xy):
    """What the RANSAC sees of fp64 pixels: cv::Point2f (tracker.cpp:251-256), widened back."""
    return np.asarray(xy, np.float64).reshape(-1, 2).astype(np.float32).astype(np.float64)


def condition(xy, K):
    fx, fy, cx, cy = K
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    return np.stack([(xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy, np.ones(len(xy))], axis=1)


def undistort(dist_xy, K, s):
    """Camera::undistort (camera.cpp:69-87): distorted pixels -> undistorted pixels, fp64."""
    fx, fy, cx, cy = K
    d = np.asarray(dist_xy, np.float64).reshape(-1, 2)
    x, y = (d[:, 0] - cx) / fx, (d[:, 1] - cy) / fy
    r = np.hypot(x, y)
    f = np.ones(len(d))
    if s != 0.0:
        big = r > 0.01
        f[big] = np.tan(r[big] * s) / (2.0 * np.tan(s / 2.0)) / r[big]
    return np.stack([f * x * fx + cx, f * y * fy + cy], axis=1)


def distort(xy, K, s):
    """The FOV model forwards: r_d = atan(2 r_u tan(s/2)) / s.  The generator's side; undistort inverts it."""
    fx, fy, cx, cy = K
    u = np.asarray(xy, np.float64).reshape(-1, 2)
    x, y = (u[:, 0] - cx) / fx, (u[:, 1] - cy) / fy
    r = np.hypot(x, y)
    f = np.ones(len(u))
    if s != 0.0:
        big = r > 1e-9
        f[big] = np.arctan(2.0 * r[big] * np.tan(s / 2.0)) / s / r[big]
    return np.stack([f * x * fx + cx, f * y * fy + cy], axis=1)


def to_pixels(Fn, K):
    """Unit norm, K^-T F K^-1, unit norm again."""
    fx, fy, cx, cy = K
    Ki = np.array([[1.0 / fx, 0.0, -cx / fx], [0.0, 1.0 / fy, -cy / fy], [0.0, 0.0, 1.0]])
    with np.errstate(all="ignore"):
        F = np.asarray(Fn, np.float64).reshape(3, 3)
        F = Ki.T @ (F / np.linalg.norm(F)) @ Ki
        return F / np.linalg.norm(F)


def to_conditioned(Fp, K):
    """Pixel F back to conditioned coordinates, unit norm (the coordinates candidates are compared in)."""
    fx, fy, cx, cy = K
    Km = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    F = Km.T @ np.asarray(Fp, np.float64).reshape(3, 3) @ Km
    n = np.linalg.norm(F)
    return F / n if n > 0 else F


def solve7(p1, p2, K):
    """Seven conditioned pairs [7, 3] -> dict(cands [m, 3, 3] pixel coordinates, lam (all roots, complex), general)."""
    A = np.einsum("pi,pj->pij", p2, p1).reshape(7, 9)
    N = np.linalg.svd(A)[2][7:]
    F1, F2 = N[0].reshape(3, 3), N[1].reshape(3, 3)
    D = F1 - F2
    ls = np.array([-1.0, 0.0, 1.0, 2.0])
    c = np.linalg.solve(np.vander(ls, 4, increasing=True), [np.linalg.det(F2 + l * D) for l in ls])
    out = dict(cands=np.zeros((0, 3, 3)), lam=np.zeros(0, complex), general=False)
    if not np.isfinite(c).all():
        return out
    cmax = np.abs(c).max()
    out["general"] = bool(cmax > 100 * COEF_FLOOR and abs(c[3]) > 100 * COEF_FLOOR * cmax)
    special = []
    if cmax <= COEF_FLOOR:
        lam, special = np.zeros(0, complex), [F1, F2]
    else:
        deg = max([k for k in range(4) if abs(c[k]) > COEF_FLOOR * cmax])
        lam = np.roots(c[deg::-1]).astype(complex) if deg > 0 else np.zeros(0, complex)
        if deg < 3:
            special = [D]
    real = sorted(l.real for l in lam if abs(l.imag) <= 1e-6 * max(abs(l), 1e-300))
    cands = []
    for Fn in [F2 + l * D for l in real] + special:
        Fp = to_pixels(Fn, K)
        if np.isfinite(Fp).all() and len(cands) < 3:
            cands.append(Fp)
    out.update(cands=np.array(cands).reshape(-1, 3, 3), lam=lam)
    return out


def ffro(Fa, Fb):
    """Frobenius distance of two unit-norm candidates up to sign."""
    return min(np.linalg.norm(Fa - Fb), np.linalg.norm(Fa + Fb))


def is_kept(sol, K):
    lam, cands = sol["lam"], sol["cands"]
    if not sol["general"] or not np.isfinite(lam).all():
        return False
    rel = np.abs(lam.imag) / np.maximum(np.abs(lam), 1e-300)
    if np.any((rel >= 1e-9) & (rel <= 1e-3)):
        return False
    cn = [to_conditioned(F, K) for F in cands]
    for a in range(len(cn)):
        for b in range(a + 1, len(cn)):
            if ffro(cn[a], cn[b]) < 1e-3:
                return False
    return True


def error(F, P1, P2):
    """OpenCV's fundamental-matrix error in pixels: max of the two squared point-to-epipolar-line distances."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    h1 = np.concatenate([P1, np.ones((len(P1), 1))], axis=1)
    h2 = np.concatenate([P2, np.ones((len(P2), 1))], axis=1)
    l2 = h1 @ F.T                                 # F p1: the line in the current image
    l1 = h2 @ F                                   # F^T p2
    with np.errstate(all="ignore"):
        d2 = np.einsum("pi,pi->p", h2, l2) ** 2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2)
        d1 = np.einsum("pi,pi->p", h1, l1) ** 2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2)
        return np.fmax(d1, d2)


def sample_residual(F, P1, P2, K, picks):
    """max |p2^T F p1| over the sample, conditioned coordinates, unit-norm F."""
    Fn = to_conditioned(F, K)
    return float(np.abs(np.einsum("pi,ij,pj->p", condition(P2[picks], K), Fn, condition(P1[picks], K))).max())


def ransac(prev_xy, cur_xy, K, threshold_px=0.3, n_hyp=1024, seed=0):
    """prev_xy / cur_xy: undistorted pixels (they pass through float32 here) -> dict(mask, F [3,3] pixel coordinates,
    n_inliers, winner, margin, kept [n_hyp] bool, cands [list of [m,3,3]], counts [list of [m]])."""
    P1, P2 = through_float(prev_xy), through_float(cur_xy)
    n = len(P1)
    out = dict(mask=np.zeros(n, np.uint8), F=np.zeros((3, 3)), n_inliers=0, winner=-1, margin=np.inf,
               kept=np.zeros(n_hyp, bool), cands=[], counts=[])
    if n < 7:
        return out
    c1, c2 = condition(P1, K), condition(P2, K)
    t2 = threshold_px * threshold_px
    best = (-1,)
    for h in range(n_hyp):
        s = sample(seed, h, n)
        sol = solve7(c1[s], c2[s], K)
        out["kept"][h] = is_kept(sol, K)
        out["cands"].append(sol["cands"])
        cnt, hb = [], None
        for F in sol["cands"]:
            d = error(F, P1, P2)
            inl = d <= t2
            c, sm = int(inl.sum()), float(d[inl].sum())
            cnt.append(c)
            if hb is None or c > hb[0] or (c == hb[0] and sm < hb[1]):
                hb = (c, sm, F, inl)
            with np.errstate(all="ignore"):
                m = np.abs(d / t2 - 1.0)
            if np.isfinite(m).any():
                out["margin"] = min(out["margin"], float(np.nanmin(m)))
        out["counts"].append(np.array(cnt, np.int32))
        if hb is not None and hb[0] > best[0]:
            best = (hb[0], h, hb[2], hb[3])
    if best[0] < 0:
        return out
    out.update(mask=best[3].astype(np.uint8), F=best[2], n_inliers=best[0], winner=best[1])
    return out


def filter_matches(prev_dist_xy, cur_dist_xy, K, s, threshold_px=0.3, n_hyp=1024, seed=0):
    """tracker.cpp:233-293: undistort both lists, RANSAC on their float casts, keep the masked pairs' fp64 coordinates."""
    up, uc = undistort(prev_dist_xy, K, s), undistort(cur_dist_xy, K, s)
    r = ransac(up, uc, K, threshold_px, n_hyp, seed)
    keep = np.flatnonzero(r["mask"]).astype(np.int32)
    r.update(keep_idx=keep, prev_xy=up[keep], cur_xy=uc[keep])
    return r


def make_pair(n, outlier_share, noise_px, seed, mode="general", s=0.0, K=K_DEFAULT):
    """Two consecutive frames of one camera -> (prev_xy, cur_xy, planted inlier mask), fp64 pixels [n, 2].
    general : translation 0.02-0.1 m, rotation <= 0.03 rad, points at 4-12 m depth
    rotation: the same with t = 0
    still   : the lists are equal
    A share of the current points is replaced by uniform pixels.  s != 0: the pixels are passed through the FOV distortion
    (the tracker's raw input); s = 0: they are the undistorted pixels."""
    fx, fy, cx, cy = K
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0.005, 0.03)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    t = rng.normal(size=3)
    t *= rng.uniform(0.02, 0.1) / np.linalg.norm(t)
    if mode == "rotation":
        t[:] = 0.0
    if mode == "still":
        t[:] = 0.0
        R = np.eye(3)
    prev = np.zeros((n, 2))
    cur = np.zeros((n, 2))
    for i in range(n):
        while True:
            p = np.array([rng.uniform(40, WIDTH - 40), rng.uniform(40, HEIGHT - 40)])
            X1 = np.array([(p[0] - cx) / fx, (p[1] - cy) / fy, 1.0]) * rng.uniform(4.0, 12.0)
            X2 = R @ X1 + t
            q = np.array([fx * X2[0] / X2[2] + cx, fy * X2[1] / X2[2] + cy])
            if X2[2] > 1.0 and 0 <= q[0] < WIDTH and 0 <= q[1] < HEIGHT:
                break
        prev[i], cur[i] = p, (p if mode == "still" else q)
    if noise_px > 0:
        prev += noise_px * rng.normal(size=(n, 2))
        cur += noise_px * rng.normal(size=(n, 2))
    inl = np.ones(n, bool)
    n_out = int(round(outlier_share * n))
    if n_out:
        bad = rng.choice(n, n_out, replace=False)
        inl[bad] = False
        cur[bad] = np.stack([rng.uniform(0, WIDTH, n_out), rng.uniform(0, HEIGHT, n_out)], axis=1)
    if s != 0.0:
        prev, cur = distort(prev, K, s), distort(cur, K, s)
    return prev, cur, inl
