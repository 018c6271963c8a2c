"""NumPy restatement of the essential-matrix RANSAC filter (xk_pr_essential_ransac), written
independently of the device code: null space by SVD, elimination by numpy.linalg.solve, roots by the eigen-
decomposition of the 10 x 10 action matrix (multiplication by x in the quotient ring).  Same sampler, same score
rule, same selection key as the device -- so masks can be compared bit for bit on scenes whose margin is not at
round-off, and candidates hypothesis by hypothesis.

Convention: rec^T E cur = 0 on normalised coordinates x = (u - cx)/fx, y = (v - cy)/fy."""
import itertools

import numpy as np

_M64 = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15

# monomials of degree <= 3 in (x, y, z) as sorted triples over (x, y, z, 1) = (0, 1, 2, 3)
_MONOS = list(itertools.combinations_with_replacement(range(4), 3))
_MID = {m: i for i, m in enumerate(_MONOS)}
_TENSOR_TO_MONO = np.array([_MID[tuple(sorted(t))] for t in itertools.product(range(4), repeat=3)])
X, Y, Z, W = 0, 1, 2, 3
_HI = [_MID[tuple(sorted(m))] for m in [(X, X, X), (X, X, Y), (X, Y, Y), (Y, Y, Y), (X, X, Z), (X, Y, Z), (Y, Y, Z),
                                         (X, Z, Z), (Y, Z, Z), (Z, Z, Z)]]
_LO_M = [(X, X, W), (X, Y, W), (Y, Y, W), (X, Z, W), (Y, Z, W), (Z, Z, W), (X, W, W), (Y, W, W), (Z, W, W), (W, W, W)]
_LO = [_MID[tuple(sorted(m))] for m in _LO_M]
_EPS3 = np.zeros((3, 3, 3))
for _p in itertools.permutations(range(3)):
    _EPS3[_p] = np.linalg.det(np.eye(3)[list(_p)])


def _mix(z):
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample(seed, h, n):
    """The five distinct point indices of hypothesis h (synth.SplitMix value i = mix(seed + (i+1) golden), i = 5h+k)."""
    picks = []
    for k in range(5):
        z = _mix((seed & _M64) + (5 * h + k + 1) * _GOLD)
        r = ((z >> 32) * (n - k)) >> 32
        for p in sorted(picks):
            if r >= p:
                r += 1
        picks.append(int(r))
    return picks


def normalise(xy, fx, fy, cx, cy):
    xy = np.asarray(xy, np.float32).reshape(-1, 2).astype(np.float64)
    return np.stack([(xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy, np.ones(len(xy))], axis=1)


def _cubics(N):
    """The ten cubic constraints on E = x N0 + y N1 + z N2 + N3 as a 10 x 20 matrix over _MONOS."""
    E = N.reshape(4, 3, 3).transpose(1, 2, 0)                       # [i, j, var]
    EEt = np.einsum("ima,kmb->ikab", E, E)
    tr = np.einsum("iiab->ab", EEt)
    C = 2.0 * np.einsum("ikab,kjc->ijabc", EEt, E) - np.einsum("ab,ijc->ijabc", tr, E)
    det = np.einsum("ijk,ia,jb,kc->abc", _EPS3, E[0], E[1], E[2])
    rows = [np.bincount(_TENSOR_TO_MONO, det.ravel(), 20)]
    for i in range(3):
        for j in range(3):
            rows.append(np.bincount(_TENSOR_TO_MONO, C[i, j].ravel(), 20))
    return np.array(rows)


def constraint_residual(E):
    """max |.| over det E and 2 E E^T E - tr(E E^T) E."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    EEt = E @ E.T
    return max(abs(np.linalg.det(E)), np.abs(2.0 * EEt @ E - np.trace(EEt) * E).max())


def solve5(cur5, rec5):
    """Five normalised pairs -> (candidates [m, 3, 3] of unit Frobenius norm, eigenvalues [10] of the action matrix)."""
    A = np.einsum("pi,pj->pij", rec5, cur5).reshape(5, 9)
    N = np.linalg.svd(A)[2][5:]
    M = _cubics(N)
    none = np.zeros((0, 3, 3)), np.full(10, np.nan, complex)
    try:
        with np.errstate(all="ignore"):
            B = np.linalg.solve(M[:, _HI], M[:, _LO])
    except np.linalg.LinAlgError:
        return none
    if not np.isfinite(B).all():
        return none
    Act = np.zeros((10, 10))
    for i, m in enumerate(_LO_M):
        t = _MID[tuple(sorted((X,) + tuple(v for v in m if v != W) + (W,) * (m.count(W) - 1)))]
        if t in _HI:
            Act[i] = -B[_HI.index(t)]
        else:
            Act[i, _LO.index(t)] = 1.0
    lam, V = np.linalg.eig(Act)
    out = []
    for k in range(10):
        if abs(lam[k].imag) > 1e-6 * max(abs(lam[k]), 1e-300):
            continue
        v = V[:, k].real
        with np.errstate(all="ignore"):
            xyz = v[6:9] / v[9]
            Ec = (xyz[0] * N[0] + xyz[1] * N[1] + xyz[2] * N[2] + N[3])
            Ec = Ec / np.linalg.norm(Ec)
        if not np.isfinite(Ec).all():
            return none
        out.append(Ec.reshape(3, 3))
    return np.array(out).reshape(-1, 3, 3), lam


def efro(Ea, Eb):
    """Frobenius distance of two unit-norm candidates up to sign."""
    return min(np.linalg.norm(Ea - Eb), np.linalg.norm(Ea + Eb))


def is_kept(cands, lam):
    if not np.isfinite(lam).all():
        return False
    rel = np.abs(lam.imag) / np.maximum(np.abs(lam), 1e-300)
    if np.any((rel >= 1e-9) & (rel <= 1e-3)):
        return False
    for a in range(len(cands)):
        for b in range(a + 1, len(cands)):
            if efro(cands[a], cands[b]) < 1e-3:
                return False
    return True


def sampson(E, cur, rec):
    """Squared Sampson distance of every pair under rec^T E cur = 0."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    Ec = cur @ E.T
    Etr = rec @ E
    num = np.einsum("pi,pi->p", rec, Ec) ** 2
    den = Ec[:, 0] ** 2 + Ec[:, 1] ** 2 + Etr[:, 0] ** 2 + Etr[:, 1] ** 2
    with np.errstate(all="ignore"):
        return num / den


def ransac(cur_xy, rec_xy, fx, fy, cx, cy, threshold_px=1.0, n_hyp=1024, seed=0):
    """-> dict(mask, E, n_inliers, winner, margin, kept [n_hyp] bool, cands [list of [m,3,3]], counts [list of [m]])."""
    cur, rec = normalise(cur_xy, fx, fy, cx, cy), normalise(rec_xy, fx, fy, cx, cy)
    n = len(cur)
    out = dict(mask=np.zeros(n, np.uint8), E=np.zeros((3, 3)), n_inliers=0, winner=-1, margin=np.inf,
               kept=np.zeros(n_hyp, bool), cands=[], counts=[])
    if n < 5:
        return out
    t2 = (threshold_px / ((fx + fy) / 2.0)) ** 2
    best = (-1, 0, 0.0, None)                                         # count, -h, sum, E
    dists = []
    for h in range(n_hyp):
        s = sample(seed, h, n)
        cands, lam = solve5(cur[s], rec[s])
        out["kept"][h] = is_kept(cands, lam)
        out["cands"].append(cands)
        cnt, dd = [], []
        hb = None
        for E in cands:
            d = sampson(E, cur, rec)
            inl = d <= t2
            c, sm = int(inl.sum()), float(d[inl].sum())
            cnt.append(c)
            dd.append(d)
            if hb is None or c > hb[0] or (c == hb[0] and sm < hb[1]):
                hb = (c, sm, E, inl)
        out["counts"].append(np.array(cnt, np.int32))
        dists.append(dd)
        if hb is not None and hb[0] > best[0]:
            best = (hb[0], h, hb[1], hb[2], hb[3])
    if best[0] < 0:
        return out
    out.update(mask=best[4].astype(np.uint8), E=best[3], n_inliers=best[0], winner=best[1])
    for h in range(n_hyp):
        for c, d in zip(out["counts"][h], dists[h]):
            if c >= best[0] - 1:
                with np.errstate(all="ignore"):
                    out["margin"] = min(out["margin"], float(np.nanmin(np.abs(d / t2 - 1.0))))
    return out


def make_scene(n, outlier_share, noise_px, seed, f=460.0, width=752, height=480):
    """Two cameras 0.3-0.9 m apart rotated by <= 0.2 rad, points at 4-12 m depth, a share of the received points
    replaced by uniform pixels; float32 pixels.  -> (cur_xy, rec_xy, planted inlier mask, E_true, K=(fx,fy,cx,cy))."""
    rng = np.random.default_rng(seed)
    cx, cy = width / 2.0, height / 2.0
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0.05, 0.2)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    t = rng.normal(size=3)
    t *= rng.uniform(0.3, 0.9) / np.linalg.norm(t)
    cur_xy = np.zeros((n, 2))
    rec_xy = np.zeros((n, 2))
    for i in range(n):
        while True:
            p = np.array([rng.uniform(40, width - 40), rng.uniform(40, height - 40)])
            Xc = np.array([(p[0] - cx) / f, (p[1] - cy) / f, 1.0]) * rng.uniform(4.0, 12.0)
            Xr = R @ Xc + t
            q = np.array([f * Xr[0] / Xr[2] + cx, f * Xr[1] / Xr[2] + cy])
            if Xr[2] > 1.0 and 0 <= q[0] < width and 0 <= q[1] < height:
                break
        cur_xy[i], rec_xy[i] = p, q
    if noise_px > 0:
        cur_xy += noise_px * rng.normal(size=(n, 2))
        rec_xy += noise_px * rng.normal(size=(n, 2))
    inl = np.ones(n, bool)
    n_out = int(round(outlier_share * n))
    if n_out:
        bad = rng.choice(n, n_out, replace=False)
        inl[bad] = False
        rec_xy[bad] = np.stack([rng.uniform(0, width, n_out), rng.uniform(0, height, n_out)], axis=1)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return cur_xy.astype(np.float32), rec_xy.astype(np.float32), inl, E / np.linalg.norm(E), (f, f, cx, cy)
