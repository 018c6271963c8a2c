"""NumPy restatement of the photometric calibration of the tracker's images (xk_trk_photo_*; Tracker::calibrateImage,
tracker.cpp:761-877, and IRPhotoCalib, irPhotoCalib.cpp), written from the definition, not from the kernels: the box-mean
intensity in exact integers, the gain RANSAC with the closed-form fit, the parameter chain operation by operation in Python
floats (IEEE fp64, no contraction), and the per-pixel correction in float32 arrays, every operation rounded once.

The sampler is the RANSAC filters' (fundamental_np), drawn four at a time; the tracking is klt_np's."""
import math

import numpy as np

import klt_np as knp
from fundamental_np import _GOLD, _M64, _mix

RING = 15
INLIER = 8.0e-3
PRIOR_W = 0.1
W2 = PRIOR_W * PRIOR_W
LUT = np.array([2 * i if i < 128 else (255 if i == 128 else 512 - 2 * i) for i in range(256)], np.uint8)


def sample(seed, h, n):
    """The four distinct point indices of hypothesis h (value i = mix(seed + (i+1) golden), i = 4h+k)."""
    picks = []
    for k in range(4):
        z = _mix((seed & _M64) + (4 * h + k + 1) * _GOLD)
        r = ((z >> 32) * (n - k)) >> 32
        for p in sorted(picks):
            if r >= p:
                r += 1
        picks.append(int(r))
    return picks


# ---- computeIntensity (tracker.cpp:860-877) ----
def intensity(img, xy, kernel_size):
    """-> (value fp64 [n], sum int32 [n], count int32 [n]) of the clipped windows rows y - hk ... y + hk - 1, columns likewise."""
    H, W = img.shape
    hk = kernel_size // 2
    I = img.astype(np.int64)
    pts = np.asarray(xy, np.int64).reshape(-1, 2)
    value, s, c = np.zeros(len(pts)), np.zeros(len(pts), np.int32), np.zeros(len(pts), np.int32)
    for i, (x, y) in enumerate(pts):
        x0, x1, y0, y1 = max(x - hk, 0), min(x + hk, W), max(y - hk, 0), min(y + hk, H)
        if x1 > x0 and y1 > y0:
            s[i] = int(I[y0:y1, x0:x1].sum())
            c[i] = (x1 - x0) * (y1 - y0)
            value[i] = float(s[i]) / (255.0 * float(c[i]))
    return value, s, c


# ---- EstimateGainsRansac (irPhotoCalib.cpp:221-312) ----
def fit_from_sums(uu, uv, vv, uo, vo):
    """The minimum of sum (o - p a - (1 - p) b)^2 + w^2 (a - 1)^2 + w^2 b^2, u = p, v = 1 - p: Cramer on the normal equations."""
    m00, m11, r0 = uu + W2, vv + W2, uo + W2
    det = m00 * m11 - uv * uv
    return (r0 * m11 - uv * vo) / det, (m00 * vo - uv * r0) / det


def fit(o, p, order=None, dtype=np.float64):
    """The closed form over the points in `order` (default: as given), summed one by one from zero in dtype."""
    o, p = np.asarray(o, dtype), np.asarray(p, dtype)
    idx = range(len(o)) if order is None else order
    uu = uv = vv = uo = vo = dtype(0)
    one = dtype(1)
    for i in idx:
        u, v = p[i], one - p[i]
        uu, uv, vv, uo, vo = uu + u * u, uv + u * v, vv + v * v, uo + u * o[i], vo + v * o[i]
    if dtype is np.float64:
        return fit_from_sums(float(uu), float(uv), float(vv), float(uo), float(vo))
    w2 = dtype(PRIOR_W) * dtype(PRIOR_W)
    m00, m11, r0 = uu + w2, vv + w2, uo + w2
    det = m00 * m11 - uv * uv
    return (r0 * m11 - uv * vo) / det, (m00 * vo - uv * r0) / det


def residual(o, p, a, b):
    """|o - (p (a - b) + b)| per point, the operations in that order."""
    return np.abs(np.asarray(o, np.float64) - (np.asarray(p, np.float64) * (a - b) + b))


def gains_ransac(o_hist, o_cur, n_hyp, seed):
    """One group of more than 4 points -> dict of ab [n_hyp, 2], inliers [n_hyp], winner, mask (of the winner), a, b (the refit),
    support, margin (the smallest | |d| - 8e-3 | over every hypothesis and point), runner_up (the best count of another
    hypothesis)."""
    o, p = np.asarray(o_hist, np.float64), np.asarray(o_cur, np.float64)
    n = len(o)
    ab, cnt = np.zeros((n_hyp, 2)), np.zeros(n_hyp, np.int32)
    margin = math.inf
    masks = []
    for h in range(n_hyp):
        a, b = fit(o, p, sample(seed, h, n))
        d = residual(o, p, a, b)
        ab[h] = (a, b)
        masks.append(d < INLIER)
        cnt[h] = int(masks[-1].sum())
        margin = min(margin, float(np.abs(d - INLIER).min()))
    winner = int(np.argmax(cnt))                       # the first of the largest: ties to the lowest hypothesis
    support = int(cnt[winner])
    mask = masks[winner]
    a, b = fit(o, p, np.flatnonzero(mask)) if support > 0 else (1.0, 0.0)
    others = np.delete(cnt, winner)
    return dict(ab=ab, inliers=cnt, winner=winner, mask=mask, a=a, b=b, support=support, margin=margin,
                runner_up=int(others.max()) if len(others) else -1)


# ---- the parameter chain (irPhotoCalib.cpp:68-82, :104-160, :212-218) ----
def relative_gains(a1, b1, a2, b2):
    e12 = (a2 - b2) / (a1 - b1)
    b12 = (b2 - b1) / (a1 - b1)
    return e12 + b12, b12


def chain_gains(a01, b01, a12, b12):
    e02 = (a01 - b01) * (a12 - b12)
    b02 = b01 + (a01 - b01) * b12
    return e02 + b02, b02


def process_frame(ring, groups, frame_back, n_hyp, seed, eps_gap, eps_base):
    """ring: list of (a, b), changed in place; groups: list of (o_hist, o_cur) -> dict of a_rel, b_rel [G], support [G], frame_ab
    [4], ransac (per group, None for a group of <= 4 points)."""
    size = len(ring)
    ap, bp = ring[-1]
    w_a = w_b = 0.0
    w_count = 0
    a_rel, b_rel, support, res = [], [], [], []
    for g, ((oh, oc), fb) in enumerate(zip(groups, frame_back)):
        if not 1 <= fb <= size:
            raise ValueError("frame_back outside the ring")
        if len(oh) <= 4:
            a_rel.append(1.0), b_rel.append(0.0), support.append(0), res.append(None)
            continue
        r = gains_ransac(oh, oc, n_hyp, seed + g)
        a_rel.append(r["a"]), b_rel.append(r["b"]), support.append(r["support"]), res.append(r)
        aoh, boh = ring[size - fb]
        aoc, boc = chain_gains(aoh, boh, r["a"], r["b"])
        apc, bpc = relative_gains(ap, bp, aoc, boc)
        w_a += apc * float(r["support"])
        w_b += bpc * float(r["support"])
        w_count += r["support"]
    wa, wb = (w_a / float(w_count), w_b / float(w_count)) if w_count >= 5 else (1.0, 0.0)
    delta = (1.0 - (wa - wb)) * eps_gap
    wa = wa + delta
    wb = wb - delta
    wa = wa - (wa - 1.0) * eps_base
    wb = wb - wb * eps_base
    ao, bo = chain_gains(ap, bp, wa, wb)
    ring.append((ao, bo))
    if len(ring) > RING:
        del ring[0]
    return dict(a_rel=np.array(a_rel), b_rel=np.array(b_rel), support=np.array(support, np.int32), frame_ab=np.array([wa, wb, ao, bo]),
                ransac=res)


# ---- getCorrectedImage (irPhotoCalib.cpp:442-472) ----
def correct(img, a, b, ps=None):
    """uint8 [H, W] -> uint8 [H, W]; float32 arrays, one rounding per operation."""
    f32 = np.float32
    v = img.astype(f32)
    ps = np.zeros(img.shape, f32) if ps is None else np.asarray(ps, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        f = v * (f32(1.0) / f32(255.0))
        c = ((f * f32(a - b) + f32(b)) - ps) * f32(255.0)
    ok = np.isfinite(c) & (np.abs(c) < f32(2147483648.0))
    x = np.where(ok, c, f32(0)).astype(np.int64)        # (astype truncates toward zero)
    m = np.where(x < 0, -((-x) % 256), x % 256)        # C's sign rule
    u = np.maximum(m, 0)
    return LUT[u]


# ---- calibrateImage (tracker.cpp:761-858) ----
def calibrate(state, raw_prev, raw_cur, prev_xy, prev_intensity, n_hyp, seed, kernel_size, eps_gap, eps_base, klt, ps=None):
    """state: dict(ring=[(a, b), ...], done=bool), changed in place.  klt: dict(win, max_level, max_iter, eps, min_eig_thr).
    -> dict of keep_idx, intensity, sum, count, estimated, a_rel, b_rel, support, frame_ab, image (the working image after the call),
    track (klt_np's result, None with fewer than 4 features), ransac."""
    prev = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
    out = dict(keep_idx=np.zeros(0, np.int32), intensity=np.zeros(0), sum=np.zeros(0, np.int32), count=np.zeros(0, np.int32),
               estimated=False, a_rel=1.0, b_rel=0.0, support=0, frame_ab=np.zeros(4), track=None, ransac=None)

    def image():
        a, b = state["ring"][-1]
        return correct(raw_cur, a, b, ps) if state["done"] else raw_cur.copy()

    if len(prev) < 4:
        out["image"] = image()
        return out
    p1 = knp.build_pyramid(raw_prev, klt["win"], klt["max_level"])
    p2 = knp.build_pyramid(raw_cur, klt["win"], klt["max_level"])
    tr = knp.track(p1, p2, prev, klt["win"], klt["max_iter"], klt["eps"], klt["min_eig_thr"])
    keep = tr["keep_idx"]
    out["track"], out["keep_idx"] = tr, keep
    ixy = np.trunc(tr["kept_cur"]).astype(np.int64)     # static_cast<int> (tracker.cpp:807-808)
    out["intensity"], out["sum"], out["count"] = intensity(raw_cur, ixy, kernel_size)
    if len(keep) < 4:
        out["image"] = image()
        return out
    r = process_frame(state["ring"], [(np.asarray(prev_intensity, np.float64)[keep], out["intensity"])], [1], n_hyp, seed, eps_gap, eps_base)
    state["done"] = True
    out.update(estimated=True, a_rel=float(r["a_rel"][0]), b_rel=float(r["b_rel"][0]), support=int(r["support"][0]), frame_ab=r["frame_ab"],
               ransac=r["ransac"][0])
    out["image"] = image()
    return out
