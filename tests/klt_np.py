"""NumPy restatement of the pyramidal Lucas-Kanade tracking of the tracker's features (Tracker::featureTracking,
tracker.cpp:623-690): cv::calcOpticalFlowPyrLK with OPTFLOW_LK_GET_MIN_EIGENVALS step by step, except that every quantity OpenCV
keeps as an integer stays an exact integer -- the sums over the window included -- and everything else is fp64.

Written from the definition, not from the kernel: one feature at a time, vectorised over its window, all sums in NumPy int64.
Beside the results it records, per feature, the exit taken at every level and the smallest margin of every discrete decision, so
that a scene can be shown to sit away from every tie before a device result is compared bit for bit."""
import math

import numpy as np

EXITS = ("eps", "oscillation", "count", "next_out", "prev_out", "min_eig")
K5 = (1, 4, 6, 4, 1)
W_ONE = 1 << 14
FLT_SCALE = 1.0 / (1 << 20)
D_FLOOR = 2.0 ** -23
DEFAULTS = dict(win=(31, 31), max_level=2, max_iter=30, eps=0.01, min_eig_thr=0.003)


def reflect(i, n):
    """reflect-101: -1 -> 1, n -> n - 2 (one reflection: every caller stays within n of the image)."""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def pyr_down(img):
    """(W, H) -> ((W+1)/2, (H+1)/2): [1 4 6 4 1] in both directions, + 128 >> 8, separable."""
    H, W = img.shape
    W2, H2 = (W + 1) // 2, (H + 1) // 2
    I = img.astype(np.int64)
    xs = reflect(2 * np.arange(W2)[None, :] + np.arange(-2, 3)[:, None], W)
    hs = sum(K5[i] * I[:, xs[i]] for i in range(5))
    ys = reflect(2 * np.arange(H2)[None, :] + np.arange(-2, 3)[:, None], H)
    v = sum(K5[j] * hs[ys[j], :] for j in range(5))
    return ((v + 128) >> 8).astype(np.uint8)


def scharr(img):
    """int16 dIx, dIy: [3 10 3] across, [-1 0 1] along, the image mirrored at its edge."""
    H, W = img.shape
    I = img.astype(np.int64)
    P = I[reflect(np.arange(-1, H + 1), H)][:, reflect(np.arange(-1, W + 1), W)]
    sv = 3 * P[:-2, :] + 10 * P[1:-1, :] + 3 * P[2:, :]
    sh = 3 * P[:, :-2] + 10 * P[:, 1:-1] + 3 * P[:, 2:]
    return (sv[:, 2:] - sv[:, :-2]).astype(np.int16), (sh[2:, :] - sh[:-2, :]).astype(np.int16)


def n_levels(width, height, win, max_level):
    """Rule 1: the largest l <= max_level with W_k > win_w and H_k > win_h for every k <= l; -1 if level 0 fails."""
    lv = -1
    for l in range(max_level + 1):
        if not (width > win[0] and height > win[1]):
            break
        lv = l
        width, height = (width + 1) // 2, (height + 1) // 2
    return lv


def build_pyramid(img, win, max_level):
    """-> list of (image uint8, dIx int16, dIy int16) for levels 0 ... levels."""
    img = np.ascontiguousarray(img, np.uint8)
    lv = n_levels(img.shape[1], img.shape[0], win, max_level)
    if lv < 0:
        raise ValueError("the window does not fit level 0")
    out = []
    for l in range(lv + 1):
        if l:
            img = pyr_down(img)
        out.append((img,) + scharr(img))
    return out


class Margins(dict):
    def note(self, name, value):
        value = float(value)
        if value < self.get(name, math.inf):
            self[name] = value


def _floor(v, m):
    f = math.floor(v)
    m.note("floor", min(v - f, f + 1.0 - v))
    return f


def _weights(a, b, m):
    args = ((1.0 - a) * (1.0 - b) * 16384.0, a * (1.0 - b) * 16384.0, (1.0 - a) * b * 16384.0)
    for v in args:
        m.note("weight_tie", abs(v - math.floor(v) - 0.5))
    w00, w01, w10 = (int(np.rint(v)) for v in args)
    return w00, w01, w10, W_ONE - w00 - w01 - w10


def _inside(fx, fy, W, H, win):
    """The bounds test on the floored corner, taken in fp64 (so that it also decides for values no integer holds)."""
    return fx >= -win[0] and fx < W and fy >= -win[1] and fy < H


def _sample(plane, ix, iy, win, w, shift, mirror):
    H, W = plane.shape
    ys, xs = iy + np.arange(win[1] + 1), ix + np.arange(win[0] + 1)
    if mirror:
        patch = plane[reflect(ys, H)][:, reflect(xs, W)].astype(np.int64)
    else:
        oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
        patch = plane[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)].astype(np.int64) * (oky[:, None] & okx[None, :])
    v = patch[:-1, :-1] * w[0] + patch[:-1, 1:] * w[1] + patch[1:, :-1] * w[2] + patch[1:, 1:] * w[3]
    return (v + (1 << (shift - 1))) >> shift


def track_one(pyr_prev, pyr_cur, pt, win, max_iter, eps, min_eig_thr):
    """One feature.  pt: the float32 pair.  -> (x, y, status, min_eig, exits per level from the top, margins)."""
    m = Margins()
    px, py = float(pt[0]), float(pt[1])
    if not (math.isfinite(px) and math.isfinite(py)):
        return px, py, 0, 0.0, [], m
    levels = len(pyr_prev) - 1
    hx, hy = (win[0] - 1) * 0.5, (win[1] - 1) * 0.5
    status, min_eig_out = 1, 0.0
    nx = ny = 0.0
    exits = []
    for l in range(levels, -1, -1):
        I, dIx, dIy = pyr_prev[l]
        J = pyr_cur[l][0]
        H, W = I.shape
        scale = 1.0 / (1 << l)
        qx, qy = px * scale, py * scale
        if l == levels:
            nx, ny = qx, qy
        else:
            nx, ny = 2.0 * nx, 2.0 * ny
        qx, qy = qx - hx, qy - hy
        fx, fy = _floor(qx, m), _floor(qy, m)
        if not _inside(fx, fy, W, H, win):
            if l == 0:
                status, min_eig_out = 0, 0.0
            exits.append("prev_out")
            continue
        ix, iy = int(fx), int(fy)
        w = _weights(qx - fx, qy - fy, m)
        Iw = _sample(I, ix, iy, win, w, 9, True)
        gx = _sample(dIx, ix, iy, win, w, 14, False)
        gy = _sample(dIy, ix, iy, win, w, 14, False)
        A11, A12, A22 = int((gx * gx).sum()) * FLT_SCALE, int((gx * gy).sum()) * FLT_SCALE, int((gy * gy).sum()) * FLT_SCALE
        D = A11 * A22 - A12 * A12
        dA = A11 - A22
        min_eig = (A22 + A11 - math.sqrt(dA * dA + 4.0 * A12 * A12)) / float(2 * win[0] * win[1])
        if l == 0:
            min_eig_out = min_eig
        m.note("min_eig", abs(min_eig - min_eig_thr) / min_eig_thr if min_eig_thr > 0 else abs(min_eig))
        m.note("det", abs(D - D_FLOOR))
        if min_eig < min_eig_thr or D < D_FLOOR:
            if l == 0:
                status = 0
            exits.append("min_eig")
            continue
        nx, ny = nx - hx, ny - hy
        pdx = pdy = 0.0
        how = "count"
        for j in range(max_iter):
            fx, fy = _floor(nx, m), _floor(ny, m)
            if not _inside(fx, fy, W, H, win):
                if l == 0:
                    status = 0
                how = "next_out"
                break
            w = _weights(nx - fx, ny - fy, m)
            diff = _sample(J, int(fx), int(fy), win, w, 9, True) - Iw
            b1, b2 = int((diff * gx).sum()) * FLT_SCALE, int((diff * gy).sum()) * FLT_SCALE
            dx, dy = (A12 * b2 - A22 * b1) / D, (A12 * b1 - A11 * b2) / D
            nx, ny = nx + dx, ny + dy
            d2 = dx * dx + dy * dy
            m.note("eps", abs(d2 - eps * eps))
            if d2 <= eps * eps:
                how = "eps"
                break
            if j > 0:
                sx, sy = abs(dx + pdx), abs(dy + pdy)
                m.note("oscillation", min(abs(sx - 0.01), abs(sy - 0.01)))
                if sx < 0.01 and sy < 0.01:
                    nx, ny = nx - dx * 0.5, ny - dy * 0.5
                    how = "oscillation"
                    break
            pdx, pdy = dx, dy
        nx, ny = nx + hx, ny + hy
        exits.append(how)
    return nx, ny, status, min_eig_out, exits, m


def post_filter(cur_xy, status, width, height, margins=None):
    """tracker.cpp:658-686: kept iff tracked and inside [-0.5, W - 0.5] x [-0.5, H - 0.5]; -> ascending indices."""
    keep = []
    for i, ((x, y), s) in enumerate(zip(cur_xy, status)):
        if s and margins is not None:
            margins[i].note("post", min(abs(x + 0.5), abs(y + 0.5), abs(x - (width - 0.5)), abs(y - (height - 0.5))))
        if s and x >= -0.5 and y >= -0.5 and x <= width - 0.5 and y <= height - 0.5:
            keep.append(i)
    return np.array(keep, np.int32)


def track(pyr_prev, pyr_cur, prev_xy, win=(31, 31), max_iter=30, eps=0.01, min_eig_thr=0.003):
    """All features of a frame (prev_xy: float32 [n, 2]) against two pyramids of build_pyramid -> dict of cur_xy fp64 [n, 2],
    status uint8 [n], min_eig [n], keep_idx, kept_prev, kept_cur, exits (list per feature), margins (Margins per feature)."""
    prev = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
    n = len(prev)
    cur, status, min_eig = np.zeros((n, 2)), np.zeros(n, np.uint8), np.zeros(n)
    exits, margins = [], []
    for i in range(n):
        x, y, s, e, ex, m = track_one(pyr_prev, pyr_cur, prev[i], win, max_iter, eps, min_eig_thr)
        cur[i], status[i], min_eig[i] = (x, y), s, e
        exits.append(ex)
        margins.append(m)
    H, W = pyr_cur[0][0].shape
    keep = post_filter(cur, status, W, H, margins)
    return dict(cur_xy=cur, status=status, min_eig=min_eig, keep_idx=keep, kept_prev=prev[keep].astype(np.float64),
                kept_cur=cur[keep], exits=exits, margins=margins)


def worst_margin(margins):
    """The smallest margin over a list of Margins, with its name."""
    best = (math.inf, None)
    for m in margins:
        for k, v in m.items():
            if v < best[0]:
                best = (v, k)
    return best
