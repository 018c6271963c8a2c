"""NumPy restatement of DESIGN 3.13: the rotated-BRIEF (ORB) description of keypoints on one image -- the 7-tap blur, the
border filter, the direction (a fixed angle or the intensity centroid) and the 256 binary tests.

Written from the definition, brute force: the blur by explicit index tables (and blur_direct, a second statement as one 49-tap
2-D sum, which tests/test_orb_np.py holds against it), the moments by a loop over the disc's pixels, the tests per keypoint.
It shares no structure with csrc/xk_orb.hip.h (no tiles, no lanes, no ballots) and no helper with the package.  Every quantity
is an integer but the centroid direction, whose square root and divisions are correctly rounded float64 operations on exact
operands: what the device computes must equal this bit for bit."""
import math

import numpy as np

TAPS = (18, 34, 49, 54, 49, 34, 18)
UMAX = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)
HALF = 15
Q = 16384
MASK64 = (1 << 64) - 1
PATTERN_SEED = 0x4F5242
GOLDEN = 0x9E3779B97F4A7C15


def reflect(i, n):
    """index -k -> k, n - 1 + k -> n - 1 - k (the edge pixel is not repeated)"""
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    return i


def blur(img):
    """G uint8 [H, W]: the horizontal pass unrounded (<= 65280), the vertical pass on it, then (sum + 32768) >> 16."""
    I = np.asarray(img).astype(np.int64)
    H, W = I.shape
    hor = np.zeros((H, W), np.int64)
    for k, t in enumerate(TAPS):
        hor += t * I[:, [reflect(x + k - 3, W) for x in range(W)]]
    ver = np.zeros((H, W), np.int64)
    for k, t in enumerate(TAPS):
        ver += t * hor[[reflect(y + k - 3, H) for y in range(H)], :]
    return ((ver + 32768) >> 16).astype(np.uint8)


def blur_direct(img):
    """The same G from the direct 2-D definition: per pixel the 49-tap sum with the reflected index."""
    I = np.asarray(img).astype(np.int64)
    H, W = I.shape
    G = np.zeros((H, W), np.uint8)
    for y in range(H):
        rows = [reflect(y + j - 3, H) for j in range(7)]
        for x in range(W):
            s = 0
            for j in range(7):
                row = I[rows[j]]
                for k in range(7):
                    s += TAPS[j] * TAPS[k] * int(row[reflect(x + k - 3, W)])
            G[y, x] = (s + 32768) >> 16
    return G


def kept(xy, W, H, edge):
    """KeyPointsFilter::runByImageBorder: the indices of the keypoints with edge <= x < W - edge, edge <= y < H - edge."""
    return [i for i, (x, y) in enumerate(np.asarray(xy).reshape(-1, 2).tolist()) if edge <= x < W - edge and edge <= y < H - edge]


def moments(img, x, y):
    """(m10, m01) of the unblurred image over the disc around (x, y): rows v = -15...15, columns |u| <= UMAX[|v|]."""
    m10 = m01 = 0
    for v in range(-HALF, HALF + 1):
        for u in range(-UMAX[abs(v)], UMAX[abs(v)] + 1):
            p = int(img[y + v, x + u])
            m10 += u * p
            m01 += v * p
    return m10, m01


def direction_centroid(m10, m01):
    if m10 == 0 and m01 == 0:
        return Q, 0
    h = np.sqrt(np.float64(m10 * m10 + m01 * m01))            # (the argument is exact: < 2^53)
    return int(np.rint(np.float64(m10) * 16384.0 / h)), int(np.rint(np.float64(m01) * 16384.0 / h))


def direction_fixed(angle_deg):
    th = np.float64(angle_deg) * (np.pi / 180.0)
    return int(np.rint(16384.0 * np.cos(th))), int(np.rint(16384.0 * np.sin(th)))


def r14(v):
    """v / 16384 rounded half away from zero, on an int64 array"""
    return np.sign(v) * ((np.abs(v) + 8192) >> 14)


def offsets(pattern, A, B):
    """-> (dx1, dy1, dx2, dy2) int64 [256]: where the 256 pairs sample, relative to the keypoint."""
    p = np.asarray(pattern).astype(np.int64)
    x1, y1, x2, y2 = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    return r14(x1 * A - y1 * B), r14(x1 * B + y1 * A), r14(x2 * A - y2 * B), r14(x2 * B + y2 * A)


def pack_bits(bits):
    """bool [256] -> uint8 [32]: bit i & 7 of byte i >> 3 is test i"""
    out = np.zeros(32, np.uint8)
    for i, b in enumerate(bits):
        if b:
            out[i >> 3] |= 1 << (i & 7)
    return out


def describe(img, xy, pattern, edge, centroid, angle_deg=-1.0, G=None):
    """-> dict of G uint8 [H, W], keep_idx int32 [m], moments int32 [m, 2], dir int32 [m, 2], desc uint8 [m, 32]."""
    img = np.asarray(img)
    H, W = img.shape
    if G is None:
        G = blur(img)
    keep = kept(xy, W, H, edge)
    pts = np.asarray(xy).reshape(-1, 2)
    mom, dirs, desc = np.zeros((len(keep), 2), np.int32), np.zeros((len(keep), 2), np.int32), np.zeros((len(keep), 32), np.uint8)
    fixed = direction_fixed(angle_deg)
    Gi = G.astype(np.int64)
    for k, i in enumerate(keep):
        x, y = int(pts[i, 0]), int(pts[i, 1])
        if centroid:
            mom[k] = moments(img, x, y)
            A, B = direction_centroid(int(mom[k, 0]), int(mom[k, 1]))
        else:
            A, B = fixed
        dirs[k] = A, B
        dx1, dy1, dx2, dy2 = offsets(pattern, A, B)
        desc[k] = pack_bits(Gi[y + dy1, x + dx1] < Gi[y + dy2, x + dx2])
    return dict(G=G, keep_idx=np.asarray(keep, np.int32), moments=mom, dir=dirs, desc=desc)


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def default_pattern():
    """int8 [256, 4]: candidate row r takes values 4r ... 4r + 3 of the splitmix64 stream of PATTERN_SEED (value i = mix(seed +
    (i + 1) golden)), each mapped to -15 ... 15 by ((z >> 32) * 31) >> 32; rows whose two points coincide are skipped."""
    rows, r = [], 0
    while len(rows) < 256:
        c = [((_mix((PATTERN_SEED + (4 * r + k + 1) * GOLDEN) & MASK64) >> 32) * 31 >> 32) - HALF for k in range(4)]
        r += 1
        if (c[0], c[1]) != (c[2], c[3]):
            rows.append(c)
    return np.asarray(rows, np.int8)


def umax_opencv():
    """The table as OpenCV's ORB builds it for a patch of 31: cvRound(sqrt(225 - v^2)) up to v = 11, then the fix-up that makes
    the disc symmetric under the exchange of u and v."""
    hp = HALF
    umax = [0] * (hp + 2)
    vmax = math.floor(hp * math.sqrt(2.0) / 2 + 1)
    vmin = math.ceil(hp * math.sqrt(2.0) / 2)
    for v in range(vmax + 1):
        umax[v] = int(np.rint(math.sqrt(hp * hp - v * v)))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return tuple(umax[:hp + 1])
