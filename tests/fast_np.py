"""NumPy restatement of DESIGN 3.12: FAST 9-of-16 corner detection with OpenCV's cornerScore, non-maximum suppression, the
border test, the order by key and the greedy neighbourhood selection of Tracker::featureDetection; and of the tile
bookkeeping around it (TiledImage::setTileForFeature, Tracker::removeOverflowFeatures).

Written from the definition, brute force: sixteen arcs of nine per sign, an explicit painted mask.  It shares no structure
with csrc/xk_fast.hip.h (no bit masks, no sliding minima, no sort network, no chunks).  Every quantity is an integer: what the
device computes must equal this bit for bit.

segment_test is a second, independent corner predicate -- the literal "nine contiguous circle pixels all brighter than
I + t or all darker than I - t" -- that tests/test_fast_np.py holds against the score image."""
import numpy as np

CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
          (-2, 2), (-1, 3))


def _circle_values(img):
    """-> (centre [H-6, W-6], ring [16, H-6, W-6]) as int32: pixel (x, y) of the interior is at [y - 3, x - 3]."""
    I = np.asarray(img).astype(np.int32)
    H, W = I.shape
    ring = np.stack([I[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] for dx, dy in CIRCLE])
    return I[3:H - 3, 3:W - 3], ring


def score_image(img, threshold):
    """S uint8 [H, W]: s at corners (s >= threshold), 0 everywhere else."""
    H, W = np.asarray(img).shape
    c, ring = _circle_values(img)
    d = ring - c[None]
    best = np.full(c.shape, -1000, np.int32)
    for sign in (1, -1):
        for k in range(16):
            arc = np.stack([sign * d[(k + j) % 16] for j in range(9)]).min(axis=0)
            best = np.maximum(best, arc)
    s = best - 1
    S = np.zeros((H, W), np.uint8)
    S[3:H - 3, 3:W - 3] = np.where(s >= threshold, s, 0).astype(np.uint8)
    return S


def segment_test(img, threshold):
    """bool [H, W]: the literal segment test at `threshold`; False on the 3-pixel frame."""
    H, W = np.asarray(img).shape
    c, ring = _circle_values(img)
    brighter = ring > (c + threshold)[None]
    darker = ring < (c - threshold)[None]
    hit = np.zeros(c.shape, bool)
    for k in range(16):
        idx = [(k + j) % 16 for j in range(9)]
        hit |= brighter[idx].all(axis=0) | darker[idx].all(axis=0)
    out = np.zeros((H, W), bool)
    out[3:H - 3, 3:W - 3] = hit
    return out


def keypoints(S, non_max_supp):
    """bool [H, W]: corners, with non_max_supp those strictly greater than their eight neighbours."""
    S = np.asarray(S).astype(np.int32)
    H, W = S.shape
    kp = S > 0
    if non_max_supp:
        P = np.zeros((H + 2, W + 2), np.int32)
        P[1:-1, 1:-1] = S
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx or dy:
                    kp &= S > P[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
    return kp


def candidate_keys(S, non_max_supp, margin):
    """uint32, ascending: ((255 - S) << 24) | (y W + x) of every keypoint inside the border."""
    H, W = S.shape
    kp = keypoints(S, non_max_supp)
    y, x = np.nonzero(kp)
    inside = (x >= margin) & (x <= W - margin - 1) & (y >= margin) & (y <= H - margin - 1)
    x, y = x[inside].astype(np.int64), y[inside].astype(np.int64)
    keys = ((255 - S[y, x].astype(np.int64)) << 24) | (y * W + x)
    return np.sort(keys).astype(np.uint32)


def unpack(keys, W):
    """-> (x, y, score) of keys."""
    k = np.asarray(keys).astype(np.int64)
    pix = k & 0xFFFFFF
    return pix % W, pix // W, 255 - (k >> 24)


def round_half_away(v):
    return int(np.sign(v) * np.floor(abs(v) + 0.5))


def old_pixels(old_xy):
    """The rounded old features that block something: Python ints (no overflow); a non-finite point is dropped."""
    out = []
    for ox, oy in np.asarray(old_xy, np.float64).reshape(-1, 2):
        if np.isfinite(ox) and np.isfinite(oy):
            out.append((round_half_away(float(ox)), round_half_away(float(oy))))
    return out


def _paint(mask, x, y, b):
    H, W = mask.shape
    x0, x1, y0, y1 = max(x - b, 0), min(x + b, W - 1), max(y - b, 0), min(y + b, H - 1)
    if x0 <= x1 and y0 <= y1:
        mask[y0:y1 + 1, x0:x1 + 1] = 1


def select_painted(keys, W, H, b, old_xy=()):
    """The reference's painted mask with every box clipped to the image -> indices into keys of the accepted candidates."""
    mask = np.zeros((H, W), np.uint8)
    for ox, oy in old_pixels(old_xy):
        _paint(mask, ox, oy, b)
    xs, ys, _ = unpack(keys, W)
    acc = []
    for i, (x, y) in enumerate(zip(xs.tolist(), ys.tolist())):
        if mask[y, x] == 0:
            acc.append(i)
            _paint(mask, x, y, b)
    return np.asarray(acc, np.int64)


def select_chebyshev(keys, W, H, b, old_xy=()):
    """The same selection stated on distances: accepted iff no old feature and no earlier accepted one within b."""
    block = list(old_pixels(old_xy))
    xs, ys, _ = unpack(keys, W)
    acc = []
    for i, (x, y) in enumerate(zip(xs.tolist(), ys.tolist())):
        if all(max(abs(x - bx), abs(y - by)) > b for bx, by in block):
            acc.append(i)
            block.append((x, y))
    return np.asarray(acc, np.int64)


def detect(img, threshold=9, non_max_supp=1, block_half_length=20, margin=20, old_xy=()):
    """-> dict S, keys (all candidates, ascending), n_candidates, accepted (indices into keys), xy int32 [n, 2], score int32 [n]."""
    img = np.asarray(img)
    H, W = img.shape
    S = score_image(img, threshold)
    keys = candidate_keys(S, non_max_supp, margin)
    acc = select_painted(keys, W, H, block_half_length, old_xy)
    x, y, s = unpack(keys[acc], W)
    return dict(S=S, keys=keys, n_candidates=len(keys), accepted=acc, xy=np.stack([x, y], axis=1).astype(np.int32).reshape(-1, 2),
                score=s.astype(np.int32))


class TileGrid:
    """TiledImage's tile parameters and counts (tiled_image.cpp:98-158): the fp64 subtraction loops as written."""

    def __init__(self, width, height, n_tiles_h, n_tiles_w, max_feat_per_tile):
        self.width, self.height, self.n_tiles_h, self.n_tiles_w = int(width), int(height), int(n_tiles_h), int(n_tiles_w)
        self.max_feat_per_tile = int(max_feat_per_tile)
        self.tile_height = float(height) / n_tiles_h
        self.tile_width = float(width) / n_tiles_w
        self.counts = np.zeros((self.n_tiles_h, self.n_tiles_w), np.int64)

    def tile(self, x_dist, y_dist):
        """setTileForFeature -> (row, col)."""
        c = float(x_dist) - self.tile_width - 0.5
        col = 0
        while c > 0:
            col += 1
            c -= self.tile_width
        r = self.height - float(y_dist) - 0.5
        row = self.n_tiles_h - 1
        while r > self.tile_height:
            row -= 1
            r -= self.tile_height
        return row, col

    def reset(self):
        self.counts[:] = 0

    def increment(self, row, col):
        if 0 <= row < self.n_tiles_h and 0 <= col < self.n_tiles_w:      # (a tile outside the grid is not counted)
            self.counts[row, col] += 1

    def count(self, row, col):
        return int(self.counts[row, col]) if 0 <= row < self.n_tiles_h and 0 <= col < self.n_tiles_w else 0


def remove_overflow(grid, prev_xy, cur_xy):
    """Tracker::removeOverflowFeatures (tracker.cpp:592-620) with its quirks: both loops run on i - 1, the second starts at
    size - 1, so the last pair is never examined; the counts are those of the current list's tiles and stay as counted while
    pairs are erased.  -> (indices of the pairs that stay, tiles of the previous list, tiles of the current list)."""
    n = len(cur_xy)
    grid.reset()
    tiles_prev, tiles_cur = [None] * n, [None] * n
    for i in range(n, 0, -1):
        tiles_prev[i - 1] = grid.tile(*prev_xy[i - 1])
        tiles_cur[i - 1] = grid.tile(*cur_xy[i - 1])
        grid.increment(*tiles_cur[i - 1])
    keep = list(range(n))
    for i in range(n - 1, 0, -1):
        if grid.count(*tiles_cur[i - 1]) > grid.max_feat_per_tile:
            del keep[i - 1]
    return keep, tiles_prev, tiles_cur
