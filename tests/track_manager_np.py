"""Plain-Python restatement of the track manager, written for clarity, not speed:

  nearly_equal / feat_eq   Feature::operator== (feature.cpp:47-68): a relative test at machine epsilon
  TileGridNp               TiledImage::setTileForFeature (tiled_image.cpp:139-158)
  normalize                Camera::normalize(track, max_size): the newest max_size observations, (u - cx) / fx, (v - cy) / fy
  baseline_delta / check_baseline / baseline_batch
                           TrackManager::checkBaseline (track_manager.cpp:576-636), in Python floats in the order of operations of
                           csrc/xk_tracks.hip.h; baseline_batch has the interface of xk_trk_baseline
  TrackManagerNp           TrackManager::manageTracks (:115-432) with a quadratic scan and lists; it counts the branches it takes
  facet                    featureTriangleAtPoint by the project's definition, in exact rationals

A feature is a Feat (undistorted pixels x, y; distorted pixels xd, yd; FAST score; tile), a track a Trk (a list of Feat with an
id), a normalised track an NTrk (a list of (x, y) with the same id), a match a [previous, current] pair of Feat."""
import collections
import itertools
import math
import struct
import sys
from fractions import Fraction

EPS = sys.float_info.epsilon
TINY = sys.float_info.min
HUGE = sys.float_info.max


class Feat:
    __slots__ = ("x", "y", "xd", "yd", "score", "row", "col")

    def __init__(self, x, y, xd=None, yd=None, score=0.0):
        self.x, self.y = float(x), float(y)
        self.xd, self.yd = float(x if xd is None else xd), float(y if yd is None else yd)
        self.score, self.row, self.col = float(score), 0, 0

    def copy(self):
        f = Feat(self.x, self.y, self.xd, self.yd, self.score)
        f.row, f.col = self.row, self.col
        return f


class Trk(list):
    id = 0

    def clone(self):
        t = Trk(self)          # features are never modified after they enter a track, but for their tile
        t.id = self.id
        return t


class NTrk(list):
    id = 0


def nearly_equal(a, b):
    """feature.cpp:51-68."""
    if a == b:
        return True
    abs_a, abs_b, diff = abs(a), abs(b), abs(a - b)
    if a == 0 or b == 0 or abs_a + abs_b < TINY:
        return diff < EPS * TINY
    return diff / min(abs_a + abs_b, HUGE) < EPS


def feat_eq(f, g):
    return nearly_equal(f.x, g.x) and nearly_equal(f.y, g.y)


class TileGridNp:
    def __init__(self, width, height, n_tiles_h, n_tiles_w):
        self.rows, self.n_tiles_h, self.n_tiles_w = height, n_tiles_h, n_tiles_w
        self.tile_height, self.tile_width = height / n_tiles_h, width / n_tiles_w

    def set_tile(self, f):
        c, col = f.xd - self.tile_width - 0.5, 0
        while c > 0:
            col += 1
            c -= self.tile_width
        r, row = self.rows - f.yd - 0.5, self.n_tiles_h - 1
        while r > self.tile_height:
            row -= 1
            r -= self.tile_height
        f.row, f.col = row, col


def normalize(trk, K, max_size=0):
    """Camera::normalize(track, max_size): K = (fx, fy, cx, cy) in pixels."""
    fx, fy, cx, cy = K
    skip = len(trk) - max_size if max_size and len(trk) > max_size else 0
    out = NTrk(((f.x - cx) / fx, (f.y - cy) / fy) for f in trk[skip:])
    out.id = trk.id
    return out


def _qmul(a, b):
    """Hamilton product of (w, x, y, z) quaternions, every operation rounded once, left to right."""
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
            a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])


def _qnorm(q_xyzw):
    x, y, z, w = (float(v) for v in q_xyzw)
    n2 = x * x + y * y + z * z + w * w
    n = math.sqrt(n2) if n2 > 0.0 else 1.0
    return (w / n, x / n, y / n, z / n)


def _div(a, b):
    """IEEE division: Python raises on a zero divisor."""
    if b == 0.0 and not math.isnan(a):
        if a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b if b != 0.0 else math.nan


def baseline_delta(ntrk, quats):
    """(delta_x, delta_y) of a normalised track of n >= 2 observations against the attitude list quats ([m][4] xyzw, m >= n):
    the reference's loop with its `if ... else if`, literally."""
    n_quats, n_obs = len(quats), len(ntrk)
    assert n_obs > 1 and n_quats >= n_obs
    i_last = n_quats - 1
    i_first = i_last - n_obs + 1
    min_x = max_x = ntrk[-1][0]
    min_y = max_y = ntrk[-1][1]
    cn = _qnorm(quats[i_last])
    for i in range(i_first, i_last + 1):
        ci = _qnorm(quats[i])
        q = _qmul((ci[0], -ci[1], -ci[2], -ci[3]), cn)
        x, y = ntrk[i - i_first]
        r = _qmul(_qmul((q[0], -q[1], -q[2], -q[3]), (0.0, x, y, 1.0)), q)
        fx, fy = _div(r[1], r[3]), _div(r[2], r[3])
        if fx < min_x:
            min_x = fx
        elif fx > max_x:
            max_x = fx
        if fy < min_y:
            min_y = fy
        elif fy > max_y:
            max_y = fy
    return max_x - min_x, max_y - min_y


def check_baseline(ntrk, quats, min_x, min_y):
    dx, dy = baseline_delta(ntrk, quats)
    return dx > min_x or dy > min_y


def baseline_batch(tracks_px, drop_last, quats, K, min_x, min_y):
    """xk_trk_baseline: tracks_px = lists of (u, v) undistorted pixels -> (norm_off, norm_xy rows, delta rows, flags)."""
    norm_off, norm_xy, delta, flag = [0], [], [], []
    for trk, drop in zip(tracks_px, drop_last):
        ql = quats[:len(quats) - int(drop)]
        t = Trk(Feat(u, v) for u, v in trk)
        n = normalize(t, K, len(ql))
        norm_xy.extend(n)
        norm_off.append(len(norm_xy))
        d = baseline_delta(n, ql)
        delta.append(d)
        flag.append(1 if (d[0] > min_x or d[1] > min_y) else 0)
    return norm_off, norm_xy, delta, flag


class TrackManagerNp:
    def __init__(self, K, min_baseline_x_n, min_baseline_y_n, multi_uav=False):
        self.K, self.min_x, self.min_y, self.multi_uav = K, min_baseline_x_n, min_baseline_y_n, multi_uav
        self.opp_ids = None                     # the caller's list (setOppUpgradesMSCKF): consumed and cleared by manage
        self.next_id = 1
        self.branches = collections.Counter()
        self.margins = []                       # |delta - threshold| of every baseline decision, for the case generator
        self.clear()
        self.new_slam_std_n, self.new_slam_msckf_n = [], []

    def clear(self):
        self.slam, self.new_slam, self.lost, self.opp, self.msckf_n, self.msckf_short_n = [], [], [], [], [], []

    def _baseline(self, ntrk, quats):
        dx, dy = baseline_delta(ntrk, quats)
        # the deciding axis: x when it passes (the `||` stops there), else y decides
        self.margins.append(abs(dx - self.min_x) if dx > self.min_x else min(abs(dx - self.min_x), abs(dy - self.min_y)))
        return dx > self.min_x or dy > self.min_y

    def manage(self, matches, cam_rots, n_poses_max, n_slam_max, min_track_length, grid):
        assert n_poses_max >= 3
        B, K = self.branches, self.K
        self.slam.extend(self.new_slam)
        self.new_slam = []
        n_bins = grid.n_tiles_h * grid.n_tiles_w
        bin_idx = [[] for _ in range(n_bins)]
        bin_idx_per = [[] for _ in range(n_bins)]
        bin_max = 0
        t, lost_count = 0, 0
        self.lost = []
        while t < len(self.slam):
            found = False
            for m in range(len(matches)):
                if feat_eq(self.slam[t][-1], matches[m][0]):
                    found = True
                    cur = matches[m][1]
                    grid.set_tile(cur)
                    b = cur.row * grid.n_tiles_w + cur.col
                    bin_idx[b].append(t)
                    bin_idx_per[b].append(t + lost_count)
                    if len(bin_idx[b]) > len(bin_idx[bin_max]):
                        bin_max = b
                    self.slam[t].append(cur)
                    del matches[m]
                    B["slam_extended"] += 1
                    break
            if not found:
                self.lost.append(t + lost_count)      # its index before this frame's deletions
                del self.slam[t]
                lost_count += 1
                B["slam_lost"] += 1
                continue
            t += 1
        if lost_count >= 2:
            B["slam_lost_two_in_a_frame"] += 1

        self.msckf_n, self.msckf_short_n = [], []
        prev_opp, self.opp = self.opp, []
        for prev, cur in matches:
            for t in range(len(prev_opp)):
                if feat_eq(prev_opp[t][-1], prev):
                    prev_opp[t].append(cur)
                    self.opp.append(prev_opp.pop(t))
                    B["opp_extended"] += 1
                    break
            else:
                trk = Trk([prev, cur])
                trk.id = self.next_id
                self.next_id += 1
                self.opp.append(trk)
                B["opp_new"] += 1

        rots_short = cam_rots[:-1]
        if self.multi_uav:
            for dead in prev_opp:
                if len(dead) < 3:
                    B["multi_dead_too_short"] += 1
                    continue
                for o in range(len(self.opp_ids)):
                    if dead.id == self.opp_ids[o]:
                        self.msckf_short_n.append(normalize(dead, K, len(cam_rots)))
                        del self.opp_ids[o]
                        B["multi_dead_matched"] += 1
                        break
                else:
                    B["multi_dead_unmatched"] += 1
        else:
            for dead in prev_opp:
                if len(dead) < 2:
                    continue
                n = normalize(dead, K, len(rots_short))
                if self._baseline(n, rots_short):
                    self.msckf_short_n.append(n)
                    B["dead_short_pass"] += 1
                else:
                    B["dead_short_fail"] += 1

        lengths = [len(t) for t in self.opp]
        self.opp.sort(key=len, reverse=True)             # list.sort is stable, as the mirror's std::stable_sort
        if any(a == b for a, b in zip(lengths, lengths[1:])) and lengths != [len(t) for t in self.opp]:
            B["sort_moved_past_equal_lengths"] += 1
        t = 0
        while t < len(self.opp):
            trk = self.opp[t]
            grid.set_tile(trk[-1])
            b = trk[-1].row * grid.n_tiles_w + trk[-1].col
            if len(trk) > min_track_length - 1:
                if len(self.slam) + len(self.new_slam) < n_slam_max:
                    self.new_slam.append(self.opp.pop(t))
                    bin_idx[b].append(len(self.slam) + len(self.new_slam) - 1)
                    if len(bin_idx[b]) > len(bin_idx[bin_max]):
                        bin_max = b
                    B["promote_free_slot"] += 1
                elif len(bin_idx[bin_max]) > len(bin_idx[b]) + 1:
                    gone = bin_idx[bin_max][-1]
                    if gone >= len(self.slam):
                        del self.new_slam[gone - len(self.slam)]
                        B["evict_new"] += 1
                    else:
                        self.lost.append(bin_idx_per[bin_max].pop())
                        del self.slam[gone]
                        B["evict_existing"] += 1
                    for lst in bin_idx:
                        for j in range(len(lst)):
                            if lst[j] > gone:
                                lst[j] -= 1
                    bin_idx[bin_max].pop()
                    self.new_slam.append(self.opp.pop(t))
                    bin_idx[b].append(len(self.slam) + len(self.new_slam) - 1)
                    for i in range(n_bins):
                        if len(bin_idx[i]) > len(bin_idx[bin_max]):
                            bin_max = i
                else:
                    if len(bin_idx[bin_max]) == len(bin_idx[b]) + 1:
                        B["no_evict_at_difference_one"] += 1
                    if len(trk) > n_poses_max - 1:
                        n = normalize(trk, K, len(cam_rots))
                        if self._baseline(n, cam_rots):
                            self.msckf_n.append(n)
                            B["overlong_pass"] += 1
                        else:
                            B["overlong_fail"] += 1
                        del self.opp[t]
                    else:
                        B["long_enough_waits"] += 1
                        t += 1
            else:
                B["too_short_waits"] += 1
                t += 1
        if self.multi_uav:
            del self.opp_ids[:]

        self.new_slam_std_n, self.new_slam_msckf_n = [], []
        std, msckf = [], []
        for trk in self.new_slam:
            n = normalize(trk, K, len(cam_rots))
            if self._baseline(n, cam_rots):
                self.new_slam_msckf_n.append(n)
                msckf.append(trk)
                B["new_slam_msckf"] += 1
            else:
                self.new_slam_std_n.append(n)
                std.append(trk)
                B["new_slam_std"] += 1
        if msckf and std and self.new_slam != msckf + std:
            B["new_slam_reordered"] += 1
        self.new_slam = msckf + std

    def normalize_slam_tracks(self, size_out):
        return [normalize(t, self.K, size_out) for t in self.slam]

    def get_opp_tracks(self):
        return [normalize(t, self.K, len(self.opp)) for t in self.opp]       # (the reference passes the LIST's size, :60)

    def most_promising(self, k):
        return sorted(self.slam, key=lambda t: -t[-1].score)[:k]


# ---- featureTriangleAtPoint -----------------------------------------------------------------------------------------
def f32(v):
    """The value rounded to float, as cv::Subdiv2D stores it (a Python float that a float holds exactly)."""
    return struct.unpack("f", struct.pack("f", v))[0]


def orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def in_circle(a, b, c, d):
    """> 0 iff d is strictly inside the circle through a, b, c taken counter-clockwise."""
    r = [(p[0] - d[0], p[1] - d[1]) for p in (a, b, c)]
    r = [(x, y, x * x + y * y) for x, y in r]
    return (r[0][0] * (r[1][1] * r[2][2] - r[1][2] * r[2][1]) - r[0][1] * (r[1][0] * r[2][2] - r[1][2] * r[2][0]) +
            r[0][2] * (r[1][0] * r[2][1] - r[1][1] * r[2][0]))


def facet_points(slam_xy_dist, width, height):
    """The point set as exact rationals: the tracks' newest distorted pixels as floats, then the three outer vertices."""
    big = 3 * max(width + 2, height + 2)
    pts = [(Fraction(f32(x)), Fraction(f32(y))) for x, y in slam_xy_dist]
    return pts + [(Fraction(-1 + big), Fraction(-1)), (Fraction(-1), Fraction(-1 + big)), (Fraction(-1 - big), Fraction(-1 - big))]


def facet(slam_xy_dist, point, width, height, dets=None):
    """The three SLAM indices of the Delaunay triangle around `point`, ascending, or [].  dets (a list): every determinant
    evaluated, with its scale, for the general-position check of the case generator."""
    n = len(slam_xy_dist)
    px, py = f32(point[0]), f32(point[1])
    if n < 3 or not (-1 <= px < width + 1 and -1 <= py < height + 1):
        return []
    pts = facet_points(slam_xy_dist, width, height)
    p = (Fraction(px), Fraction(py))

    def note(v, *qs):
        if dets is not None:
            span = max(max(abs(q[0] - r[0]), abs(q[1] - r[1])) for q in qs for r in qs)
            dets.append((v, span, len(qs)))
        return v

    for i, j, k in itertools.combinations(range(n + 3), 3):
        a, b, c = pts[i], pts[j], pts[k]
        o = note(orient(a, b, c), a, b, c)
        if o == 0:
            continue
        if o < 0:
            b, c = c, b
        if note(orient(a, b, p), a, b, p) < 0 or note(orient(b, c, p), b, c, p) < 0 or note(orient(c, a, p), c, a, p) < 0:
            continue
        if any(note(in_circle(a, b, c, pts[l]), a, b, c, pts[l]) > 0 for l in range(n + 3) if l not in (i, j, k)):
            continue
        return [i, j, k] if k < n else []      # combinations come in lexicographic order: the first is the smallest
    return []
