"""Inputs of the track manager's tests: batches for xk_trk_baseline, the scripted sequence for manageTracks and the
point sets of the facet search.  Every generator ASSERTS that no decision of its case hinges on rounding: baseline extents stay
more than 1e-9 from their threshold, the facet determinants at least 1e-6 of their scale from zero (in exact rationals)."""
import math
from fractions import Fraction

import numpy as np

import track_manager_np as tm

WIDTH, HEIGHT = 640, 480
CAM_FRACTIONS = (0.625, 0.75, 0.5, 0.5)                   # fx, fy, cx, cy over the image size, as x::Camera takes them
K = (CAM_FRACTIONS[0] * WIDTH, CAM_FRACTIONS[1] * HEIGHT, CAM_FRACTIONS[2] * WIDTH, CAM_FRACTIONS[3] * HEIGHT)
MIN_BASELINE = (0.05, 0.05)
BASELINE_MARGIN = 1e-9


def quat_about(axis, angle):
    """(x, y, z, w) of a rotation by angle about a unit axis."""
    s = math.sin(angle / 2)
    return [axis[0] * s, axis[1] * s, axis[2] * s, math.cos(angle / 2)]


def attitude_list(rng, n, max_angle_deg=30.0, scale=1.0):
    """n attitudes on a smooth arc of at most max_angle_deg between first and last, not normalised exactly (scale)."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    total = math.radians(max_angle_deg) * rng.uniform(0.3, 1.0)
    start = quat_about((0.0, 0.0, 1.0), rng.uniform(-0.2, 0.2))
    out = []
    for i in range(n):
        a = quat_about(axis, total * i / max(n - 1, 1))
        # start then the arc (x, y, z, w): plain Hamilton product
        w = tm._qmul((a[3], a[0], a[1], a[2]), (start[3], start[0], start[1], start[2]))
        out.append([scale * w[1], scale * w[2], scale * w[3], scale * w[0]])
    return out


def pixel_track(rng, length):
    """Undistorted pixels of a feature that drifts across the image: normalised coordinates within +-0.45."""
    x0, y0 = rng.uniform(-0.3, 0.3, size=2)
    step = rng.uniform(-0.15, 0.15, size=2) / max(length, 8)
    jit = rng.normal(scale=2e-3, size=(length, 2))
    return [((x0 + step[0] * i + jit[i, 0]) * K[0] + K[2], (y0 + step[1] * i + jit[i, 1]) * K[1] + K[3]) for i in range(length)]


def _assert_margins(case):
    _, _, delta, flag = tm.baseline_batch(case["tracks"], case["drop_last"], case["quats"], K, *case["min_baseline"])
    for (dx, dy), f in zip(delta, flag):
        if not (math.isfinite(dx) and math.isfinite(dy)):
            continue
        deciding = abs(dx - case["min_baseline"][0]) if dx > case["min_baseline"][0] else \
            min(abs(dx - case["min_baseline"][0]), abs(dy - case["min_baseline"][1]))
        assert deciding > BASELINE_MARGIN, (dx, dy)
    return case


def baseline_cases():
    """name -> dict(tracks, drop_last, quats, min_baseline).  The smallest shapes at which the kernel can go wrong."""
    rng = np.random.default_rng(20260116)
    cases = {}

    def case(name, lengths, drops, n_quats, min_baseline=MIN_BASELINE, angle=30.0, scale=1.0):
        cases[name] = _assert_margins(dict(tracks=[pixel_track(rng, n) for n in lengths], drop_last=list(drops),
                                           quats=attitude_list(rng, n_quats, angle, scale), min_baseline=min_baseline))

    case("one_track", [4], [0], 6)
    lengths = [int(v) for v in rng.integers(2, 41, size=300)]
    lengths[:6] = [2, 30, 29, 31, 40, 3]                              # two observations, exactly n_quats, n_quats - 1, longer: cropped
    drops = [int(v) for v in rng.integers(0, 2, size=300)]
    drops[:6] = [1, 0, 1, 1, 0, 0]
    case("k300_mixed", lengths, drops, 30, min_baseline=(0.02, 0.03), scale=1.7)
    case("full_wave", [64, 64, 70, 2, 63, 65], [0, 1, 0, 1, 1, 1], 64)
    case("two_quats", [2, 3, 9, 2, 5], [0, 0, 0, 0, 0], 2, min_baseline=(0.004, 0.004))
    case("drop_to_two", [2, 7], [1, 1], 3, min_baseline=(0.004, 0.004))
    # special values: a NaN observation in the middle of a track; a ray whose rotated z is exactly zero (a quarter turn about y
    # against an identity last pose, on a feature at the principal point's column), which gives an infinite extent
    q = [[0.0, 1.0, 0.0, 1.0], [0.0, 0.1, 0.0, 1.0], [0.0, 0.05, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0]]
    nan_trk = pixel_track(rng, 4)
    nan_trk[1] = (float("nan"), nan_trk[1][1])
    zero_z = [(K[2], K[3] + 36.0)] + pixel_track(rng, 3)
    nan_last = pixel_track(rng, 3)
    nan_last[2] = (nan_last[2][0], float("nan"))
    cases["special_values"] = _assert_margins(dict(tracks=[nan_trk, zero_z, pixel_track(rng, 4), nan_last], drop_last=[0, 0, 0, 1], quats=q,
                                                   min_baseline=MIN_BASELINE))
    return cases


# ---- the scripted sequence ------------------------------------------------------------------------------------------------------
SEQ = dict(n_poses_max=6, n_slam_max=4, min_track_length=3, tiles=(2, 2), n_frames=20)


def sequence(multi_uav=False):
    """A camera moving along x with a slow yaw over 24 landmarks, 20 frames, with scripted dropouts.  -> list of frames, each a
    dict(matches = [[previous Feat, current Feat]] in descending FAST order, cam_rots [n_poses_max][4], point (the facet query),
    opp_ids (multi_uav: the ids the caller upgrades this frame))."""
    rng = np.random.default_rng(7)
    n_lm, n_frames, N = 24, SEQ["n_frames"], SEQ["n_poses_max"]
    # 14 landmarks in the upper-left quarter of the view, the rest spread: the tiles fill unevenly, which is what evicts
    lm = []
    for i in range(n_lm):
        depth = 3.0 + 2.0 * (i % 3) if i % 4 else 60.0 + i         # every fourth one is far: its baseline fails
        if i < 14:
            xn, yn = rng.uniform(-0.55, -0.1), rng.uniform(-0.45, -0.05)
        else:
            xn, yn = rng.uniform(-0.5, 0.6), rng.uniform(-0.45, 0.45)
        lm.append((xn * depth + 0.6, yn * depth, depth))
    score = [float(200 - 3 * i + (i * 7) % 5) for i in range(n_lm)]
    # dropouts: landmark -> the frames at which the tracker loses it (it is detected again one frame later)
    drop = {l: set() for l in range(n_lm)}
    for l in range(n_lm):
        for f in range(2, n_frames):
            if rng.uniform() < 0.09:
                drop[l].add(f)
    drop[0] |= {6}; drop[1] |= {6}                                  # two persistent features lost in one frame
    first_seen = [0 if l < 18 else 2 + (l - 18) for l in range(n_lm)]

    yaw = [0.012 * f for f in range(n_frames)]
    pos = [(0.12 * f, 0.01 * f, 0.0) for f in range(n_frames)]
    quats = [quat_about((0.0, 1.0, 0.0), yaw[f]) for f in range(n_frames)]     # the sign checkBaseline's de-rotation undoes

    def project(l, f):
        c, s = math.cos(yaw[f]), math.sin(yaw[f])
        dx, dy, dz = lm[l][0] - pos[f][0], lm[l][1] - pos[f][1], lm[l][2] - pos[f][2]
        x, y, z = c * dx - s * dz, dy, s * dx + c * dz
        u, v = x / z * K[0] + K[2], y / z * K[1] + K[3]
        return tm.Feat(u, v, u, v, score[l])

    def visible(l, f):
        if f < first_seen[l] or f in drop[l]:
            return False
        p = project(l, f)
        return 1.0 < p.x < WIDTH - 1.0 and 1.0 < p.y < HEIGHT - 1.0

    frames = []
    for f in range(1, n_frames):
        both = [l for l in range(n_lm) if visible(l, f - 1) and visible(l, f)]
        both.sort(key=lambda l: -score[l])
        rots = [quats[max(0, g)] for g in range(f - N + 1, f + 1)]
        matches = [[project(l, f - 1), project(l, f)] for l in both]
        for i, (prev, _) in enumerate(matches):                    # the association is nearlyEqual, not bit equality: every third
            if i % 3 == 1:                                         # previous feature arrives one ulp off what the track holds
                prev.x = math.nextafter(prev.x, math.inf if i % 2 else -math.inf)
                prev.y = math.nextafter(prev.y, -math.inf)
        frame = dict(matches=matches, cam_rots=rots,
                     point=(WIDTH * (0.3 + 0.02 * (f % 5)), HEIGHT * (0.35 + 0.03 * (f % 3))), opp_ids=[])
        frames.append(frame)
    return frames


def run_sequence(multi_uav=False, frames=None, on_frame=None):
    """The restatement over the sequence -> the manager (its branch counts and margins).  multi_uav: every frame the caller
    upgrades the ids of the two oldest opportunistic tracks of the frame before, one of which may have died."""
    frames = sequence(multi_uav) if frames is None else frames
    mgr = tm.TrackManagerNp(K, MIN_BASELINE[0], MIN_BASELINE[1], multi_uav)
    grid = tm.TileGridNp(WIDTH, HEIGHT, *SEQ["tiles"])
    for i, fr in enumerate(frames):
        if multi_uav:
            fr["opp_ids"] = sorted(t.id for t in mgr.opp)[:6]
            mgr.opp_ids = list(fr["opp_ids"])
        mgr.manage([[p.copy(), c.copy()] for p, c in fr["matches"]], fr["cam_rots"], SEQ["n_poses_max"], SEQ["n_slam_max"],
                   SEQ["min_track_length"], grid)
        if on_frame:
            on_frame(i, fr, mgr)
    assert min(mgr.margins) > BASELINE_MARGIN, min(mgr.margins)
    return mgr


# ---- facets -----------------------------------------------------------------------------------------------------------------------
def assert_general_position(points, query, width, height):
    """Every orientation and in-circle determinant the search evaluates is non-zero, and at least 1e-6 of its scale: span^2
    for an orientation (3 points), span^4 for an in-circle test (4 points)."""
    dets = []
    out = tm.facet(points, query, width, height, dets)
    for v, span, n in dets:
        assert v != 0 and abs(v) >= Fraction(1, 10**6) * span ** (2 if n == 3 else 4), (float(v), float(span), n)
    return out


def facet_cases():
    """name -> dict(points [n][2] distorted pixels, query, expect)."""
    rng = np.random.default_rng(11)
    cases = {}

    def case(name, pts, query, expect=None):
        got = assert_general_position(pts, query, WIDTH, HEIGHT)
        if expect is not None:
            assert got == expect, (name, got, expect)
        cases[name] = dict(points=[tuple(p) for p in pts], query=tuple(query), expect=got)

    tri = [(100.25, 80.5), (500.75, 120.125), (310.5, 400.0)]
    case("one_triangle", tri, (300.0, 200.0), [0, 1, 2])
    case("outside_hull", tri, (600.0, 450.0), [])
    # the query lies inside the hull of four points but in a triangle that reaches an outer vertex: none here, so a query just
    # beyond a hull edge, whose triangle is (edge, outer vertex)
    case("hull_triangle_outer_vertex", tri + [(320.0, 60.0)], (90.0, 300.0), [])
    case("outside_rectangle", tri, (-5.0, 10.0), [])
    case("two_tracks", tri[:2], (300.0, 200.0), [])
    pts12 = [(float(x), float(y)) for x, y in zip(rng.uniform(20, 620, 12), rng.uniform(20, 460, 12))]
    case("twelve_points", pts12, (331.7, 247.3))
    assert cases["twelve_points"]["expect"], "the query of the 12-point case must fall into an inner triangle"
    return cases
