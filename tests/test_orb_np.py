"""The restatement tests/orb_np.py and the scenes of tests/orb_cases.py, without a GPU: the blur against its direct 2-D
definition, the disc table against OpenCV's construction, the equivariance of blur, moments and descriptors under quarter turns
and a mirror (what catches an x / y or sign slip that the device and the restatement could share), the conditions the scenes
state, and the default pattern."""
import numpy as np
import pytest

import orb_cases as oc
import orb_np as onp

DEFAULT_HEAD = [[-2, -15, 7, -14], [13, 12, -10, 9], [9, 11, 9, -14]]      # the first rows of the default pattern, as first drawn


def test_blur_equals_the_direct_definition():
    rng = np.random.default_rng(3)
    strided = oc.strided_image()
    assert strided.shape == (121, 176) or strided.strides[0] == 176
    for im in (rng.integers(0, 256, (16, 16), dtype=np.uint8), rng.integers(0, 256, (17, 33), dtype=np.uint8), strided[:, :161]):
        assert np.array_equal(onp.blur(im), onp.blur_direct(im)), im.shape
    for c in (0, 1, 77, 255):                                     # the taps sum to 256 and the rounding is exact on a constant
        assert np.all(onp.blur(np.full((16, 21), c, np.uint8)) == c)
    assert sum(onp.TAPS) == 256
    imp = np.zeros((33, 17), np.uint8)
    imp[20, 8] = 255
    want = (255 * np.outer(onp.TAPS, onp.TAPS) + 32768) >> 16
    G = onp.blur(imp)
    assert np.array_equal(G[17:24, 5:12], want) and G.sum() == want.sum()
    # the border reflects without repeating the edge pixel: an impulse in column 1 comes back through column -1 -> 1
    imp = np.zeros((16, 16), np.uint8)
    imp[8, 1] = 255
    G = onp.blur(imp)
    assert G[8, 0] == (255 * 54 * (49 + 49) + 32768) >> 16        # column 0 sees column 1 twice: at +1 and at -1 -> 1
    assert G[8, 1] == (255 * 54 * (54 + 34) + 32768) >> 16        # column 1: itself, and at -2 -> -1 -> 1
    assert G[8, 2] == (255 * 54 * (49 + 18) + 32768) >> 16        # column 2: at -1, and at -3 -> -1 -> 1
    assert G[8, 3] == (255 * 54 * 34 + 32768) >> 16               # column 3: at -2 only; column 0 is not repeated


def test_umax_is_opencvs_construction():
    assert onp.umax_opencv() == onp.UMAX
    # the disc is symmetric under the exchange of u and v, which is what makes the moments turn with the image
    disc = {(u, v) for v in range(-15, 16) for u in range(-onp.UMAX[abs(v)], onp.UMAX[abs(v)] + 1)}
    assert disc == {(v, u) for u, v in disc} and len(disc) == sum(2 * u + 1 for u in onp.UMAX) * 2 - 31


def _turned(im, pts, q):
    """The image after q quarter turns of np.rot90 and the keypoints (x, y) -> (y, W - 1 - x) per turn."""
    pts = np.asarray(pts, np.int64)
    for _ in range(q):
        W = im.shape[1]
        im, pts = np.rot90(im), np.stack([pts[:, 1], W - 1 - pts[:, 0]], axis=1)
    return np.ascontiguousarray(im), pts


@pytest.mark.parametrize("pattern", ["default", "corners"])
def test_equivariance_under_quarter_turns_and_a_mirror(pattern):
    im = np.asarray(oc.rects_image())
    H, W = im.shape
    edge = 25
    pat = onp.default_pattern() if pattern == "default" else oc.corner_pattern()
    rng = np.random.default_rng(9)
    pts = np.stack([rng.integers(edge, W - edge, 30), rng.integers(edge, H - edge, 30)], axis=1)
    G0 = onp.blur(im)
    ref_c = onp.describe(im, pts, pat, edge, 1)
    assert len(ref_c["keep_idx"]) == 30 and len({d.tobytes() for d in ref_c["desc"]}) > 20
    for q in range(4):
        imq, ptq = _turned(im, pts, q)
        assert np.array_equal(onp.blur(imq), np.rot90(G0, q)), q
        got = onp.describe(imq, ptq, pat, edge, 1)
        m = ref_c["moments"].astype(np.int64)
        for _ in range(q):
            m = np.stack([m[:, 1], -m[:, 0]], axis=1)             # (m10, m01) -> (m01, -m10) per turn
        assert np.array_equal(got["moments"], m), q
        assert np.array_equal(got["desc"], ref_c["desc"]), q
        for th in (-1.0, 37.0):                                   # fixed mode: the angle turns with the image
            a = onp.describe(im, pts, pat, edge, 0, th)
            b = onp.describe(imq, ptq, pat, edge, 0, th - 90.0 * q)
            assert np.array_equal(a["desc"], b["desc"]), (q, th)
    # the mirror x -> W - 1 - x: the blur and m01 stay, m10 changes sign, and the descriptors are those of the pattern with y negated
    imm = np.ascontiguousarray(im[:, ::-1])
    ptm = np.stack([W - 1 - pts[:, 0], pts[:, 1]], axis=1)
    patm = pat * np.array([1, -1, 1, -1], np.int8)
    assert np.array_equal(onp.blur(imm), G0[:, ::-1])
    got = onp.describe(imm, ptm, patm, edge, 1)
    assert np.array_equal(got["moments"], ref_c["moments"] * np.array([-1, 1]))
    assert np.array_equal(got["desc"], ref_c["desc"])
    assert np.array_equal(onp.describe(imm, ptm, patm, edge, 0, 180.0 - 37.0)["desc"], onp.describe(im, pts, pat, edge, 0, 37.0)["desc"])
    # and the map is not trivially invariant: an unturned pattern on the turned image gives other bits
    imq, ptq = _turned(im, pts, 1)
    assert not np.array_equal(onp.describe(imq, ptq, pat, edge, 0, 37.0)["desc"], onp.describe(im, pts, pat, edge, 0, 37.0)["desc"])


@pytest.mark.parametrize("name", oc.GPU_SCENES)
def test_scene_conditions(name):
    sc = oc.SCENES[name]
    im, pts, r = oc.pixels(name), oc.points(name), oc.restated(name)
    H, W = im.shape
    e = sc["edge"]
    n_kept = len(r["keep_idx"])
    assert n_kept == sc["n_kept"] and 1 <= n_kept < len(pts)                       # keeps at least one, drops at least one
    assert np.all(np.diff(r["keep_idx"]) > 0)
    xs, ys = pts[:, 0].tolist(), pts[:, 1].tolist()
    assert e - 1 in xs and W - e in xs and e - 1 in ys and H - e in ys and min(xs) < 0 and max(ys) > H
    if n_kept >= 5:
        assert e in xs and W - e - 1 in xs and e in ys and H - e - 1 in ys
        assert len({tuple(p) for p in pts[r["keep_idx"]].tolist()}) < n_kept          # a duplicate among the kept
        k = pts[r["keep_idx"]]
        first = {}
        for row, p in enumerate(k.tolist()):
            j = first.setdefault(tuple(p), row)
            assert np.array_equal(r["desc"][j], r["desc"][row])
    if sc["textured"]:
        assert 0.3 <= np.unpackbits(r["desc"]).mean() <= 0.7, np.unpackbits(r["desc"]).mean()
    if not sc["centroid"]:
        assert not r["moments"].any() and np.all(r["dir"] == onp.direction_fixed(sc["angle"]))
    else:
        A, B = r["dir"][:, 0].astype(np.int64), r["dir"][:, 1].astype(np.int64)
        assert np.all(np.abs(A * A + B * B - 16384 * 16384) <= 2 * 16384)             # a unit vector in Q14 up to the rounding


def test_ramp_reaches_offset_21_and_flat_has_no_direction():
    r = oc.restated("ramp_centroid_corners_k5")
    assert np.all(r["dir"] == (11585, 11585)) and np.all(r["moments"][:, 0] == r["moments"][:, 1]) and np.all(r["moments"] > 0)
    off = np.stack(onp.offsets(oc.corner_pattern(), 11585, 11585))
    assert np.abs(off).max() == 21
    # no direction at all takes a sample further than 22 pixels: what the filter's edge >= 25 has to cover, with the blur's 3
    worst = 0
    for deg in np.arange(0.0, 360.0, 0.25):
        A, B = onp.direction_fixed(deg)
        worst = max(worst, int(np.abs(np.stack(onp.offsets(oc.corner_pattern(), A, B))).max()))
    assert worst <= 22
    f = oc.restated("flat_centroid_k5")
    assert not f["moments"].any() and np.all(f["dir"] == (16384, 0)) and not f["desc"].any()


def test_fixed_angles_are_far_from_a_rounding_tie():
    for deg in oc.ANGLES:
        th = np.float64(deg) * (np.pi / 180.0)
        for v in (16384.0 * np.cos(th), 16384.0 * np.sin(th)):
            assert abs(abs(v - np.floor(v)) - 0.5) > 1e-6, (deg, v)
    assert {sc["angle"] for sc in oc.SCENES.values() if not sc["centroid"]} == set(oc.ANGLES)
    assert onp.direction_fixed(0.0) == (16384, 0) and onp.direction_fixed(90.0) == (0, 16384) and onp.direction_fixed(180.0) == (-16384, 0)
    assert onp.direction_fixed(-1.0) == (16382, -286)


def test_default_pattern_obeys_its_rules():
    p = onp.default_pattern()
    assert p.dtype == np.int8 and p.shape == (256, 4) and p.min() == -15 and p.max() == 15
    assert not np.any((p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3]))
    assert np.array_equal(p, onp.default_pattern())
    assert p[:3].tolist() == DEFAULT_HEAD                                            # pinned: agents that exchange descriptors share it
    c = oc.corner_pattern()
    assert c.shape == (256, 4) and np.abs(c).max() == 15 and not np.any((c[:, 0] == c[:, 2]) & (c[:, 1] == c[:, 3]))


def test_shifted_pair_is_a_shift():
    a, b = oc.shifted_pair()
    dx, dy = oc.SHIFT
    assert np.array_equal(b[dy:, dx:], a[:-dy, :-dx]) and not np.array_equal(a, b)
    pts = np.array([[40, 40], [100, 70], [123, 85]])
    ra = onp.describe(a, pts, onp.default_pattern(), 31, 1)
    rb = onp.describe(b, pts + (dx, dy), onp.default_pattern(), 31, 1)
    assert len(ra["desc"]) == 3 and np.array_equal(ra["desc"], rb["desc"]) and np.array_equal(ra["moments"], rb["moments"])

