"""The restatement tests/fast_np.py and the scenes of tests/fast_cases.py, without a GPU: the score image against an independent
segment test, the painted-mask selection against its statement on distances, the properties of a selection (separation,
maximality, order), the rectangle corners, the chains of the dots scenes, and the tile loops on hand-computed cases."""
import numpy as np
import pytest

import fast_cases as fc
import fast_np as fnp


@pytest.mark.parametrize("threshold", fc.THRESHOLDS)
def test_score_image_equals_the_segment_test(threshold):
    for name, im in fc.distinct_images():
        S = fnp.score_image(im, threshold)
        assert np.array_equal(S >= threshold, fnp.segment_test(im, threshold)), (name, threshold)
        assert np.array_equal(S > 0, S >= threshold), name              # 0 everywhere else
        assert not S[:3].any() and not S[-3:].any() and not S[:, :3].any() and not S[:, -3:].any()
        assert S.max() <= 254
        # s is the largest threshold at which the pixel is still a corner: the score does not depend on the threshold asked
        if threshold > 1:
            S1 = fnp.score_image(im, 1)
            assert np.array_equal(S, np.where(S1 >= threshold, S1, 0)), name


@pytest.mark.parametrize("name", fc.GPU_SCENES)
def test_selection_properties(name):
    sc = fc.SCENES[name]
    H, W = fc.pixels(name).shape
    r = fc.restated(name)
    keys, acc, b = r["keys"], r["accepted"], sc["b"]
    assert r["n_candidates"] <= sc["max_candidates"] and len(acc) <= sc["max_features"], (r["n_candidates"], len(acc))
    assert np.array_equal(acc, fnp.select_chebyshev(keys, W, H, b, sc["old"]))
    assert np.all(np.diff(keys.astype(np.int64)) > 0)                       # unique, ascending
    assert np.all(np.diff(keys[acc].astype(np.int64)) > 0)
    x, y, s = fnp.unpack(keys, W)
    assert np.array_equal(s, r["S"][y, x]) and np.all(s >= sc["threshold"])
    m = sc["m"]
    assert np.all((x >= max(m, 3)) & (x <= W - max(m, 3) - 1) & (y >= max(m, 3)) & (y <= H - max(m, 3) - 1))
    pts = np.stack([x, y], axis=1)
    A = pts[acc]
    old = fnp.old_pixels(sc["old"])                                          # Python ints: no overflow for the far ones
    if len(A) > 1:
        D = np.abs(A[:, None, :] - A[None, :, :]).max(axis=2)
        np.fill_diagonal(D, b + 1)
        assert D.min() > b                                                   # pairwise more than b apart
    assert len(A) <= -(-W // (b + 1)) * -(-H // (b + 1))
    blockers = [(int(px), int(py)) for px, py in A] + old
    accepted = set(acc.tolist())
    for i in range(min(len(keys), 600)):                                     # (a prefix of the large scenes: the check is quadratic)
        xi, yi = int(x[i]), int(y[i])
        if i in accepted:
            assert all(max(abs(xi - bx), abs(yi - by)) > b for bx, by in old), i
        else:                                                                # maximal: no rejected candidate could be added
            assert any(max(abs(xi - bx), abs(yi - by)) <= b for bx, by in blockers), i
    assert np.array_equal(r["xy"], A.astype(np.int32).reshape(-1, 2)) and np.array_equal(r["score"], s[acc])


def test_the_scenes_do_what_they_are_there_for():
    n = lambda name: len(fc.restated(name)["accepted"])
    c = lambda name: fc.restated(name)["n_candidates"]
    xs = lambda name: fc.restated(name)["xy"][:, 0].tolist()
    # dots: 17 dots of decreasing brightness 5 px apart, b = 5 -- accept / reject alternate along the row; the tie row in raster order
    d = fc.restated("dots")
    assert c("dots") == 2 * fc.DOT_N and n("dots") == 18
    first = d["xy"][d["xy"][:, 1] == fc.DOT_Y][:, 0].tolist()
    assert first == [fc.DOT_X0 + 10 * i for i in range(9)]
    assert d["xy"][d["xy"][:, 1] == fc.TIE_Y][:, 0].tolist() == first and np.all(d["score"][-9:] == 150 - 20 - 1)
    f = fc.restated("dots_old_flips_chain")
    assert f["xy"][f["xy"][:, 1] == fc.DOT_Y][:, 0].tolist() == [fc.DOT_X0 + 5 + 10 * i for i in range(8)]
    assert c("dots_t254_nothing") == 0 and n("dots_t254_nothing") == 0
    assert n("dots_b0_all") == c("dots_b0_all") == 2 * fc.DOT_N
    assert n("dots_b_whole_image_one") == 1 and xs("dots_b_whole_image_one") == [fc.DOT_X0]
    assert c("dots_m_beyond_half_nothing") == 0
    assert c("tiny16") == 2 and c("tiny16_m3") == 2 and not fc.restated("tiny16")["S"][2, 5]      # the frame scores 0 also with m = 0
    assert c("noise130x97_t1_nms0") > 2048 and n("noise130x97_t1_nms0") > 320
    assert c("boxes640x480_cap32768") > 64
    for name in fc.GPU_SCENES:
        if name.startswith("klt16") and "olds" not in name:
            assert 5 <= n(name) <= c(name), name
    o = fc.restated("klt160_olds")
    base = fnp.detect(fc.pixels("klt160_olds"), 9, 1, 6, 8)
    assert not np.array_equal(o["accepted"], base["accepted"])                # the old features block something


def test_rectangle_corners_are_found():
    sc = fc.SCENES["rects_b3"]
    assert sc["b"] == 3
    r = fc.restated("rects_b3")
    H, W = fc.pixels("rects_b3").shape
    inner = sc["m"] + 3
    checked = 0
    for cx, cy in fc.rect_corners():
        if inner <= cx <= W - inner - 1 and inner <= cy <= H - inner - 1:
            d = np.abs(r["xy"] - np.array([cx, cy])).max(axis=1)
            assert d.min() <= 2, (cx, cy)
            checked += 1
    assert checked == 21                                      # of 28: seven lie nearer the edge than m + 3


def test_tile_loops_on_hand_computed_cases():
    g = fnp.TileGrid(640, 480, 3, 4, 2)                       # tiles 160 wide, 160 high; rows counted from the BOTTOM tile up
    assert (g.tile_width, g.tile_height) == (160.0, 160.0)
    assert g.tile(0.0, 0.0) == (0, 0)                         # r = 479.5: two subtractions
    assert g.tile(160.5, 479.0) == (2, 0)                     # c = 0: not > 0
    assert g.tile(160.51, 479.0) == (2, 1)
    assert g.tile(320.5, 319.5) == (2, 1)                     # r = 160 is not > 160; c = 160 -> one step
    assert g.tile(320.6, 319.4) == (1, 2)
    assert g.tile(639.0, 0.0) == (0, 3)                       # the last tile: c = 478.5 -> 3 steps
    assert g.tile(639.5, -0.5) == (0, 3)                      # r = 480 -> two steps, 160 left: not > 160
    g2 = fnp.TileGrid(100, 70, 3, 3, 1)                       # tile sizes that are no fp64 integers: the loops, not a closed form
    tw, th = 100.0 / 3, 70.0 / 3
    c, col = 99.0 - tw - 0.5, 0
    while c > 0:
        col, c = col + 1, c - tw
    assert g2.tile(99.0, 1.0)[1] == col == 2
    assert g2.tile(99.0, 1.0)[0] == 0 and g2.tile(10.0, 69.0) == (2, 0)


def test_remove_overflow_keeps_the_quirks():
    g = fnp.TileGrid(640, 480, 3, 4, 2)
    cur = [(10.0, 10.0), (20.0, 20.0), (30.0, 30.0), (600.0, 400.0), (40.0, 40.0)]       # four in tile (0, 0), limit 2
    prev = [(x + 1.0, y) for x, y in cur]
    keep, tp, tc = fnp.remove_overflow(g, prev, cur)
    assert tc == [(0, 0), (0, 0), (0, 0), (2, 3), (0, 0)]
    assert keep == [3, 4]                                     # all of the overflowing tile but the LAST pair, which is never examined
    assert g.count(0, 0) == 4                                 # the counts stay as counted
    g.max_feat_per_tile = 4
    assert fnp.remove_overflow(g, prev, cur)[0] == [0, 1, 2, 3, 4]
    assert fnp.remove_overflow(g, [], [])[0] == []
    assert fnp.remove_overflow(g, prev[:1], cur[:1])[0] == [0]
