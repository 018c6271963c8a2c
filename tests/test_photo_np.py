"""What the device cases of tests/test_gpu_photo.py rest on, verified from the restatement tests/photo_np.py alone (no GPU):
every hypothesis and point of every gains case sits >= 1e-9 from the inlier bound, the winner is strictly ahead wherever (a, b)
is compared, the chain's two maps invert each other, a planted gain is found with exactly its inlier set, the correction's table
is the reference's (irPhotoCalib.cpp:42-51), the measured tolerance is the recorded one, and the per-frame scene sits away
from every tie of the tracking."""
import numpy as np
import pytest

import photo_cases as pc
import photo_np as pnp

GAIN_CASES = [(n, h) for n in pc.GAIN_N for h in pc.GAIN_HYP]


def test_sampler_draws_four_distinct_indices():
    for n in (5, 6, 64, 257):
        for h in range(64):
            s = pnp.sample(pc.RANSAC_SEED, h, n)
            assert len(set(s)) == 4 and all(0 <= i < n for i in s)
    assert pnp.sample(1, 0, 100) != pnp.sample(1, 1, 100) and pnp.sample(1, 0, 100) != pnp.sample(2, 0, 100)


@pytest.mark.parametrize("n,n_hyp", GAIN_CASES)
def test_gains_case_margin_and_winner(n, n_hyp):
    o, p, r = pc.gain_case(n, n_hyp)
    assert len(o) == n and r["ab"].shape == (n_hyp, 2)
    assert r["margin"] >= pc.MARGIN, r["margin"]
    assert r["support"] >= 1 and r["inliers"][r["winner"]] == r["support"] == int(r["mask"].sum())
    assert not np.any(r["inliers"][:r["winner"]] >= r["support"])          # ties go to the lowest hypothesis
    if pc.strict(n, n_hyp):
        assert r["support"] > r["runner_up"]


def test_most_cases_compare_the_gains():
    """Every size and every hypothesis count has a case whose (a, b) is compared."""
    for n in pc.GAIN_N:
        assert any(pc.strict(n, h) for h in pc.GAIN_HYP), n
    for h in pc.GAIN_HYP[:-1]:
        assert any(pc.strict(n, h) for n in pc.GAIN_N), h


def test_chain_and_relative_gains_invert_each_other():
    rng = np.random.default_rng(0)
    for _ in range(200):
        a1, b1 = rng.uniform(0.7, 1.4), rng.uniform(-0.2, 0.2)
        a2, b2 = rng.uniform(0.7, 1.4), rng.uniform(-0.2, 0.2)
        a, b = pnp.chain_gains(a1, b1, *pnp.relative_gains(a1, b1, a2, b2))
        assert abs(a - a2) <= 8 * np.finfo(float).eps * abs(a2) and abs(b - b2) <= 8 * np.finfo(float).eps * max(abs(b2), abs(a2))
    assert pnp.chain_gains(1.0, 0.0, 1.25, -0.5) == (1.25, -0.5) and pnp.relative_gains(1.0, 0.0, 1.25, -0.5) == (1.25, -0.5)


def test_planted_gain_is_found_with_its_inlier_set():
    """30 % outliers, inlier noise far below the bound: the winner's mask is exactly the planted set and the refit the planted pair."""
    o, p, good = pc.gain_data(120, 4242, noise=5.0e-4)
    assert abs(good.mean() - 0.7) < 0.01
    r = pnp.gains_ransac(o, p, 64, 11)
    assert np.array_equal(r["mask"], good) and r["support"] == int(good.sum())
    assert abs(r["a"] - pc.PLANTED[0]) < 2e-3 and abs(r["b"] - pc.PLANTED[1]) < 2e-3
    assert r["margin"] >= pc.MARGIN


def test_fit_is_the_minimum_of_the_cost():
    o, p, _ = pc.gain_data(40, 9, outliers=0.0)
    a, b = pnp.fit(o, p)

    def cost(a, b):
        return float(((o - p * a - (1 - p) * b) ** 2).sum() + pnp.W2 * (a - 1) ** 2 + pnp.W2 * b * b)

    c0 = cost(a, b)
    for da, db in ((1e-4, 0), (-1e-4, 0), (0, 1e-4), (0, -1e-4), (7e-5, -7e-5)):
        assert cost(a + da, b + db) > c0
    assert pnp.fit([], []) == (1.0, 0.0)                                    # the prior alone: the identity


def test_process_frame_small_groups_and_the_ring():
    ring = [(1.0, 0.0)]
    o, p, _ = pc.gain_data(4, 1)
    r = pnp.process_frame(ring, [(o, p)], [1], 4, 0, 0.0, 0.0)
    assert r["support"][0] == 0 and (r["a_rel"][0], r["b_rel"][0]) == (1.0, 0.0) and ring == [(1.0, 0.0), (1.0, 0.0)]
    o, p, _ = pc.gain_data(5, pc.case_seed(5, 1))
    for _ in range(20):
        pnp.process_frame(ring, [(o, p)], [1], 1, pc.RANSAC_SEED, 0.02, 0.01)
    assert len(ring) == pnp.RING
    with pytest.raises(ValueError):
        pnp.process_frame(ring, [(o, p)], [16], 1, 0, 0.0, 0.0)


def test_table_is_the_reference_table():
    for i in range(256):                                                    # irPhotoCalib.cpp:42-51, entry by entry
        want = (i * 2) & 255 if i < 128 else (255 if i == 128 else (512 - 2 * i) & 255)
        assert pnp.LUT[i] == want
    assert pnp.LUT.dtype == np.uint8 and pnp.LUT[0] == 0 and pnp.LUT[127] == 254 and pnp.LUT[129] == 254 and pnp.LUT[255] == 2


def test_correction_cases_cover_the_sign_rule_and_the_wrap():
    im = pc.cor_image()
    assert np.array_equal(np.unique(im), np.arange(256))
    assert np.array_equal(pnp.correct(im, 1.0, 0.0), pnp.LUT[im])           # v / 255 * 255 truncates back to v for every byte
    a, b = pc.COR_PAIRS[1][:2]
    f32 = np.float32
    c = ((im.astype(f32) * (f32(1) / f32(255))) * f32(a - b) + f32(b)) * f32(255)
    assert (c <= -1).any() and (c >= 256).any()                             # the remainder's sign rule and the wrap both act
    out = pnp.correct(im, a, b)
    assert np.all(out[c <= -1] == 0) and out.dtype == np.uint8
    assert not np.array_equal(pnp.correct(im, 0.8, 0.05, pc.cor_spatial()), pnp.correct(im, 0.8, 0.05))
    assert np.array_equal(pnp.correct(im, float("nan"), 0.0), np.zeros_like(im))


def test_intensity_windows():
    im = pc.int_image()
    W, H = pc.INT_SIZE
    for ks in pc.INT_KERNELS:
        v, s, c = pnp.intensity(im, pc.int_points(), ks)
        hk = ks // 2
        assert c[0] == hk * hk and c[4] == min(2 * hk, W) * min(2 * hk, H)
        assert c[7] == 0 and v[7] == 0.0 and s[7] == 0
        assert np.all(v[c > 0] == s[c > 0] / (255.0 * c[c > 0]))
    v, s, c = pnp.intensity(im, [(7, 11)], 2)
    assert s[0] == int(im[10:12, 6:8].astype(int).sum()) and c[0] == 4       # the asymmetric window of tracker.cpp:866-867


def test_measured_tolerance_is_the_recorded_one():
    m = pc.measured_deviation()
    print("largest relative deviation of a refit under 16 summation orders:", m, "bound", pc.GAINS_RTOL)
    assert 0.0 < m <= pc.GAINS_MEASURED and pc.GAINS_RTOL == 16 * pc.GAINS_MEASURED
    assert pc.GAINS_RTOL < 1e-2 * pc.MARGIN                                  # far below the distance of any point from the inlier bound


def test_frame_scene():
    """About 40 features, all decisions of the tracking away from a tie (the floor margins are 0 by construction: FAST features
    are integer pixels, so a window's corner is an exact integer or half-integer at every level, and its floor is exact), the
    RANSAC away from its bound with a strict winner, and the three calls do what the GPU test expects of them."""
    xy, val = pc.frame_features()
    assert 35 <= len(xy) <= 45
    (r0, ring0), (r1, ring1), (r2, ring2) = pc.frame_restated()
    im1, im2 = pc.frame_images()
    assert not r0["estimated"] and ring0 == [(1.0, 0.0)] and np.array_equal(r0["image"], im2)
    assert r1["estimated"] and len(ring1) == 2 and len(r1["keep_idx"]) >= 35
    worst = min(v for m in r1["track"]["margins"] for k, v in m.items() if k != "floor")
    assert worst >= pc.MARGIN, worst
    assert r1["ransac"]["margin"] >= pc.MARGIN and r1["support"] > r1["ransac"]["runner_up"]
    assert np.array_equal(r1["image"], pnp.correct(im2, *ring1[-1]))
    assert not r2["estimated"] and ring2 == ring1 and np.array_equal(r2["image"], r1["image"])
    # the estimate sees the planted change of brightness: 0.9 v + 12 on the current frame, inverted
    a, b = r1["a_rel"], r1["b_rel"]
    assert abs((a - b) - 1.0 / 0.9) < 0.03 and abs(b + 12.0 / 255.0 / 0.9) < 0.02


def test_three_group_case():
    """The groups of the G = 3 case draw from seed + g: each away from the inlier bound."""
    for g, n in enumerate((63, 64, 65)):
        o, p, _ = pc.gain_case(n, 63)
        r = pnp.gains_ransac(o, p, 63, pc.RANSAC_SEED + g)
        assert r["margin"] >= pc.MARGIN and r["support"] >= 5, (g, r["margin"])
