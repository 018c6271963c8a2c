"""The cases that tests/test_gpu_photo.py runs on the device, defined once so that tests/test_photo_np.py can verify their stated
conditions from the restatement alone, without a GPU: every | |d| - 8e-3 | >= 1e-9, the winner ahead of the runner-up where (a, b)
is compared, the tracking margins of the per-frame scene.  Inputs and restatement results are computed once per process and shared.

The gains tolerance is MEASURED ON THE RESTATEMENT, never on the device: every compared case's refit in numpy.longdouble against
the same refit in fp64 under 16 random summation orders; the largest relative deviation is GAINS_MEASURED (test_photo_np.py
recomputes it and asserts it does not exceed the recorded value) and the bound is 16 x that: the margin covers orders not sampled
and the chain's further dozen operations."""
import functools

import numpy as np

import fast_np as fnp
import klt_cases as kc
import photo_np as pnp

MARGIN = 1e-9
GAINS_MEASURED = 7.8e-14      # measured_deviation() gives 7.70e-14 (in b of the n = 63, one-hypothesis case: 3 inliers); recorded rounded up
GAINS_RTOL = 16 * GAINS_MEASURED
PLANTED = (0.86, 0.07)        # o = p (a - b) + b

GAIN_N = (5, 63, 64, 65, 255, 256, 257)
GAIN_HYP = (1, 63, 65, 256)
# (n, n_hyp) -> data seed where it is not 1000 n + n_hyp, chosen on the CPU (choose_seeds below) for the margin and, where one exists
# within 400 tries, for a winner strictly ahead of the runner-up.  None exists for n = 5 with several hypotheses (five subsets of
# four) or for 256 hypotheses (many draw inliers only and tie): those cases compare counts, winner and support, not (a, b)
GAIN_SEEDS = {(63, 63): 63103, (63, 65): 63103, (64, 65): 64128, (65, 63): 65065, (255, 63): 255067, (255, 65): 255067, (256, 63): 256068,
              (256, 65): 256068, (257, 63): 257070, (257, 65): 257070, (5, 1): 5003, (5, 256): 5257}
RANSAC_SEED = 7


def gain_data(n, seed, noise=6.0e-3, outliers=0.3):
    """-> (o_hist, o_cur, planted inlier mask): the planted pair with uniform noise of the threshold's order, so that hypotheses
    differ in their counts, and `outliers` of the points far off."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, n)
    a, b = PLANTED
    o = p * (a - b) + b + rng.uniform(-noise, noise, n)
    bad = np.zeros(n, bool)
    bad[rng.permutation(n)[:int(round(outliers * n))]] = True
    o[bad] += rng.choice([-1.0, 1.0], bad.sum()) * rng.uniform(0.05, 0.4, bad.sum())
    for v in (o, p):
        v.setflags(write=False)
    return o, p, ~bad


def case_seed(n, n_hyp):
    return GAIN_SEEDS.get((n, n_hyp), 1000 * n + n_hyp)


@functools.lru_cache(maxsize=None)
def gain_case(n, n_hyp):
    """-> (o_hist, o_cur, the restated RANSAC of the group)."""
    o, p, _ = gain_data(n, case_seed(n, n_hyp))
    return o, p, pnp.gains_ransac(o, p, n_hyp, RANSAC_SEED)


def strict(n, n_hyp):
    """(a, b) of the case is compared: its winner is strictly ahead."""
    r = gain_case(n, n_hyp)[2]
    return r["support"] > r["runner_up"]


def choose_seeds(tries=400):
    """What GAIN_SEEDS was filled from."""
    out = {}
    for n in GAIN_N:
        for nh in GAIN_HYP:
            fallback = None
            for s in range(1000 * n + nh, 1000 * n + nh + tries):
                o, p, _ = gain_data(n, s)
                r = pnp.gains_ransac(o, p, nh, RANSAC_SEED)
                if r["margin"] < 1e-7 or r["support"] < 1:
                    continue
                if fallback is None:
                    fallback = s
                if r["support"] > r["runner_up"]:
                    fallback = s
                    break
            out[(n, nh)] = fallback
    return out


def measured_deviation(orders=16):
    """The largest relative deviation of a compared case's fp64 refit, under `orders` random summation orders, from its refit in
    numpy.longdouble."""
    worst = 0.0
    rng = np.random.default_rng(99)
    for n in GAIN_N:
        for nh in GAIN_HYP:
            if not strict(n, nh):
                continue
            o, p, r = gain_case(n, nh)
            idx = np.flatnonzero(r["mask"])
            ea, eb = pnp.fit(o, p, idx, np.longdouble)
            for _ in range(orders):
                a, b = pnp.fit(o, p, rng.permutation(idx))
                worst = max(worst, abs(float((a - ea) / ea)), abs(float((b - eb) / eb)))
    return worst


def close(got, ref):
    """Within GAINS_RTOL of ref, relative, component by component (a component that is exactly 0, as b of an identity gain, must be
    met exactly)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(np.all(np.abs(got - ref) <= GAINS_RTOL * np.abs(ref)))


# ---- intensity ----
INT_SIZE = (40, 36)
INT_KERNELS = (2, 30, 31, 64)


@functools.lru_cache(maxsize=None)
def int_image():
    W, H = INT_SIZE
    im = np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8)
    im.setflags(write=False)
    return im


def int_points():
    W, H = INT_SIZE
    return np.array([(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2), (W, H // 2), (-1, 3), (W + 40, H + 40), (-41, 5),
                     (7, 11), (W - 2, 1)], np.int32)


# ---- correction ----
COR_SIZE = (48, 20)
COR_PAIRS = ((1.0, 0.0, False), (1.3, -0.1, False), (0.8, 0.05, True))


@functools.lru_cache(maxsize=None)
def cor_image():
    W, H = COR_SIZE
    rng = np.random.default_rng(6)
    v = np.concatenate([np.arange(256), rng.integers(0, 256, W * H - 256)]).astype(np.uint8)
    im = rng.permutation(v).reshape(H, W)
    im.setflags(write=False)
    return im


@functools.lru_cache(maxsize=None)
def cor_spatial():
    W, H = COR_SIZE
    ps = np.random.default_rng(8).uniform(-0.2, 0.2, (H, W)).astype(np.float32)
    ps.setflags(write=False)
    return ps


# ---- the per-frame chain ----
FRAME = dict(size=(96, 80), win=(10, 10), max_level=1, max_iter=30, eps=0.01, min_eig_thr=0.003, kernel_size=10, shift=(2, 1), seed=31,
             threshold=10, b=2, margin=10, n_hyp=40, ransac_seed=1, eps_gap=0.02, eps_base=0.01)


@functools.lru_cache(maxsize=None)
def frame_images():
    """-> (first, second): the second is the first shifted by FRAME['shift'] with v' = clip(round(0.9 v + 12))."""
    q = FRAME
    W, H = q["size"]
    tex = kc.texture(q["seed"], W, H, 160)
    im1 = kc.render(tex, (), W, H)
    moved = kc.render(tex, (), W, H, t=q["shift"])
    im2 = np.clip(np.rint(0.9 * moved.astype(np.float64) + 12.0), 0, 255).astype(np.uint8)
    for im in (im1, im2):
        im.setflags(write=False)
    return im1, im2


@functools.lru_cache(maxsize=None)
def frame_features():
    """-> (float32 [n, 2] pixels of the features detected in the first image, their intensities there)."""
    q = FRAME
    im1, _ = frame_images()
    det = fnp.detect(im1, q["threshold"], 1, q["b"], q["margin"])
    xy = det["xy"].astype(np.int32)
    value, _, _ = pnp.intensity(im1, xy, q["kernel_size"])
    return xy.astype(np.float32), value


def frame_klt():
    q = FRAME
    return dict(win=q["win"], max_level=q["max_level"], max_iter=q["max_iter"], eps=q["eps"], min_eig_thr=q["min_eig_thr"])


@functools.lru_cache(maxsize=None)
def frame_restated():
    """Three calls on the pair, as the GPU test makes them: 3 features before any estimate (nothing happens), all features (an
    estimate), 3 features again (corrected with the old pair).  -> list of (result, ring after it)."""
    q = FRAME
    im1, im2 = frame_images()
    xy, val = frame_features()
    state = dict(ring=[(1.0, 0.0)], done=False)
    out = []
    for k in (3, len(xy), 3):
        r = pnp.calibrate(state, im1, im2, xy[:k], val[:k], q["n_hyp"], q["ransac_seed"], q["kernel_size"], q["eps_gap"], q["eps_base"], frame_klt())
        out.append((r, list(state["ring"])))
    return out
