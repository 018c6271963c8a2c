"""The scenes that tests/test_gpu_klt.py runs on the device, defined once so that tests/test_klt_np.py can verify their
stated conditions (every margin >= 1e-9, the exits they are there for, the validity of the definition) from the
restatement alone, without a GPU.  Images and restatement results are computed once per process and shared.

An image is a function of continuous coordinates -- a sum of Gaussian blobs (sigma 1.5 ... 5 px) on grey, with painted
regions -- evaluated at warped pixel centres and quantised to uint8: a feature at p in the first image is at A p + t in
the second.  No image file, no SciPy."""
import functools

import numpy as np

import klt_np as knp

K_CHAIN = (120.0, 120.0, 80.0, 60.0)      # intrinsics of the chained scene's MatchFilter (160 x 120 image), s = 0
MAX_FEATURES = 320
FEATURES_PER_WORKGROUP = 4                # of xk_klt_track: n = 3, 4, 5 straddle it


def texture(seed, width, height, n_blobs=300):
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-20, width + 20, n_blobs), rng.uniform(-20, height + 20, n_blobs)], axis=1)
    return c, rng.uniform(1.5, 5.0, n_blobs), rng.uniform(25.0, 70.0, n_blobs) * rng.choice([-1.0, 1.0], n_blobs)


def scene_function(tex, paints, X, Y):
    c, sig, amp = tex
    v = np.full(X.shape, 128.0)
    for (cx, cy), s, a in zip(c, sig, amp):
        v += a * np.exp(-((X - cx) ** 2 + (Y - cy) ** 2) / (2.0 * s * s))
    for kind, x0, y0, x1, y1 in paints:
        inside = (X >= x0) & (X < x1) & (Y >= y0) & (Y < y1)
        if kind == "flat":                # nothing to track at any level
            p = np.full(X.shape, 128.0)
        elif kind == "wave8":             # period 8: period 2 two levels up, where a central difference sees nothing
            p = 128.0 + 90.0 * np.cos(2 * np.pi * X / 8.0) * np.cos(2 * np.pi * Y / 8.0)
        else:                             # "faint": enough gradient to pass min_eig, little enough for long steps
            p = 128.0 + 14.0 * np.sin(X / 3.0) + 14.0 * np.cos(Y / 2.5)
        v = np.where(inside, p, v)
    return v


def render(tex, paints, width, height, A=np.eye(2), t=(0.0, 0.0), bright=()):
    """The image whose pixel x shows the scene at A^-1 (x - t); bright: (x0, y0, x1, y1, step) added in image coordinates."""
    x, y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    Ai = np.linalg.inv(np.asarray(A, np.float64))
    X = Ai[0, 0] * (x - t[0]) + Ai[0, 1] * (y - t[1])
    Y = Ai[1, 0] * (x - t[0]) + Ai[1, 1] * (y - t[1])
    v = scene_function(tex, paints, X, Y)
    for x0, y0, x1, y1, step in bright:
        v = v + step * ((x >= x0) & (x < x1) & (y >= y0) & (y < y1))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def edge_points(width, height):
    """The window across each edge and two corners, outside the frame near and far, one non-finite point."""
    return [(3.3, height / 2 + 0.4), (width - 2.6, height / 2 - 3.3), (width / 2 + 0.7, 2.2), (width / 2 - 5.1, height - 1.7),
            (2.7, 3.1), (width - 1.4, height - 2.2), (-200.5, 50.2), (-12.3, 40.6), (width + 40.7, height + 30.2),
            (float("nan"), 10.0)]


# name -> size, row stride, window, max_level, max_iter, n, motion (A about the image centre, t), seed, paints, second-image
# brightness steps, special points.  The seeds were chosen on the CPU for the conditions tests/test_klt_np.py asserts.
def _scenes():
    S = {}

    def add(name, size=(160, 120), stride=None, win=(31, 31), max_level=2, max_iter=30, n=64, A=None, t=(0.0, 0.0), seed=1,
            paints=(), bright=(), special=(), eps=0.01, thr=0.003):
        S[name] = dict(name=name, size=size, stride=stride or size[0], win=win, max_level=max_level, max_iter=max_iter, n=n,
                       A=np.eye(2) if A is None else np.asarray(A, np.float64), t=t, seed=seed, paints=tuple(paints),
                       bright=tuple(bright), special=tuple(special), eps=eps, thr=thr)

    e160, e161 = edge_points(160, 120), edge_points(161, 121)
    add("w31_n257", n=257, t=(3.3, -2.1), seed=11, special=e160)
    add("w31_flat_n5", n=5, t=(1.1, 0.7), seed=11, paints=[("flat", 96, 66, 146, 116)], special=[(121.3, 91.2), (119.6, 89.4)])
    add("w31_maxlevel4", max_level=4, n=65, t=(2.0, 1.5), seed=12)
    add("w21_odd_n255", size=(161, 121), stride=176, win=(21, 21), n=255, t=(-6.0, 4.5), seed=13, special=e161)
    add("w15_affine_n256", win=(15, 15), n=256, A=[[1.01, 0.02], [-0.015, 0.99]], t=(1.2, -0.8), seed=14, special=e160)
    add("w5_n64", size=(161, 121), stride=176, win=(5, 5), n=64, t=(0.4, -0.3), seed=15,
        paints=[("wave8", 16, 16, 80, 80), ("faint", 0, 88, 40, 121)], bright=[(0, 88, 40, 121, 70.0)],
        special=e161[:6] + [(48.3, 47.6), (44.2, 52.3), (5.6, 104.3), (8.2, 110.4), (12.4, 99.7)])
    add("w9x5_n63", win=(9, 5), n=63, t=(0.7, 0.6), seed=16, paints=[("wave8", 40, 24, 120, 88)],
        special=e160[:6] + [(80.4, 56.3), (76.7, 60.2)])
    add("w21_6px_level0_n5", win=(21, 21), max_level=0, n=5, t=(6.0, 0.0), seed=17)
    add("w21_6px_n63", win=(21, 21), n=63, t=(6.0, 0.0), seed=17)
    add("w31_iter1_n4", max_iter=1, n=4, t=(1.5, 0.5), seed=18)
    add("w31_iter2_n3", max_iter=2, n=3, t=(1.5, 0.5), seed=18)
    add("w15_n1", win=(15, 15), n=1, t=(0.3, 0.2), seed=19)
    add("w15_n0", win=(15, 15), n=0, t=(0.3, 0.2), seed=19)
    add("chain_w21_n120", win=(21, 21), n=120, t=(2.4, -1.6), seed=20)
    return S


SCENES = _scenes()
GPU_SCENES = list(SCENES)
CHAIN = "chain_w21_n120"
CHAIN_RANSAC = dict(threshold_px=0.3, n_hyp=128, seed=0)
# three images on one object (win 15): tracked 1 -> 2, then 2 -> 3
SEQUENCE = dict(size=(160, 120), win=(15, 15), max_level=2, seed=21, n=40, t12=(1.7, -0.9), t23=(-2.2, 1.4))
SEQUENCE_RESIZED = dict(size=(96, 80), win=(9, 9), max_level=1, seed=22, n=20, t=(0.8, 0.6))


def _centre_motion(sc):
    """A about the image centre: x -> A (x - c) + c + t, as x -> A x + t'."""
    c = np.array([(sc["size"][0] - 1) / 2.0, (sc["size"][1] - 1) / 2.0])
    return sc["A"], c - sc["A"] @ c + np.asarray(sc["t"], np.float64)


@functools.lru_cache(maxsize=None)
def images(name):
    """-> (first, second) uint8 [H, stride] with the image in the first W columns and 0xA5 in the padding."""
    sc = SCENES[name]
    W, H = sc["size"]
    tex = texture(sc["seed"], W, H)
    A, t = _centre_motion(sc)
    out = []
    for im in (render(tex, sc["paints"], W, H), render(tex, sc["paints"], W, H, A, t, sc["bright"])):
        buf = np.full((H, sc["stride"]), 0xA5, np.uint8)
        buf[:, :W] = im
        buf.setflags(write=False)
        out.append(buf)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def points(name):
    """float32 [n, 2]: the special points first, the rest uniform with the window >= 8 px inside both images."""
    sc = SCENES[name]
    W, H = sc["size"]
    rng = np.random.default_rng(sc["seed"] + 1000)
    mx, my = (sc["win"][0] - 1) / 2 + 9 + abs(sc["t"][0]) + 2, (sc["win"][1] - 1) / 2 + 9 + abs(sc["t"][1]) + 2
    p = np.stack([rng.uniform(mx, W - 1 - mx, sc["n"]), rng.uniform(my, H - 1 - my, sc["n"])], axis=1)
    k = min(len(sc["special"]), sc["n"])
    if k:
        p[:k] = np.asarray(sc["special"][:k])
    p = p.astype(np.float32)
    p.setflags(write=False)
    return p


def planted(name):
    """Where the scene's motion takes each point (fp64 [n, 2])."""
    A, t = _centre_motion(SCENES[name])
    return points(name).astype(np.float64) @ A.T + t


def interior(name):
    """Features whose window lies >= 8 px inside both images."""
    sc = SCENES[name]
    W, H = sc["size"]
    hx, hy = (sc["win"][0] - 1) / 2 + 8, (sc["win"][1] - 1) / 2 + 8
    ok = np.ones(sc["n"], bool)
    for q in (points(name).astype(np.float64), planted(name)):
        with np.errstate(invalid="ignore"):
            ok &= (q[:, 0] - hx >= 0) & (q[:, 0] + hx <= W - 1) & (q[:, 1] - hy >= 0) & (q[:, 1] + hy <= H - 1)
    return ok


@functools.lru_cache(maxsize=None)
def pyramids(name):
    sc = SCENES[name]
    W = sc["size"][0]
    return tuple(knp.build_pyramid(im[:, :W], sc["win"], sc["max_level"]) for im in images(name))


@functools.lru_cache(maxsize=None)
def restated(name):
    sc = SCENES[name]
    p1, p2 = pyramids(name)
    return knp.track(p1, p2, points(name), sc["win"], sc["max_iter"], sc["eps"], sc["thr"])


@functools.lru_cache(maxsize=None)
def sequence():
    """-> three images, the points, and the restated results of 1 -> 2 and 2 -> 3 (from the first result's kept points)."""
    q = SEQUENCE
    W, H = q["size"]
    tex = texture(q["seed"], W, H)
    t13 = (q["t12"][0] + q["t23"][0], q["t12"][1] + q["t23"][1])
    ims = [render(tex, (), W, H), render(tex, (), W, H, t=q["t12"]), render(tex, (), W, H, t=t13)]
    rng = np.random.default_rng(q["seed"] + 1000)
    p = np.stack([rng.uniform(24, W - 25, q["n"]), rng.uniform(24, H - 25, q["n"])], axis=1).astype(np.float32)
    pyr = [knp.build_pyramid(im, q["win"], q["max_level"]) for im in ims]
    r12 = knp.track(pyr[0], pyr[1], p, q["win"])
    p2 = r12["kept_cur"].astype(np.float32)
    r23 = knp.track(pyr[1], pyr[2], p2, q["win"])
    r13 = knp.track(pyr[0], pyr[2], p2, q["win"])       # what a stale previous slot would give
    return ims, p, r12, p2, r23, r13


@functools.lru_cache(maxsize=None)
def resized():
    q = SEQUENCE_RESIZED
    W, H = q["size"]
    tex = texture(q["seed"], W, H, 120)
    ims = [render(tex, (), W, H), render(tex, (), W, H, t=q["t"])]
    rng = np.random.default_rng(q["seed"] + 1000)
    p = np.stack([rng.uniform(16, W - 17, q["n"]), rng.uniform(16, H - 17, q["n"])], axis=1).astype(np.float32)
    pyr = [knp.build_pyramid(im, q["win"], q["max_level"]) for im in ims]
    return ims, p, knp.track(pyr[0], pyr[1], p, q["win"])
