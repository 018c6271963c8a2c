"""The scenes that tests/test_gpu_fast.py runs on the device, defined once so that tests/test_fast_np.py can verify the
restatement (tests/fast_np.py) and the scenes' stated conditions without a GPU.  Images and restated results are computed
once per process and shared; nothing here is random at run time (fixed seeds)."""
import functools

import numpy as np

import fast_np as fnp
import klt_cases as kc

KLT_A, KLT_B = "w31_n257", "w21_odd_n255"        # 160 x 120, and 161 x 121 in rows of 176 bytes
DOT_X0, DOT_STEP, DOT_N, DOT_Y, TIE_Y = 8, 5, 17, 12, 30
RECTS = ((12, 10, 30, 24), (40, 14, 58, 33), (66, 9, 88, 21), (14, 36, 33, 55), (45, 41, 60, 57), (70, 30, 90, 52), (2, 2, 9, 7))


def _readonly(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def dots_image():
    """96 x 48: single bright pixels every 5 px along row 12 with strictly decreasing brightness -- with b = 5 every decision
    depends on the one before -- and a second row of equal brightness (ties: raster order)."""
    im = np.full((48, 96), 20, np.uint8)
    for i in range(DOT_N):
        im[DOT_Y, DOT_X0 + DOT_STEP * i] = 250 - 5 * i
        im[TIE_Y, DOT_X0 + DOT_STEP * i] = 150
    return _readonly(im)


@functools.lru_cache(maxsize=None)
def rect_image():
    """96 x 64: bright rectangles (x0, y0, x1, y1 inclusive) on a dark ground, both under a small deterministic texture: on flat
    rectangles neighbouring pixels tie in score and the strict suppression leaves no keypoint at all."""
    y, x = np.mgrid[0:64, 0:96]
    im = 30 + (5 * x + 3 * y) % 11
    for x0, y0, x1, y1 in RECTS:
        im[y0:y1 + 1, x0:x1 + 1] = (180 + (7 * x + 13 * y) % 23)[y0:y1 + 1, x0:x1 + 1]
    return _readonly(im.astype(np.uint8))


def rect_corners():
    return [(x, y) for x0, y0, x1, y1 in RECTS for x in (x0, x1) for y in (y0, y1)]


@functools.lru_cache(maxsize=None)
def noise_image(width, height, seed):
    return _readonly(np.random.default_rng(seed).integers(0, 256, (height, width), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def boxes_image(width, height, seed, n):
    """Random rectangles of random brightness, drawn over one another, under noise of +-6 (on exact rectangles neighbouring
    pixels tie in score and the strict suppression leaves few keypoints)."""
    rng = np.random.default_rng(seed)
    im = np.full((height, width), 90, np.int32)
    for _ in range(n):
        x0, y0 = int(rng.integers(0, width - 4)), int(rng.integers(0, height - 4))
        w, h = int(rng.integers(4, 60)), int(rng.integers(4, 60))
        im[y0:y0 + h, x0:x0 + w] = int(rng.integers(10, 246))
    im += rng.integers(-6, 7, im.shape)
    return _readonly(np.clip(im, 0, 255).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def tiny_image():
    """16 x 16, the smallest image xk_trk_klt_setup takes: one dot where a score exists, one on the 3-pixel frame."""
    im = np.full((16, 16), 40, np.uint8)
    im[8, 7] = 200
    im[3, 12] = 120
    im[2, 5] = 255
    return _readonly(im)


def _scenes():
    S = {}

    def add(name, image, width, threshold=9, nms=1, b=20, m=20, old=(), max_candidates=2048, max_features=320):
        S[name] = dict(name=name, image=image, width=width, threshold=threshold, nms=nms, b=b, m=m,
                       old=np.asarray(old, np.float64).reshape(-1, 2), max_candidates=max_candidates, max_features=max_features)

    for tag, name, W in (("klt160", KLT_A, 160), ("klt161", KLT_B, 161)):
        for which in (0, 1):
            im = functools.partial(lambda n, w: kc.images(n)[w], name, which)
            add(f"{tag}_{which}_t9_b20_m20", im, W, 9, 1, 20, 20)
            add(f"{tag}_{which}_t9_b4_m4", im, W, 9, 1, 4, 4)
            add(f"{tag}_{which}_t20_b6_m8", im, W, 20, 1, 6, 8)
    add("dots", dots_image, 96, 9, 1, 5, 4)
    # one old feature that blocks only the first dot (x = 8) flips the whole chain
    add("dots_old_flips_chain", dots_image, 96, 9, 1, 5, 4, old=[(DOT_X0 - 5.0, float(DOT_Y))])
    add("dots_t254_nothing", dots_image, 96, 254, 1, 5, 4)
    add("dots_b0_all", dots_image, 96, 9, 1, 0, 4)
    add("dots_b_whole_image_one", dots_image, 96, 9, 1, 200, 4)
    add("dots_m_beyond_half_nothing", dots_image, 96, 9, 1, 5, 60)
    add("rects_b3", rect_image, 96, 9, 1, 3, 4)
    add("rects_m0_nms0", rect_image, 96, 9, 0, 2, 0)
    add("tiny16", tiny_image, 16, 9, 1, 2, 0)
    add("tiny16_m3", tiny_image, 16, 9, 1, 2, 3)
    # widths that are no multiple of 4 or 64; threshold 1; no suppression; more than 2048 candidates (several turns of the sort's
    # inner loop); a selection of several hundred
    add("noise67x33_t1", functools.partial(noise_image, 67, 33, 5), 67, 1, 1, 2, 0, max_features=400)
    add("noise130x97_t1_nms0", functools.partial(noise_image, 130, 97, 6), 130, 1, 0, 3, 3, max_candidates=8192, max_features=1024)
    add("noise130x97_t30", functools.partial(noise_image, 130, 97, 6), 130, 30, 1, 1, 5, max_candidates=4096, max_features=2048)
    # old features: on the border, outside the image by less and by more than b, far outside any int, a NaN, two within b of
    # each other, halves that round away from zero
    add("klt160_olds", functools.partial(lambda: kc.images(KLT_A)[0]), 160, 9, 1, 6, 8,
        old=[(0.0, 0.0), (159.0, 119.0), (-3.0, 40.0), (-50.0, 40.0), (163.4, 60.0), (1e12, 50.0), (80.0, -1e300), (float("nan"), 30.0),
             (40.0, float("inf")), (60.2, 50.7), (63.0, 52.0), (100.5, 30.5), (-0.5, 90.5), (120.49999, 80.5)])
    # 640 x 480 with the largest key list: the blocked mask does not fit the LDS behind the keys and lives in global memory
    add("boxes640x480_cap32768", functools.partial(boxes_image, 640, 480, 7, 260), 640, 9, 1, 20, 20, max_candidates=32768,
        max_features=512, old=[(320.0, 240.0), (100.3, 99.6)])
    add("boxes640x480_b3", functools.partial(boxes_image, 640, 480, 7, 260), 640, 30, 1, 3, 20, max_candidates=32768, max_features=2048)
    return S


SCENES = _scenes()
GPU_SCENES = list(SCENES)
THRESHOLDS = (1, 9, 30, 254)


def image(name):
    """uint8 [H, >= W]: the scene's image, possibly a view with a row stride beyond its width."""
    sc = SCENES[name]
    return sc["image"]()


def pixels(name):
    sc = SCENES[name]
    return np.ascontiguousarray(image(name)[:, :sc["width"]])


@functools.lru_cache(maxsize=None)
def restated(name):
    sc = SCENES[name]
    return fnp.detect(pixels(name), sc["threshold"], sc["nms"], sc["b"], sc["m"], sc["old"])


def distinct_images():
    """[(name of the first scene that uses it, pixels)], one entry per distinct image of the scenes (they are cached objects)."""
    out = {}
    for name in SCENES:
        out.setdefault(id(image(name)), (name, pixels(name)))
    return list(out.values())


# the three-image sequence of tests/test_gpu_fast_host.py: the KLT sequence's images
HOST = dict(threshold=9, nms=1, b=6, m=8, max_candidates=4096, n_tiles_h=3, n_tiles_w=4, max_feat_per_tile=4, n_feat_min=400,
            max_features=512)
