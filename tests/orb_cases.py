"""The scenes that tests/test_gpu_orb.py runs on the device, defined once so that tests/test_orb_np.py can verify the
restatement (tests/orb_np.py) and the scenes' stated conditions without a GPU.  Images, keypoint lists and restated results
are computed once per process and shared; nothing here is random at run time (fixed seeds)."""
import functools

import numpy as np

import fast_cases as fc
import klt_cases as kc
import orb_np as onp

ANGLES = (-1.0, 0.0, 37.0, 90.0, 180.0)         # every fixed angle a GPU scene uses
KLT_ODD = "w21_odd_n255"                        # 161 x 121 in rows of 176 bytes
SHIFT = (5, 3)                                  # of tests/test_gpu_orb.py's chain and of host/examples/describe_main.cpp


def _readonly(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def rects_image():
    """96 x 80: random rectangles under noise of +-6: corners and edges at every orientation of the tests."""
    return fc.boxes_image(96, 80, 31, 40)


@functools.lru_cache(maxsize=None)
def ramp_image():
    """96 x 80: the diagonal ramp I = 40 + x + y.  Its centroid direction is the diagonal, (A, B) = (11585, 11585), under which
    the pattern points (+-15, +-15) land 21 pixels from the keypoint: the furthest a sample gets."""
    y, x = np.mgrid[0:80, 0:96]
    return _readonly((40 + x + y).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def flat_image():
    return _readonly(np.full((80, 96), 77, np.uint8))


@functools.lru_cache(maxsize=None)
def big_image():
    return fc.boxes_image(640, 480, 7, 260)


@functools.lru_cache(maxsize=None)
def strided_image():
    return kc.images(KLT_ODD)[1]


@functools.lru_cache(maxsize=None)
def corner_pattern():
    """A caller's pattern: the four diagonals between the corners (+-15, +-15) first, then a fixed random draw."""
    rng = np.random.default_rng(77)
    rows = [(15, 15, -15, -15), (-15, 15, 15, -15), (15, -15, 15, 15), (-15, -15, 0, 0)]
    while len(rows) < 256:
        c = tuple(int(v) for v in rng.integers(-15, 16, 4))
        if c[:2] != c[2:]:
            rows.append(c)
    return _readonly(np.asarray(rows, np.int8))


@functools.lru_cache(maxsize=None)
def keypoints(W, H, edge, n_kept, seed):
    """int32 [n, 2] of which exactly n_kept pass the border filter.  Lists of five or more kept hold the filter's four boundary
    pairs in x and in y, a duplicate, a negative and an over-large coordinate; every list drops something.  Kept and dropped
    points are interleaved by a fixed shuffle."""
    rng = np.random.default_rng(seed)
    cx, cy = W // 2, H // 2
    drop = [(edge - 1, cy), (W - edge, cy), (cx, edge - 1), (cx, H - edge), (-5, cy), (cx, 10 ** 6), (-2 ** 31, 2 ** 31 - 1)]
    keep = [(edge, cy), (W - edge - 1, cy), (cx, edge), (cx, H - edge - 1), (edge, cy)] if n_kept >= 5 else []
    while len(keep) < n_kept:
        keep.append((int(rng.integers(edge, W - edge)), int(rng.integers(edge, H - edge))))
    for _ in range(max(n_kept // 8, 2)):              # dropped points inside the image, in the border zone
        drop.append((int(rng.integers(0, edge)), int(rng.integers(0, H))) if rng.integers(2) else (int(rng.integers(0, W)), int(rng.integers(H - edge, H))))
    pts = np.asarray(keep + drop, np.int64)
    return _readonly(pts[rng.permutation(len(pts))].astype(np.int32))


def _scenes():
    S = {}

    def add(name, image, width, edge, n_kept, centroid, angle=-1.0, pattern=None, textured=True):
        S[name] = dict(name=name, image=image, width=width, edge=edge, n_kept=n_kept, centroid=centroid, angle=angle, pattern=pattern,
                       textured=textured, seed=len(S) + 1)

    # 1, 63, 64, 65, 257 kept keypoints: the tails of a wavefront's ballot, of a workgroup of four and of the compaction's chunk
    add("rects_centroid_k63", rects_image, 96, 25, 63, 1)
    add("rects_fixed-1_k64", rects_image, 96, 25, 64, 0, -1.0)
    add("rects_fixed37_corners_k65", rects_image, 96, 25, 65, 0, 37.0, corner_pattern)
    add("rects_fixed0_k1", rects_image, 96, 25, 1, 0, 0.0)
    add("rects_fixed180_corners_k63", rects_image, 96, 25, 63, 0, 180.0, corner_pattern)
    add("rects_centroid_corners_k257", rects_image, 96, 25, 257, 1, pattern=corner_pattern)
    # a view with a row stride beyond its width, an odd size that is no multiple of the blur's tile, OpenCV's edge
    add("strided161_centroid_corners_k257", strided_image, 161, 31, 257, 1, pattern=corner_pattern)
    add("strided161_fixed90_k65", strided_image, 161, 31, 65, 0, 90.0)
    add("ramp_centroid_corners_k5", ramp_image, 96, 25, 5, 1, pattern=corner_pattern, textured=False)
    add("flat_centroid_k5", flat_image, 96, 25, 5, 1, textured=False)
    # more keypoints than the description's grid holds wavefronts
    add("big640_centroid_k3000", big_image, 640, 31, 3000, 1)
    add("big640_fixed-1_corners_k3000", big_image, 640, 31, 3000, 0, -1.0, corner_pattern)
    return S


SCENES = _scenes()
GPU_SCENES = list(SCENES)


def image(name):
    """uint8 [H, >= W]: the scene's image, possibly a view with a row stride beyond its width."""
    return SCENES[name]["image"]()


def pixels(name):
    return np.ascontiguousarray(image(name)[:, :SCENES[name]["width"]])


def pattern(name):
    """The pattern the scene passes (None: the default) and the one the restatement uses."""
    p = SCENES[name]["pattern"]
    return (None, onp.default_pattern()) if p is None else (p(), p())


def points(name):
    sc = SCENES[name]
    return keypoints(sc["width"], pixels(name).shape[0], sc["edge"], sc["n_kept"], sc["seed"])


@functools.lru_cache(maxsize=None)
def blurred(image_fn, width):
    return _readonly(onp.blur(np.ascontiguousarray(image_fn()[:, :width])))


@functools.lru_cache(maxsize=None)
def restated(name):
    sc = SCENES[name]
    return onp.describe(pixels(name), points(name), pattern(name)[1], sc["edge"], sc["centroid"], sc["angle"], G=blurred(sc["image"], sc["width"]))


def shifted_pair():
    """The rectangles scene and its copy shifted by SHIFT (what moves in from the border is noise of its own): inside the
    overlap every pixel of the second image is the first one's at (x - 5, y - 3)."""
    a = np.asarray(fc.boxes_image(160, 120, 41, 90))
    b = np.array(fc.noise_image(160, 120, 42))
    b[SHIFT[1]:, SHIFT[0]:] = a[:-SHIFT[1], :-SHIFT[0]]
    return _readonly(a.copy()), _readonly(b)


# host/examples/describe_main.cpp and the chain of tests/test_gpu_orb.py: detection and description of the shifted pair
HOST = dict(threshold=9, nms=1, b=4, m=8, max_candidates=4096, max_features=256, edge=31, orientation=1, angle=-1.0, max_desc=4096)
