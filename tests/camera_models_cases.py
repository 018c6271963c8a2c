"""The coefficient sets and scenes that tests/test_gpu_camera_models*.py run on the device, defined once so that
tests/test_camera_models_np.py can verify their stated conditions from the restatement (tests/camera_models_np.py) alone, without a
GPU.  Restatement results are computed once per process and shared.  K = fundamental_np.K_DEFAULT on 752 x 480 throughout."""
import functools

import numpy as np

import camera_models_np as cnp
import fundamental_cases as fc
import fundamental_np as fnp

K = fnp.K_DEFAULT
WIDTH, HEIGHT = fnp.WIDTH, fnp.HEIGHT
MAX_MATCHES = 1024

# name -> (model, coefficients)
EUROC = (cnp.RADTAN, (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0))          # a real calibration
BARREL = (cnp.RADTAN, (0.12, 0.02, -0.0005, 0.0007))                                      # the four-coefficient form
FOLDING = (cnp.RADTAN, (-0.35, 0.15, 0.001, -0.0008, -0.03))                              # folds inside the image
TUMVI = (cnp.EQUIDISTANT, (0.0034823894, 0.0007150348, -0.0020532361, 0.0002029367))      # a real calibration
KB = (cnp.EQUIDISTANT, (-0.05, 0.01, -0.004, 0.0005))                                     # a stronger equidistant model
SETS = dict(EUROC=EUROC, BARREL=BARREL, FOLDING=FOLDING, TUMVI=TUMVI, KB=KB)
REGULAR = ("EUROC", "BARREL", "TUMVI", "KB")                                              # every pixel converges

N_DRAW = 20000               # the CPU conditions' uniform draw
N_GPU = 500                  # the device tests' random pixels, in front of the fixed ones
FIXED = np.array([[K[2], K[3]], [K[2] + 200.0, K[3]], [K[2], K[3] - 150.0], [0.0, 0.0], [WIDTH - 1.0, 0.0], [0.0, HEIGHT - 1.0],
                  [WIDTH - 1.0, HEIGHT - 1.0]])     # the principal point, a point on each axis, the four corners
FOLD_DETJ = 0.05             # FOLDING: below this det J at the restatement's solution a point is not compared


@functools.lru_cache(maxsize=None)
def draw(n, seed=11):
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0.0, WIDTH, n), rng.uniform(0.0, HEIGHT, n)], axis=1)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def gpu_points():
    p = np.concatenate([draw(N_GPU, 12), FIXED])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def restated_undistort(name, which="gpu"):
    """-> (xy, state, steps, detj) of the set's undistortion of gpu_points() or of the N_DRAW draw."""
    model, k = SETS[name]
    out = cnp.undistort(gpu_points() if which == "gpu" else draw(N_DRAW), K, model, k)
    for a in out:
        a.setflags(write=False)
    return out


# The filter on distorted pixels: scenes of fundamental_cases.pair on UNDISTORTED pixels, pushed through the restatement's distort.
# name, n, outlier share, noise [px], n_hyp, scene seed, in the pattern of fundamental_cases.DISTORTED_CASES; the scene seeds were
# chosen on the CPU for the restatement's conditions (margin >= 1e-6, every hypothesis kept), which test_camera_models_np.py asserts.
FILTER_CASES = [("EUROC", 40, 0.3, 0.0, 128, 400), ("EUROC", 300, 0.3, 0.05, 64, 400),
                ("TUMVI", 40, 0.3, 0.0, 128, 400), ("TUMVI", 300, 0.3, 0.05, 64, 400)]
FILTER_SEED = 4


@functools.lru_cache(maxsize=None)
def filter_scene(name, n, share, noise, scene_seed):
    """-> distorted previous and current pixels [n, 2] of the scene under the set."""
    model, k = SETS[name]
    p, c, _ = fc.pair(n, share, noise, scene_seed)
    dp, dc = cnp.distort(p, K, model, k), cnp.distort(c, K, model, k)
    for a in (dp, dc):
        a.setflags(write=False)
    return dp, dc


@functools.lru_cache(maxsize=None)
def restated_filter(name, n, share, noise, n_hyp, scene_seed):
    """fundamental_np's filter fed the restatement's undistortion -> its dict with keep_idx, prev_xy, cur_xy, and `states`."""
    model, k = SETS[name]
    dp, dc = filter_scene(name, n, share, noise, scene_seed)
    up, sp = cnp.undistort(dp, K, model, k)[:2]
    uc, sc = cnp.undistort(dc, K, model, k)[:2]
    r = fnp.ransac(up, uc, K, fc.THR, n_hyp, FILTER_SEED)
    keep = np.flatnonzero(r["mask"]).astype(np.int32)
    r.update(keep_idx=keep, prev_xy=up[keep], cur_xy=uc[keep], states=np.concatenate([sp, sc]))
    return r
