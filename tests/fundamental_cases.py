"""The scenes that tests/test_gpu_fundamental.py runs on the device, defined once so that tests/test_fundamental_np.py
can verify their stated conditions (margin >= 1e-6, every hypothesis kept) from the restatement alone, without a GPU.
Restatement results are computed once per process and shared."""
import functools

import numpy as np

import fundamental_np as fnp

K = fnp.K_DEFAULT
S_FOV = 0.95                 # FOV parameter of the distorted scenes
THR = 0.3                    # tracker.cpp: outlier_param1
MAX_MATCHES = 512

# n, outlier share, noise [px], n_hyp, scene seed.  63 / 64 / 65 straddle a wavefront, 255 / 256 / 257 the scoring
# workgroup; at n = 7 every hypothesis is the same sample.  The seeds were chosen on the CPU for the stated conditions.
MASK_CASES = [(7, 0.0, 0.0, 1, 200), (8, 0.125, 0.0, 63, 200), (9, 1 / 3, 0.05, 65, 200), (63, 0.3, 0.0, 256, 201),
              (64, 0.5, 0.05, 65, 200), (65, 0.5, 0.0, 63, 200), (255, 0.4, 0.05, 65, 200), (256, 0.2, 0.0, 256, 200),
              (257, 0.5, 0.05, 1, 200)]
CANDIDATE_CASE = (120, 0.3, 0.05, 256, 2)
PLANTED_CASE = (40, 0.3, 0.0, 256, 305)          # recovered exactly under RANSAC seeds 1, 2, 3
DISTORTED_CASE = (100, 0.3, 0.0, 128, 400)       # through the FOV distortion: the input of filter_matches
DISTORTED_CASES = [DISTORTED_CASE, (300, 0.3, 0.05, 64, 400)]      # (300: the compaction crosses a chunk of 256)


@functools.lru_cache(maxsize=None)
def pair(n, share, noise, seed, mode="general", s=0.0):
    p, c, inl = fnp.make_pair(n, share, noise, seed, mode, s)
    for a in (p, c, inl):
        a.setflags(write=False)
    return p, c, inl


@functools.lru_cache(maxsize=None)
def restated(n, share, noise, n_hyp, scene_seed, seed=0):
    p, c, _ = pair(n, share, noise, scene_seed)
    return fnp.ransac(p, c, K, THR, n_hyp, seed)


@functools.lru_cache(maxsize=None)
def restated_filter(n, share, noise, n_hyp, scene_seed, seed=0):
    p, c, _ = pair(n, share, noise, scene_seed, "general", S_FOV)
    return fnp.filter_matches(p, c, K, S_FOV, THR, n_hyp, seed)


def collinear_pair(n=40):
    """All points of both frames on one image line each: every sample is degenerate."""
    s = np.linspace(50.0, 700.0, n)
    return np.stack([s, 0.4 * s + 30.0], axis=1), np.stack([s + 7.0, 0.4 * s + 33.0], axis=1)
