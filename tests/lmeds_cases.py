"""The scenes that tests/test_gpu_lmeds.py runs on the device, defined once so that tests/test_lmeds_np.py can verify their stated
conditions from the restatement alone, without a GPU: every hypothesis `kept`, gap >= 1e-6 between the two smallest per-hypothesis
medians (the winner cannot flip on round-off), margin >= 1e-6 of every pair from sigma^2 under the winner (the mask cannot either),
noise > 0 (a noise-free scene has round-off medians), an outlier share below one half.  Restatement results are computed once per
process and shared."""
import functools

import fundamental_cases as fc
import lmeds_np as lnp

K = fc.K
S_FOV = fc.S_FOV
MAX_MATCHES = 520                         # (the 513 case)
LMEDS, RANSAC = 4, 8                      # cv::LMEDS, cv::RANSAC: the values of outlier_method
STAGE = 4096                              # XK_RANSAC_MED_STAGE: up to this many errors per candidate are staged in LDS

# n, outlier share, noise [px], n_hyp, scene seed.  15 / 16 / 17: the smallest n whose medians are not round-off, both parities; 64 / 65
# straddle a wavefront, 255 / 256 / 257 the workgroup, 513 takes a third trip.  The seeds were chosen on the CPU for the stated conditions.
MASK_CASES = [(15, 0.3, 0.05, 32, 302), (16, 0.3, 0.05, 32, 302), (17, 0.3, 0.05, 32, 302), (31, 0.3, 0.05, 32, 302),
              (64, 0.3, 0.05, 32, 302), (65, 0.3, 0.05, 32, 302), (255, 0.3, 0.05, 32, 302), (256, 0.3, 0.05, 32, 302),
              (257, 0.3, 0.05, 32, 302), (513, 0.3, 0.05, 32, 302)]
MEDIAN_CASE = (257, 0.3, 0.05, 32, 302)            # medians hypothesis by hypothesis
DISTORTED_CASES = [(100, 0.3, 0.05, 64, 302), (300, 0.3, 0.05, 64, 302)]      # through the FOV distortion: the input of filter_matches


@functools.lru_cache(maxsize=None)
def restated(n, share, noise, n_hyp, scene_seed, seed=0):
    p, c, _ = fc.pair(n, share, noise, scene_seed)
    return lnp.lmeds(p, c, K, n_hyp, seed)


@functools.lru_cache(maxsize=None)
def restated_filter(n, share, noise, n_hyp, scene_seed, seed=0):
    p, c, _ = fc.pair(n, share, noise, scene_seed, "general", S_FOV)
    return lnp.filter_matches(p, c, K, S_FOV, n_hyp, seed)
