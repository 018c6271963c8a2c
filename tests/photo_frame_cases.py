"""The scenes that tests/test_gpu_photo_frame.py runs through xk_trk_photo_frame, defined once so that tests/test_photo_frame_np.py
can verify their stated conditions from the restatement (photo_frame_np.PhotoTrackerNp) alone, without a GPU.  Images and restated
sequences are computed once per process and shared.

Every scene is a 160 x 120 camera with klt_cases.K_CHAIN intrinsics, at most 320 features and at most 8 frames per sequence.  A
scene holds one or more SEQUENCES; the tracker is reset (xk_trk_frame_reset) before every sequence after the first, so each starts
with a first frame, and the photometric state (the ring, the done flag) carries over from one sequence to the next.

    gain_walk  the walk texture of tracker_frame_cases under a different affine brightness per frame, with descriptors: every later
               frame estimates gains, a frame re-detects after the calibration is done, the overflow pass removes a pair, and the
               corrected image differs from the raw one
    switch     gain_walk with a threshold_photo: the frame of the first estimate re-detects, with the switched threshold already
    dense      block_half_length 2: more than 257 resident features on a calibrating frame
    starved    isolated spots: three resident features (no calibration tracking, no estimate) before and after the calibration is
               done; four or more of which the calibration keeps three (the ring does not advance; corrected iff done); an empty
               resident list; lists of 7, 6, 1 and 2 pairs into the RANSAC and the overflow pass
    blank      a uniform image: nothing is ever detected
    full       max_matches so small that old plus new features exceed it in mid-frame, after the frame's calibration has advanced
               the ring: XK_ECAPACITY, then a first frame
    spatial    gain_walk with a spatial setup of 16-pixel cells: rows accumulate on every estimating frame"""
import functools

import numpy as np

import klt_cases as kc
import photo_frame_np as pfn
import tracker_frame_cases as tc

W, H = tc.W, tc.H
SEED = tc.SEED                             # frame i of a sequence: the RANSAC draws with SEED + i, the gain RANSAC with SEED_PHOTO + i
SEED_PHOTO = 101
SP_MAX_COUNT, SP_MAX_ROWS, SP_THR = 500, 4096, 0.9
WALK_STEP = (2.7, -1.7)                   # of the walk texture per frame (tracker_frame_cases' walk takes (2.6, -1.7): under these gains one of
                                          # its resident positions lies 7e-10 px from a float32 rounding boundary)


def brighten(img, gain, offset):
    """v' = clip(round(gain v + offset)): the camera's affine brightness of one frame."""
    return np.clip(np.rint(gain * np.asarray(img, np.float64) + offset), 0, 255).astype(np.uint8)


GAINS = [(1.0, 0.0), (0.95, 8.0), (0.92, 14.0), (0.96, 10.0), (0.9, 20.0), (0.94, 16.0), (0.91, 22.0), (0.95, 12.0)]


def _bright(images, gains=GAINS):
    return [brighten(im, *gains[i % len(gains)]) for i, im in enumerate(images)]


# seven spots in general position, one per tile of the 3 x 4 grid and well inside the margin on every frame; FAINT is detected by FAST
# (threshold 9) but its window's smaller eigenvalue, 0.0013, is below min_eig_thr: the tracking never keeps it
SPOTS = [(30.0, 34.0), (100.0, 33.0), (127.0, 52.0), (62.0, 47.0), (32.0, 72.0), (72.0, 88.0), (112.0, 86.0)]
FAINT = (62.0, 47.0)
FAINT_AMP = 18.0
SPOT_AMP = 40.0


def _spots(spots, k, faint=()):
    """Gaussian spots as tracker_frame_cases.blobs, moved k steps, under frame k's brightness; `faint` ones at FAINT_AMP.  They stand
    on a ramp from 10 to 90 across the image, so that the features' box means differ (a gain fit over equal intensities is
    ill-conditioned: its offset would be compared to a bound it cannot meet) and every value stays below 128, where the
    correction's table is monotone."""
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    v = 10.0 + 80.0 * x / W
    for amp, group in ((SPOT_AMP, spots), (FAINT_AMP, faint)):
        for cx, cy in tc._moved(list(group), k):
            v += amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * 1.6 * 1.6))
    return brighten(np.clip(np.rint(v), 0, 255), *GAINS[k % len(GAINS)])


def _scenes():
    S = {}
    base = dict(tc.SCENES["walk"], kernel_size=10, eps_gap=0.02, eps_base=0.01, photo_max_hyp=64, n_hyp_photo=48, threshold_photo=-1,
                spatial=None)
    for k in ("name", "sequences"):
        base.pop(k)
    plain = dict(base, describe=None, block_half_length=8, n_feat_min=0, n_tiles_h=1, n_tiles_w=1, max_feat_per_tile=10000)

    def add(name, sequences, like=base, **kw):
        S[name] = dict(like, name=name, sequences=sequences, **kw)

    walk = _bright(tc._walk_images(31, 6, WALK_STEP))
    add("gain_walk", [walk])
    add("switch", [walk], threshold_photo=14)
    add("dense", [_bright(tc._walk_images(32, 3, (1.1, 0.6), n_blobs=900))], like=plain, block_half_length=2, margin=10)
    S7, S3 = SPOTS, SPOTS[:3]
    three = [_spots(S3, 0), _spots(S3, 1)]
    three_and_faint = [_spots(S3, 0, [FAINT]), _spots(S3, 1, [FAINT])]
    add("starved", [
        [_spots(S7[:1], 0), _spots(S7[:1], 1)],                                     # a list of 1 into the overflow pass
        [_spots(tc.PAIR, 0), _spots(tc.PAIR, 1)],                                   # a list of 2 in one tile: the first pair goes
        three + [_spots(S3, 2)],                                                    # 3 resident before done: nothing; then an empty list
        three_and_faint,                                                            # 4 resident, the calibration keeps 3: before done
        # done from frame 1, whose working plane is corrected and the previous one is not: nothing survives; frame 2 re-detects 7 from an
        # empty list: 7 pairs; frame 3 has lost a spot, whose window still tracks: 7; frame 4 drops it: 6 pairs keep nothing; frame 5: empty
        [_spots(S7, 0), _spots(S7, 1), _spots(S7, 2), _spots(S7[:6], 3), _spots(S7[:6], 4), _spots(S7, 5)],
        three,                                                                      # 3 resident after done: corrected
        three_and_faint,                                                            # the calibration keeps 3 after done: corrected, the ring stays
    ], like=plain, block_half_length=10, n_feat_min=1, n_tiles_h=3, n_tiles_w=4, max_feat_per_tile=1)
    add("blank", [[np.full((H, W), 128, np.uint8)] * 3], like=plain)
    add("full", [_bright(tc._walk_images(31, 4, WALK_STEP))], like=plain, block_half_length=6, max_matches=40, n_feat_min=1000)
    add("spatial", [walk], spatial=dict(div=16, max_count=SP_MAX_COUNT, max_rows=SP_MAX_ROWS, coverage_thr=SP_THR))
    return S


SCENES = _scenes()


def tracker_np(name):
    sc = SCENES[name]
    kw = {k: sc[k] for k in ("max_matches", "win", "max_level", "max_iter", "eps", "min_eig_thr", "threshold", "non_max_supp",
                             "block_half_length", "margin", "max_candidates", "n_feat_min", "n_tiles_h", "n_tiles_w", "max_feat_per_tile",
                             "threshold_px", "n_hyp", "kernel_size", "eps_gap", "eps_base", "n_hyp_photo", "threshold_photo")}
    d, sp = sc["describe"], sc["spatial"]
    return pfn.PhotoTrackerNp(W, H, kc.K_CHAIN, 0.0, describe=None if d is None else dict(d, pattern=tc.pattern()),
                              spatial=None if sp is None else dict(div=sp["div"], max_count=sp["max_count"], max_rows=sp["max_rows"]), **kw)


def run_np(name, pairs=None):
    """Every sequence of the scene through PhotoTrackerNp -> per sequence, per frame: its dict with `features` (the resident list
    after it), `ring` (after it) and, in a spatial scene, `sp_rows`; or the CapacityError it raised (with .calibration, .planes and
    .ring).  pairs: per sequence, per frame, the ring pair to take as given (None: the restated one)."""
    t = tracker_np(name)
    out = []
    for si, seq in enumerate(SCENES[name]["sequences"]):
        t.reset()
        frames = []
        for i, img in enumerate(seq):
            try:
                r = t.track(img, seed=SEED + i, seed_photo=SEED_PHOTO + i, ring_pair=None if pairs is None else pairs[si][i])
                r["features"] = {k: v.copy() for k, v in t.features.items()}
            except pfn.CapacityError as e:
                r = e
            if isinstance(r, Exception):
                r.ring = list(t.state["ring"])
            else:
                r["ring"] = list(t.state["ring"])
                if t.spatial is not None:
                    r["sp_rows"] = len(t.sp_state["b"])
            frames.append(r)
        out.append(frames)
    return out


@functools.lru_cache(maxsize=None)
def restated(name):
    return run_np(name)
