"""The scenes that tests/test_gpu_tracker_frame.py runs through xk_trk_frame, defined once so that tests/test_tracker_frame_np.py
can verify their stated conditions from the restatement (tracker_frame_np.TrackerNp) alone, without a GPU.  Images and restated
sequences are computed once per process and shared.

Every scene is a 160 x 120 camera with klt_cases.K_CHAIN intrinsics, at most 320 features and at most 8 frames.  A scene holds one
or more SEQUENCES of images; the tracker is reset (xk_trk_frame_reset) before every sequence after the first, so each sequence
starts with a first frame.

    walk      a translating, slightly affine texture over 6 frames with descriptors: frames that re-detect, frames that do not, and
              a frame on which the overflow pass removes a pair
    dense     block_half_length 2: the first frame accepts more than 257 features, so the frames' counts straddle the 256-wide
              compaction chunk and the 4-features-per-workgroup tracking
    starved   a few isolated blobs: frames whose surviving pairs number 7, 6 and 0 (the RANSAC's edge), a frame that starts from an
              empty resident list (the re-detection starts from nothing), and lists of 1 and 2 pairs into the overflow pass (its
              never-examined last pair)
    blank     a uniform image: nothing is ever detected
    full      max_matches so small that old plus new features exceed it: XK_ECAPACITY, then a first frame"""
import functools

import numpy as np

import klt_cases as kc
import orb_np as onp
import tracker_frame_np as tnp

W, H = 160, 120
SEED = 7                                   # of every frame's RANSAC: frame i of a sequence draws with SEED + i


def blobs(centres, sigma=1.6, amp=90.0):
    """Isolated Gaussian spots on grey: one FAST corner (all 16 ring pixels darker) and one trackable window each."""
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    v = np.full((H, W), 128.0)
    for cx, cy in centres:
        v += amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma * sigma))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def _walk_images(seed, n, step, A=((1.004, 0.003), (-0.002, 0.997)), n_blobs=300):
    tex = kc.texture(seed, W, H, n_blobs)
    A = np.asarray(A, np.float64)
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    out, M, t = [], np.eye(2), np.zeros(2)
    for _ in range(n):
        out.append(kc.render(tex, (), W, H, M, c - M @ c + t))
        M, t = A @ M, t + np.asarray(step, np.float64)
    return out


# seven spots in general position (no three on a line), well inside the margin; the motion between frames is a small affine map,
# which a fundamental matrix fits exactly
SPOTS = [(30.0, 31.0), (62.0, 28.0), (101.0, 33.0), (127.0, 29.0), (33.0, 62.0), (70.0, 57.0), (104.0, 66.0)]
PAIR = [(52.0, 88.0), (70.0, 92.0)]          # two spots of one tile, further apart than block_half_length


def _moved(spots, k):
    return [(x + 1.3 * k + 0.004 * k * (y - 60.0), y - 0.8 * k + 0.006 * k * (x - 80.0)) for x, y in spots]


def _scenes():
    S = {}
    base = dict(max_matches=kc.MAX_FEATURES, win=(16, 16), max_level=0, max_iter=30, eps=0.01, min_eig_thr=0.003,
                threshold=9, non_max_supp=1, block_half_length=8, margin=25, max_candidates=8192, describe=None,
                n_feat_min=0, n_tiles_h=1, n_tiles_w=1, max_feat_per_tile=10000, threshold_px=0.3, n_hyp=128)

    def add(name, sequences, **kw):
        S[name] = dict(base, name=name, sequences=sequences, **kw)

    add("walk", [_walk_images(31, 6, (2.6, -1.7))], describe=dict(edge=25, centroid=1, angle_deg=-1.0, max_desc=kc.MAX_FEATURES),
        block_half_length=6, n_feat_min=34, n_tiles_h=3, n_tiles_w=4, max_feat_per_tile=5)
    add("dense", [_walk_images(32, 3, (1.1, 0.6), n_blobs=900)], block_half_length=2, margin=10, n_feat_min=0)
    add("starved", [
        # 7 detected; 7 tracked, 7 pairs; one spot gone: 6 pairs, nothing kept; an empty list: the re-detection starts from nothing
        [blobs(_moved(SPOTS, 0)), blobs(_moved(SPOTS, 1)), blobs(_moved(SPOTS[:6], 2)), blobs(_moved(SPOTS[:6], 3)), blobs(_moved(SPOTS, 4))],
        [blobs(_moved(SPOTS[:1], 0)), blobs(_moved(SPOTS[:1], 1))],           # a list of 1 into the overflow pass
        [blobs(_moved(PAIR, 0)), blobs(_moved(PAIR, 1))],                     # a list of 2 in one tile: the first pair goes, the last is never examined
    ], block_half_length=10, n_feat_min=1, n_tiles_h=3, n_tiles_w=4, max_feat_per_tile=1)
    add("blank", [[np.full((H, W), 128, np.uint8)] * 3], n_feat_min=0)
    add("full", [_walk_images(31, 4, (2.6, -1.7))], block_half_length=6, max_matches=40, n_feat_min=1000)
    return S


SCENES = _scenes()


def pattern():
    return onp.default_pattern()


def tracker_np(name):
    sc = SCENES[name]
    kw = {k: sc[k] for k in ("max_matches", "win", "max_level", "max_iter", "eps", "min_eig_thr", "threshold", "non_max_supp",
                             "block_half_length", "margin", "max_candidates", "n_feat_min", "n_tiles_h", "n_tiles_w", "max_feat_per_tile",
                             "threshold_px", "n_hyp")}
    d = sc["describe"]
    return tnp.TrackerNp(W, H, kc.K_CHAIN, 0.0, describe=None if d is None else dict(d, pattern=pattern()), **kw)


@functools.lru_cache(maxsize=None)
def restated(name):
    """-> per sequence, per frame: TrackerNp.track's dict, or the CapacityError it raised.  `features` is added: the resident list
    after the frame."""
    t = tracker_np(name)
    out = []
    for seq in SCENES[name]["sequences"]:
        t.reset()
        frames = []
        for i, img in enumerate(seq):
            try:
                r = t.track(img, seed=SEED + i)
                r["features"] = {k: v.copy() for k, v in t.features.items()}
            except tnp.CapacityError as e:
                r = e
            frames.append(r)
        out.append(frames)
    return out
