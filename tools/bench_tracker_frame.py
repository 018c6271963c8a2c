"""Per-frame wall time of xk_trk_frame against the same frames through the CHAIN of the stage entries, which is what
every caller did before it (push_image, track, detect, track, filter_matches through the host), on the GPU box.  Both go through
the same ctypes binding, so both carry its cost; a frame ends in its own synchronisation, so a host clock around it is the frame.

640 x 480 images of one blob scene, alternating between two positions (the features persist, the tracker stays in steady state),
no descriptors, one tile, window 31 x 31, max_level 2, 256 hypotheses (the settings of tools/bench_klt.py and
bench_fundamental.py); about 200 and about 400 features (block_half_length 26 and 17).  Per feature count, three kinds of frame, frame entry and chain alternating in blocks of --frames frames, three repeats:

    steady, nothing queued     n_feat_min = 0: the re-detection branch is not queued at all
    steady, queued + skipped   n_feat_min = 1: its launches are issued on every frame and return at the flag
    re-detecting               n_feat_min = 100000: every frame detects on the previous image and tracks what it accepts

    python tools/bench_tracker_frame.py [--frames 300] [--method ransac|lmeds]
--method lmeds: both sides under xk_trk_outlier_method(4).
--model euroc: both sides under a radial-tangential lens (xk_trk_camera_model); the scene is rendered without one, so
the feature counts are the scene's, the times are those of the launches.
The frame entry of another build of the library (the parent commit's, as the yardstick of a change to the host code):
    python tools/bench_tracker_frame.py --only-frame --lib /path/to/the/parent's/libxk.so
One profiler run of its own lists the HIP calls of a frame (the single hipStreamSynchronize, the two hipMemcpyAsync):
    rocprofv3 --hip-trace --stats --output-format csv -d DIR -o f -- python tools/bench_tracker_frame.py --frames 50 --only-frame"""
import argparse, os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--only-frame", action="store_true", help="the frame entry alone, steady and queued (profiler runs)")
ap.add_argument("--lib", default=None, help="the libxk.so to load instead of this tree's")
ap.add_argument("--method", choices=("ransac", "lmeds"), default="ransac", help="the outlier_method of both sides")
ap.add_argument("--model", choices=("fov", "euroc"), default="fov", help="euroc: both sides under xk_trk_camera_model(1, EuRoC's radtan coefficients)")
args = ap.parse_args()

import torch
from x_multi_agent_amd import engine, tracker

if not torch.cuda.is_available():
    sys.exit("bench_tracker_frame: no GPU -- a time measured anywhere else says nothing")
W, H, WIN, MAX_LEVEL, N_HYP, MAX_FEATURES = 640, 480, (31, 31), 2, 256, 2048
K = (500.0, 500.0, 320.0, 240.0)


def blobs_image(seed, shift):
    """Gaussian blobs (sigma 1.5 ... 5 px) on grey, each added on its own 8-sigma patch, the whole scene moved by `shift`."""
    rng = np.random.default_rng(seed)
    n = 4000
    cx, cy = rng.uniform(-10, W + 10, n) + shift[0], rng.uniform(-10, H + 10, n) + shift[1]
    sig, amp = rng.uniform(1.5, 5.0, n), rng.uniform(25.0, 70.0, n) * rng.choice([-1.0, 1.0], n)
    v = np.full((H, W), 128.0)
    for x0, y0, s, a in zip(cx, cy, sig, amp):
        xa, xb, ya, yb = max(int(x0 - 4 * s), 0), min(int(x0 + 4 * s) + 2, W), max(int(y0 - 4 * s), 0), min(int(y0 + 4 * s) + 2, H)
        if xa < xb and ya < yb:
            y, x = np.mgrid[ya:yb, xa:xb]
            v[ya:yb, xa:xb] += a * np.exp(-((x - x0) ** 2 + (y - y0) ** 2) / (2 * s * s))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


pair = (blobs_image(7, (0.0, 0.0)), blobs_image(7, (3.3, -2.1)))
eng = engine.Engine(4, 0, 4, lib_path=args.lib)


def make(b, n_feat_min, frame):
    mf = tracker.MatchFilter(eng, MAX_FEATURES, K, 0.0)
    k = tracker.Klt(eng, 0, W, H, WIN, MAX_LEVEL, match_filter=mf)
    if args.method == "lmeds":
        mf.outlier_method(4)
    if args.model == "euroc":
        mf.camera_model(tracker.CAM_RADTAN, (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0))
    k.detect_setup(9, 1, b, 20, 32768)
    if frame:
        k.frame_setup(n_feat_min, 1, 1, 100000, 0.3, N_HYP)
    return mf, k


class Frame:
    def __init__(self, b, n_feat_min):
        self.mf, self.k = make(b, n_feat_min, True)
        self.i = 0

    def step(self):
        r = self.k.frame(pair[self.i & 1], seed=self.i)
        self.i += 1
        return r["n_matches"] if self.i > 1 else r["n_accepted"], r["redetected"]

    def close(self):
        self.k.close()
        self.mf.close()


class Chain:
    """The same frame over the stage entries.  One tile that never overflows: removeOverflowFeatures keeps every pair, so the host
    pass between the two device calls costs this side nothing here."""

    def __init__(self, b, n_feat_min):
        self.mf, self.k = make(b, n_feat_min, False)
        self.n_feat_min, self.i, self.xy = n_feat_min, 0, None

    def step(self):
        k, redetected = self.k, 0
        k.push_image(pair[self.i & 1])
        if self.xy is None:
            self.xy = k.detect(1)["xy"].astype(np.float64)
            self.i += 1
            return len(self.xy), 0
        r = k.track(self.xy.astype(np.float32))
        prev, cur = self.xy[r["keep_idx"]], r["kept_cur"]
        if len(cur) < self.n_feat_min:
            redetected = 1
            nxy = k.detect(0, prev)["xy"].astype(np.float64)
            r2 = k.track(nxy.astype(np.float32))
            prev, cur = np.concatenate([prev, nxy[r2["keep_idx"]]]), np.concatenate([cur, r2["kept_cur"]])
        mask, m, pxy, cxy = self.mf.filter_matches(prev, cur, 0.3, N_HYP, self.i)
        self.xy = cur[m]
        self.i += 1
        return len(m), redetected

    def close(self):
        self.k.close()
        self.mf.close()


def block(obj):
    t0 = time.perf_counter()
    for _ in range(args.frames):
        n, red = obj.step()
    return 1e3 * (time.perf_counter() - t0) / args.frames, n, red


for b in (26, 17):
    for label, n_feat_min in (("steady, nothing queued  ", 0), ("steady, queued + skipped", 1), ("re-detecting            ", 100000)):
        if args.only_frame and n_feat_min != 1:
            continue
        sides = [("frame", Frame(b, n_feat_min))] + ([] if args.only_frame else [("chain", Chain(b, n_feat_min))])
        for _, o in sides:
            for w in range(30):
                o.step()
        res = {name: [] for name, _ in sides}
        for rep in range(3):
            for name, o in sides:
                res[name].append(block(o))
        line = f"b = {b:2d}  {label}"
        for name, _ in sides:
            line += f"  {name}: " + " / ".join(f"{t:6.3f}" for t, _, _ in res[name]) + f" ms per frame ({res[name][-1][1]} features, re-detected {res[name][-1][2]})"
        if len(sides) == 2:
            fm, cm = min(t for t, _, _ in res["frame"]), min(t for t, _, _ in res["chain"])
            line += f"  best: {fm:.3f} vs {cm:.3f} ms, frame / chain = {fm / cm:.3f}"
        print(line, flush=True)
        for _, o in sides:
            o.close()
eng.close()
