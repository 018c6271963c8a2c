"""Per-frame wall time of xk_trk_photo_frame against the same frames through the CHAIN of the stage entries, which is
what every caller of a PHOTOMETRIC_CALI build did before it (push_image, photo_calibrate, track, photo_intensity, detect,
photo_intensity, track, photo_intensity, filter_matches through the host), on the GPU box.  Both go through the same ctypes binding,
so both carry its cost; a frame ends in its own synchronisation, so a host clock around it is the frame.

The scene of tools/bench_tracker_frame.py (640 x 480 blobs alternating between two positions, no descriptors, one tile, window
31 x 31, max_level 2, 256 hypotheses, about 200 and about 400 features), at half the exposure, the second position under another brightness
(v' = 0.93 v + 6 of the first): every frame after the first estimates gains and corrects its image.  Per feature count, steady frames
(n_feat_min = 1: the re-detection is queued and skipped) and re-detecting frames (n_feat_min = 100000), frame entry and chain
alternating in blocks of --frames frames, three repeats.

    python tools/bench_photo_frame.py [--frames 300]
The chain uses only entries that exist without the photometric frame, so the yardstick is the chain ON A BUILD OF THE PARENT COMMIT:
    python tools/bench_photo_frame.py --only-chain --lib /path/to/the/parent's/libxk.so
--second W H MAX_LEVEL MIN_EIG_THR declares the second Lucas-Kanade parameter set (xk_trk_klt_second) on both sides: the frame
switches to it on the device once the calibration is done, the chain calls klt_select(done) between photo_calibrate and track.  Every
line above is then a time AFTER the switch (the scene estimates gains from its second tracked image on).  A frame that tracks BEFORE
the switch exists only at a start: after a uniform image the list is empty, the next image but one re-detects on its predecessor and
tracks what it found with the first set, and the image after that estimates.  The option therefore adds, per feature count, cycles of
photo_reset, frame_reset, a uniform image, the two images and --after further frames of a re-detecting tracker, and reports the
re-detecting frame before the switch (no calibration yet: its list was empty) and the re-detecting frames after it separately.
One profiler run of its own lists the HIP calls of a frame (the single hipStreamSynchronize, the two hipMemcpyAsync):
    rocprofv3 --hip-trace --stats --output-format csv -d DIR -o f -- python tools/bench_photo_frame.py --frames 50 --only-frame"""
import argparse, os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--only-frame", action="store_true", help="the frame entry alone, steady frames (profiler runs)")
ap.add_argument("--only-chain", action="store_true", help="the chain alone (with --lib: on another build of the library)")
ap.add_argument("--lib", default=None, help="the libxk.so to load instead of this tree's")
ap.add_argument("--second", nargs=4, default=None, metavar=("W", "H", "MAX_LEVEL", "MIN_EIG_THR"), help="the second Lucas-Kanade parameter set")
ap.add_argument("--after", type=int, default=20, help="with --second: frames after the switch per cycle")
args = ap.parse_args()
SECOND = None if args.second is None else dict(win=(int(args.second[0]), int(args.second[1])), max_level=int(args.second[2]),
                                               min_eig_thr=float(args.second[3]))

import torch
from x_multi_agent_amd import engine, tracker

if not torch.cuda.is_available():
    sys.exit("bench_photo_frame: no GPU -- a time measured anywhere else says nothing")
W, H, WIN, MAX_LEVEL, N_HYP, MAX_FEATURES = 640, 480, (31, 31), 2, 256, 2048
K = (500.0, 500.0, 320.0, 240.0)
KERNEL, EPS_GAP, EPS_BASE, PHOTO_HYP = 30, 0.02, 0.01, 256


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
    return v


# at half the exposure of bench_tracker_frame's images, so that every value stays below 128, where the correction's table
# (irPhotoCalib.cpp:42-51) is monotone: across its fold at 128 two frames corrected with slightly different gains differ locally and
# the steady-state list decays to a dozen features
pair = (np.clip(np.rint(0.5 * blobs_image(7, (0.0, 0.0))), 0, 255).astype(np.uint8),
        np.clip(np.rint(0.465 * blobs_image(7, (3.3, -2.1)) + 6.0), 0, 255).astype(np.uint8))
eng = engine.Engine(4, 0, 4, lib_path=args.lib)


def make(b, n_feat_min, frame):
    mf = tracker.MatchFilter(eng, MAX_FEATURES, K, 0.0)
    k = tracker.Klt(eng, 0, W, H, WIN, MAX_LEVEL, match_filter=mf, **({} if SECOND is None else dict(second=SECOND)))
    k.detect_setup(9, 1, b, 20, 32768)
    k.photo_setup(KERNEL, EPS_GAP, EPS_BASE, PHOTO_HYP)
    if frame:
        k.frame_setup(n_feat_min, 1, 1, 100000, 0.3, N_HYP)
        k.photo_frame_setup(PHOTO_HYP, -1)
    return mf, k


class Frame:
    def __init__(self, b, n_feat_min):
        self.mf, self.k = make(b, n_feat_min, True)
        self.i = 0

    def step(self):
        r = self.k.photo_frame(pair[self.i & 1], seed=self.i, seed_photo=self.i)
        self.i += 1
        return r["n_matches"] if self.i > 1 else r["n_accepted"], r["redetected"], int(r["estimated"])

    def close(self):
        self.k.close()
        self.mf.close()


class Chain:
    """The same frame over the stage entries.  One tile that never overflows: removeOverflowFeatures keeps every pair, so the host
    pass between the device calls costs this side nothing here."""

    def __init__(self, b, n_feat_min):
        self.mf, self.k = make(b, n_feat_min, False)
        self.n_feat_min, self.i, self.xy, self.val, self.done = n_feat_min, 0, None, None, False

    def step(self):
        k, redetected = self.k, 0
        k.push_image(pair[self.i & 1])
        if self.xy is None:
            xy = k.detect(1)["xy"]
            self.xy, self.val = xy.astype(np.float64), k.photo_intensity(xy, 1, 1)[0].copy()
            self.i += 1
            return len(self.xy), 0, 0
        c = k.photo_calibrate(self.xy.astype(np.float32), self.val, max(1, min(len(self.xy), PHOTO_HYP)), self.i)
        if SECOND is not None:
            self.done = self.done or bool(c["estimated"])
            k.klt_select(1 if self.done else 0)
        r = k.track(self.xy.astype(np.float32))
        prev, cur = self.xy[r["keep_idx"]], r["kept_cur"]
        val = k.photo_intensity(np.trunc(cur).astype(np.int32), 1, 0)[0].copy()
        if len(cur) < self.n_feat_min:
            redetected = 1
            d = k.detect(0, prev)["xy"]
            k.photo_intensity(d, 0, 1)
            nxy = d.astype(np.float64)
            r2 = k.track(nxy.astype(np.float32))
            v2 = k.photo_intensity(np.trunc(r2["kept_cur"]).astype(np.int32), 1, 0)[0].copy()
            prev, cur, val = np.concatenate([prev, nxy[r2["keep_idx"]]]), np.concatenate([cur, r2["kept_cur"]]), np.concatenate([val, v2])
        mask, m, pxy, cxy = self.mf.filter_matches(prev, cur, 0.3, N_HYP, self.i)
        self.xy, self.val = cur[m], val[m]
        self.i += 1
        return len(m), redetected, int(c["estimated"])

    def close(self):
        self.k.close()
        self.mf.close()


def block(obj):
    t0 = time.perf_counter()
    for _ in range(args.frames):
        n, red, est = obj.step()
    return 1e3 * (time.perf_counter() - t0) / args.frames, n, red, est


for b in (26, 17):
    for label, n_feat_min in (("steady      ", 1), ("re-detecting", 100000)):
        if args.only_frame and n_feat_min != 1:
            continue
        sides = ([] if args.only_chain else [("frame", Frame(b, n_feat_min))]) + ([] if args.only_frame else [("chain", Chain(b, n_feat_min))])
        for _, o in sides:
            for w in range(30):
                o.step()
        res = {name: [] for name, _ in sides}
        for rep in range(3):
            for name, o in sides:
                res[name].append(block(o))
        line = f"b = {b:2d}  {label}"
        for name, _ in sides:
            last = res[name][-1]
            line += f"  {name}: " + " / ".join(f"{t[0]:6.3f}" for t in res[name]) + f" ms per frame ({last[1]} features, re-detected {last[2]}, estimated {last[3]})"
        if len(sides) == 2:
            fm, cm = min(t[0] for t in res["frame"]), min(t[0] for t in res["chain"])
            line += f"  best: {fm:.3f} vs {cm:.3f} ms, frame / chain = {fm / cm:.3f}"
        print(line, flush=True)
        for _, o in sides:
            o.close()

def switch_cycles(b):
    """Cycles from a start on a re-detecting tracker with the second set -> (ms of the frame that tracks before the switch, ms per frame
    after it, features)."""
    f = Frame(b, 100000)
    blank = np.full((H, W), 64, np.uint8)
    before, after, n = [], [], 0
    cycles = max(3, args.frames // max(args.after, 1))
    for c in range(cycles + 2):                                     # (two cycles of warm-up)
        f.k.photo_reset()
        f.k.frame_reset()
        f.i = 0
        f.k.photo_frame(blank)
        f.step()
        t0 = time.perf_counter()
        r = f.k.photo_frame(pair[1], seed=1, seed_photo=1)
        t1 = time.perf_counter()
        assert not r["done"] and r["n_new_tracked"] > 0, "the frame before the switch tracked nothing"
        f.i = 2
        for _ in range(args.after):
            n, red, est = f.step()
        t2 = time.perf_counter()
        if c >= 2:
            before.append(1e3 * (t1 - t0))
            after.append(1e3 * (t2 - t1) / args.after)
    f.close()
    return before, after, n


if SECOND is not None and not args.only_chain and not args.only_frame:
    for b in (26, 17):
        before, after, n = switch_cycles(b)
        print(f"b = {b:2d}  re-detecting frame BEFORE the switch (first set, no calibration): median {np.median(before):6.3f} min {min(before):6.3f} ms;  "
              f"AFTER it (second set): median {np.median(after):6.3f} min {min(after):6.3f} ms per frame ({n} features, {len(before)} cycles)", flush=True)
eng.close()
