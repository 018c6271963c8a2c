"""Cost of the feature detection on the GPU box: milliseconds per xk_trk_detect on one 640 x 480 image (old features
in, three launches, the result block out, one synchronisation) at thresholds 9 and 30 with n_old = 0 and 200, block_half_length
20, margin 20, timed with HIP events on the handle's stream over --calls calls after 20 (repeated three times: the spread is
printed), and one core's time for the NumPy restatement beside it:
    python tools/bench_fast.py [--calls 200]
The per-kernel split comes from a run of its own under the profiler (tracing slows the host, so the times above are taken
without it):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/bench_fast.py --calls 50 --no-cpu
    python tools/bench_fast.py --kernel-stats DIR"""
import argparse, csv, glob, os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--no-cpu", action="store_true", help="skip the NumPy restatement (profiler runs)")
ap.add_argument("--kernel-stats", metavar="DIR", help="print the xk_fast_* rows of a rocprofv3 --kernel-trace --stats run and exit")
args = ap.parse_args()
if args.kernel_stats:
    files = glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit("bench_fast: no *kernel_stats.csv under " + args.kernel_stats)
    for r in csv.DictReader(open(files[0])):
        if "xk_fast" in r["Name"]:
            print(f"{r['Name'][:40]:40s} calls {r['Calls']:>6s} avg_us {float(r['AverageNs']) / 1e3:8.2f} min_us {float(r['MinNs']) / 1e3:8.2f} "
                  f"max_us {float(r['MaxNs']) / 1e3:8.2f}")
    sys.exit(0)

import torch
import fast_np as fnp
from x_multi_agent_amd import engine, tracker

if not torch.cuda.is_available():
    sys.exit("bench_fast: no GPU -- a time measured anywhere else says nothing")
W, H, B, M = 640, 480, 20, 20


def blobs_image(seed):
    """Gaussian blobs (sigma 1.5 ... 5 px) on grey, each added on its own 8-sigma patch (the image of tools/bench_klt.py)."""
    rng = np.random.default_rng(seed)
    n = 4000
    cx, cy = rng.uniform(-10, W + 10, n), rng.uniform(-10, H + 10, n)
    sig, amp = rng.uniform(1.5, 5.0, n), rng.uniform(25.0, 70.0, n) * rng.choice([-1.0, 1.0], n)
    v = np.full((H, W), 128.0)
    for x0, y0, s, a in zip(cx, cy, sig, amp):
        xa, xb, ya, yb = max(int(x0 - 4 * s), 0), min(int(x0 + 4 * s) + 2, W), max(int(y0 - 4 * s), 0), min(int(y0 + 4 * s) + 2, H)
        if xa < xb and ya < yb:
            y, x = np.mgrid[ya:yb, xa:xb]
            v[ya:yb, xa:xb] += a * np.exp(-((x - x0) ** 2 + (y - y0) ** 2) / (2 * s * s))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


im = blobs_image(7)
eng = engine.Engine(4, 0, 4)
klt = tracker.Klt(eng, 1024, W, H)
stream = torch.cuda.ExternalStream(eng.L.xk_stream(eng.h))
klt.push_image(im)


def timed(fn):
    out = []
    for rep in range(3):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record(stream)
        for i in range(args.calls):
            fn(i)
        ev1.record(stream)
        ev1.synchronize()
        out.append((ev0.elapsed_time(ev1) / args.calls, 1e3 * (time.perf_counter() - t0) / args.calls))
    return (" / ".join(f"{e:6.3f}" for e, _ in out) + " ms per call (HIP events, three repeats), " + " / ".join(f"{w:6.3f}" for _, w in out)
            + " ms host wall")


# max_candidates 16384: the keys and the blocked mask share the LDS; 32768: the mask lives in global memory
for threshold, cap in ((9, 16384), (30, 16384), (9, 32768)):
    klt.detect_setup(threshold, True, B, M, cap)
    for n_old in (0, 200):
        rng = np.random.default_rng(n_old)
        old = np.stack([rng.uniform(0, W - 1, n_old), rng.uniform(0, H - 1, n_old)], axis=1)
        for w in range(20):
            got = klt.detect(1, old)
        line = f"detect {W} x {H}, threshold {threshold:2d}, max_candidates {cap:5d}, n_old {n_old:3d}: " + timed(lambda i: klt.detect(1, old))
        line += f", {got['n_candidates']} candidates, {len(got['xy'])} accepted"
        if not args.no_cpu:
            t0 = time.perf_counter()
            ref = fnp.detect(im, threshold, 1, B, M, old)
            cpu = time.perf_counter() - t0
            line += (f";  NumPy restatement, one core: {1e3 * cpu:8.1f} ms, bit-equal: "
                     f"{np.array_equal(ref['xy'], got['xy']) and np.array_equal(ref['score'], got['score'])}")
        print(line, flush=True)
klt.close()
eng.close()
