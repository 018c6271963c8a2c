"""Cost of the per-frame feature tracking on the GPU box: milliseconds per xk_trk_push_image (one 640 x 480 image
through the pinned staging, its pyramid and derivatives: 1 copy + 5 launches) and per xk_trk_track (host buffers in and out,
one launch pair, one synchronisation) at n = 100 and 400, window 31 x 31, max_level 2, timed separately with HIP events on the
handle's stream over --calls calls after warm-up (repeated three times: the spread is printed); the upload of the image alone
(the same bytes, pinned to device, on a stream of its own) is timed beside push_image, whose figure contains it; and one core's
time for the NumPy restatement:
    python tools/bench_klt.py [--calls 200]
The per-kernel split comes from a run of its own under the profiler (tracing slows the host, so the times above are taken
without it):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/bench_klt.py --calls 50 --no-cpu
    python tools/bench_klt.py --kernel-stats DIR"""
import argparse, csv, glob, os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--no-cpu", action="store_true", help="skip the NumPy restatement (profiler runs)")
ap.add_argument("--kernel-stats", metavar="DIR", help="print the xk_klt_* rows of a rocprofv3 --kernel-trace --stats run and exit")
args = ap.parse_args()
if args.kernel_stats:
    files = glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit("bench_klt: no *kernel_stats.csv under " + args.kernel_stats)
    for r in csv.DictReader(open(files[0])):
        if "xk_klt" in r["Name"]:
            print(f"{r['Name'][:40]:40s} calls {r['Calls']:>6s} avg_us {float(r['AverageNs']) / 1e3:8.2f} min_us {float(r['MinNs']) / 1e3:8.2f} "
                  f"max_us {float(r['MaxNs']) / 1e3:8.2f}")
    sys.exit(0)

import torch
import klt_np as knp
from x_multi_agent_amd import engine, tracker

if not torch.cuda.is_available():
    sys.exit("bench_klt: no GPU -- a time measured anywhere else says nothing")
W, H, WIN, MAX_LEVEL = 640, 480, (31, 31), 2


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


shift = (3.3, -2.1)
im1, im2 = blobs_image(7, (0.0, 0.0)), blobs_image(7, shift)
eng = engine.Engine(4, 0, 4)
klt = tracker.Klt(eng, 512, W, H, WIN, MAX_LEVEL)
stream = torch.cuda.ExternalStream(eng.L.xk_stream(eng.h))


def timed(fn, stream=stream):
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


pair = (im1, im2)
for w in range(20):
    klt.push_image(pair[w & 1])
print(f"push_image {W} x {H}, levels {klt.levels()}: " + timed(lambda i: klt.push_image(pair[i & 1])), flush=True)
# the upload alone on a stream of torch's own: its allocators remember every stream a pinned block was used on and record an
# event there when the block is freed, which must not be the handle's stream -- that one is gone once the engine is closed
own = torch.cuda.Stream()
pinned, dev = torch.from_numpy(im1.copy()).pin_memory(), torch.empty((H, W), dtype=torch.uint8, device="cuda")
with torch.cuda.stream(own):
    for w in range(20):
        dev.copy_(pinned, non_blocking=True)
    print(f"  of which the upload of {W * H} bytes alone: " + timed(lambda i: dev.copy_(pinned, non_blocking=True), own), flush=True)
own.synchronize()
del pinned, dev
klt.push_image(im1)
klt.push_image(im2)
for n in (100, 400):
    rng = np.random.default_rng(n)
    pts = np.stack([rng.uniform(30, W - 31, n), rng.uniform(30, H - 31, n)], axis=1).astype(np.float32)
    for w in range(20):
        got = klt.track(pts)
    line = f"track n = {n:3d}: " + timed(lambda i: klt.track(pts))
    err = np.linalg.norm(got["cur_xy"] - (pts + np.float32(shift)), axis=1)
    line += f", {len(got['keep_idx'])} kept, median error {np.median(err):.3f} px"
    if not args.no_cpu:
        p1, p2 = knp.build_pyramid(im1, WIN, MAX_LEVEL), knp.build_pyramid(im2, WIN, MAX_LEVEL)
        t0 = time.perf_counter()
        ref = knp.track(p1, p2, pts, WIN)
        cpu = time.perf_counter() - t0
        line += (f";  NumPy restatement, one core: {1e3 * cpu:8.1f} ms, same status: {np.array_equal(ref['status'], got['status'])}, "
                 f"max |d position| {np.abs(ref['cur_xy'] - got['cur_xy']).max():.1e}")
    print(line, flush=True)
klt.close()
eng.close()
