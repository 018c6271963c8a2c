"""Cost of the description on the GPU box, on one 640 x 480 image: milliseconds per xk_trk_describe (keypoints in,
filter and description, the result block out, one synchronisation) at 100, 400 and 3000 keypoints with a fixed angle and with the
intensity centroid; the blur alone (push_image + describe_stage against push_image alone: the difference holds the blur and the
copy of G to the host, so the kernel's own time is the profiler's); and xk_trk_detect on the same image in the same run as the
yardstick.  Timed with HIP events on the handle's stream over --calls calls after 20 (repeated three times: the spread is printed):
    python tools/bench_orb.py [--calls 200]
The per-kernel split comes from a run of its own under the profiler (tracing slows the host, so the times above are taken
without it):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/bench_orb.py --calls 50
    python tools/bench_orb.py --kernel-stats DIR"""
import argparse, csv, glob, os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--kernel-stats", metavar="DIR", help="print the xk_orb_* and xk_fast_* rows of a rocprofv3 --kernel-trace --stats run and exit")
args = ap.parse_args()
if args.kernel_stats:
    files = glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit("bench_orb: no *kernel_stats.csv under " + args.kernel_stats)
    for r in csv.DictReader(open(files[0])):
        if "xk_orb" in r["Name"] or "xk_fast" in r["Name"]:
            print(f"{r['Name'][:40]:40s} calls {r['Calls']:>6s} avg_us {float(r['AverageNs']) / 1e3:8.2f} min_us {float(r['MinNs']) / 1e3:8.2f} "
                  f"max_us {float(r['MaxNs']) / 1e3:8.2f}")
    sys.exit(0)

import torch
import fast_cases as fc
import orb_np as onp
from x_multi_agent_amd import engine, tracker

if not torch.cuda.is_available():
    sys.exit("bench_orb: no GPU -- a time measured anywhere else says nothing")
W, H, EDGE = 640, 480, 31
im = np.ascontiguousarray(fc.boxes_image(W, H, 7, 260))
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


klt.detect_setup(9, True, 20, EDGE, 16384)
for w in range(20):
    det = klt.detect(1)
print(f"detect {W} x {H}, threshold 9 (the yardstick): " + timed(lambda i: klt.detect(1)) + f", {det['n_candidates']} candidates, {len(det['xy'])} accepted",
      flush=True)

rng = np.random.default_rng(1)
for mode, label in ((0, "fixed angle -1"), (1, "intensity centroid")):
    klt.describe_setup(mode, -1.0, EDGE, None, 4096)
    for n in (100, 400, 3000):
        pts = np.stack([rng.integers(EDGE, W - EDGE, n), rng.integers(EDGE, H - EDGE, n)], axis=1).astype(np.int32)
        for w in range(20):
            got = klt.describe(pts, 1)
        line = f"describe {W} x {H}, {label:18s}, {n:4d} keypoints: " + timed(lambda i: klt.describe(pts, 1)) + f", {len(got['keep_idx'])} kept"
        if n == 100:
            ref = onp.describe(im, pts, onp.default_pattern(), EDGE, mode)
            line += f";  bit-equal to the NumPy restatement: {all(np.array_equal(ref[k], got[k]) for k in ('keep_idx', 'moments', 'dir', 'desc'))}"
        print(line, flush=True)

# the blur: a push invalidates it, the stage recomputes it (and copies G out); the push alone beside it
for w in range(20):
    klt.push_image(im)
    klt.describe_stage(1)
print(f"push_image alone               : " + timed(lambda i: klt.push_image(im)), flush=True)
print(f"push_image + blur + G to host  : " + timed(lambda i: (klt.push_image(im), klt.describe_stage(1))), flush=True)
klt.close()
eng.close()
