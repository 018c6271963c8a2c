"""Cost of the photometric calibration on the GPU box, on a pair of 640 x 480 images: milliseconds per
xk_trk_photo_calibrate (features and intensities in, raw tracking, intensities, gain estimate, correction and pyramid rebuild,
results out, one synchronisation) with 100 and 400 features; the correction plus pyramid rebuild alone (xk_trk_photo_correct, waited
for) beside xk_trk_push_image on the same image; and what the second plane adds to a push (push with against push without a photo
setup, two xk_trk in one process, interleaved).  Timed with HIP events on the handle's stream over --calls calls after 20 (repeated
three times: the spread is printed):
    python tools/bench_photo.py [--calls 200]
The per-kernel split -- and with it the correction kernel's achieved bandwidth against the bytes it must move, W H (1 + 1 + 4) --
comes from a run of its own under the profiler (tracing slows the host, so the times above are taken without it):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/bench_photo.py --calls 50
    python tools/bench_photo.py --kernel-stats DIR"""
import argparse, csv, glob, os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

W, H = 640, 480
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--kernel-stats", metavar="DIR", help="print the xk_photo_* and xk_klt_* rows of a rocprofv3 --kernel-trace --stats run and exit")
args = ap.parse_args()
if args.kernel_stats:
    files = glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit("bench_photo: no *kernel_stats.csv under " + args.kernel_stats)
    for r in csv.DictReader(open(files[0])):
        if "xk_photo" in r["Name"] or "xk_klt" in r["Name"]:
            line = (f"{r['Name'][:40]:40s} calls {r['Calls']:>6s} avg_us {float(r['AverageNs']) / 1e3:8.2f} min_us {float(r['MinNs']) / 1e3:8.2f} "
                    f"max_us {float(r['MaxNs']) / 1e3:8.2f}")
            if "xk_photo_correct" in r["Name"]:
                line += f"  -> {6 * W * H / float(r['AverageNs']):6.1f} GB/s of the {6 * W * H} bytes it must move (at the average)"
            print(line)
    sys.exit(0)

import torch
import fast_cases as fc
import photo_np as pnp
from x_multi_agent_amd import engine, tracker

if not torch.cuda.is_available():
    sys.exit("bench_photo: no GPU -- a time measured anywhere else says nothing")
im1 = np.ascontiguousarray(fc.boxes_image(W, H, 7, 260))
im2 = np.zeros_like(im1)
im2[1:, 2:] = im1[:-1, :-2]                                        # shifted by (2, 1) ...
im2 = np.clip(np.rint(0.9 * im2.astype(np.float64) + 12.0), 0, 255).astype(np.uint8)   # ... and 0.9 v + 12
eng = engine.Engine(4, 0, 4)
klt = tracker.Klt(eng, 1024, W, H)
plain = tracker.Klt(eng, 1024, W, H)                               # no photo setup: the push as it was
stream = torch.cuda.ExternalStream(eng.L.xk_stream(eng.h))
klt.detect_setup(9, True, 8, 31, 16384)
klt.photo_setup(30, 0.0, 0.0, 512)
klt.photo_set_spatial(np.random.default_rng(2).uniform(-0.02, 0.02, (H, W)).astype(np.float32))
klt.push_image(im1)
feats = klt.detect(1)["xy"]
klt.push_image(im2)
plain.push_image(im1)
plain.push_image(im2)


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


print(f"{len(feats)} features detected in the first image", flush=True)
for n in (100, 400):
    if len(feats) < n:
        print(f"calibrate: only {len(feats)} features, {n} skipped")
        continue
    xy = feats[:n].astype(np.float32)
    val = klt.photo_intensity(feats[:n], 0, 0)[0]
    for w in range(20):
        got = klt.photo_calibrate(xy, val, None, w)
    line = f"calibrate {W} x {H}, {n:4d} features, {min(n, 512)} hypotheses: " + timed(lambda i: klt.photo_calibrate(xy, val, None, i))
    print(line + f", {len(got['keep_idx'])} kept, support {got['support']}, a {got['a_rel']:.4f} b {got['b_rel']:.4f}", flush=True)
    klt.photo_reset()


def correct_waited(i):
    klt.photo_correct(1)
    stream.synchronize()


def push_waited(k):
    k.push_image(im2)
    stream.synchronize()


for w in range(20):
    correct_waited(w), push_waited(klt), push_waited(plain)
img = klt.level(1, 0)[0]
print("correction + pyramid rebuild, waited for : " + timed(correct_waited), flush=True)
for rep in range(2):                                               # both orders
    print("push_image with the raw plane, waited for: " + timed(lambda i: push_waited(klt)), flush=True)
    print("push_image without a photo setup, waited : " + timed(lambda i: push_waited(plain)), flush=True)
klt.close()
plain.close()
eng.close()
