"""Cost of x::TrackManager::manageTracks on the GPU box: a window of N = 30 poses, about 400 matches a frame, 20
persistent features, 4 x 4 tiles, on a synthetic stream (features drifting across a 640 x 480 image with a slow pan, 4 % of them
lost every frame and detected again).  The C++ mirror (xk_track_manager_example) times every frame itself with the steady clock:
the whole of manageTracks, and inside it the one xk_trk_baseline call (copy in, launch, copy out, wait); the host list work is the
difference.  The first --warmup frames fill the window and are left out; the run is repeated three times and the spread printed:
    python tools/bench_track_manager.py [--frames 120] [--warmup 40]
The kernel's own time comes from a run of its own under the profiler, on the same case:
    python tools/bench_track_manager.py --keep-case case.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- x_multi_agent_amd/xk_track_manager_example case.txt"""
import argparse, os, subprocess, sys, tempfile
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "x_multi_agent_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=120)
ap.add_argument("--warmup", type=int, default=40)
ap.add_argument("--features", type=int, default=440)
ap.add_argument("--keep-case", metavar="PATH", help="also write the case file there, e.g. for a profiler run of the example on it")
args = ap.parse_args()
if not os.path.exists("/dev/kfd"):
    sys.exit("bench_track_manager: no GPU -- a time measured anywhere else says nothing")
exe = os.path.join(PKG, "xk_track_manager_example")
if not os.path.exists(exe):
    sys.exit("bench_track_manager: build first (python -m x_multi_agent_amd.build)")

W, H, N = 640, 480, 30
rng = np.random.default_rng(5)
n = args.features
xy = np.stack([rng.uniform(5, W - 5, n), rng.uniform(5, H - 5, n)], axis=1)
vel = rng.normal(scale=0.6, size=(n, 2)) + np.array([2.5, 0.4])          # a pan plus each feature's own parallax
score = rng.uniform(20, 250, n)
seen = np.ones(n, bool)
yaw = 0.0
quats = []
rows = [f"0.625 0.75 0.5 0.5 0.0 {W} {H} 0.05 0.05 1024 0 {N} 20 5 4 4 {args.frames}"]
for f in range(args.frames):
    prev, was = xy.copy(), seen.copy()
    xy = xy + vel + rng.normal(scale=0.05, size=(n, 2))
    gone = (xy[:, 0] < 2) | (xy[:, 0] > W - 2) | (xy[:, 1] < 2) | (xy[:, 1] > H - 2)
    xy[gone] = np.stack([rng.uniform(5, 60, gone.sum()), rng.uniform(5, H - 5, gone.sum())], axis=1)     # a new feature enters
    seen = ~gone & (rng.uniform(size=n) > 0.04)
    yaw += 0.004
    quats.append([0.0, np.sin(yaw / 2), 0.0, np.cos(yaw / 2)])
    both = np.flatnonzero(was & seen & ~gone)
    both = both[np.argsort(-score[both], kind="stable")]
    rots = [quats[max(0, g)] for g in range(f - N + 1, f + 1)]
    rows.append(f"{len(both)} {N} 0 320.0 240.0")
    rows.extend(" ".join(repr(float(v)) for v in (prev[i, 0], prev[i, 1], prev[i, 0], prev[i, 1], xy[i, 0], xy[i, 1], xy[i, 0], xy[i, 1], score[i]))
                for i in both)
    rows.extend(" ".join(repr(float(v)) for v in q) for q in rots)
    rows.append("")

env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
with tempfile.TemporaryDirectory() as d:
    case = os.path.join(d, "case.txt")
    open(case, "w").write("\n".join(rows) + "\n")
    if args.keep_case:
        open(args.keep_case, "w").write("\n".join(rows) + "\n")
    for rep in range(3):
        r = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
        if r.returncode != 0:
            sys.exit("bench_track_manager: the example failed: " + r.stderr)
        F = np.array([[float(v) for v in line.split()[1:]] for line in r.stdout.splitlines() if line.startswith("F ")])[args.warmup:]
        per_frame = []                                                 # measurement tracks handed out, frame by frame
        for line in r.stdout.splitlines():
            if line.startswith("F "):
                per_frame.append(0)
            elif line.startswith(("T msckf", "T short", "T new_")):
                per_frame[-1] += 1
        handed_out = float(np.mean(per_frame[args.warmup:]))
        dev, tot, host = F[:, 1], F[:, 2], F[:, 2] - F[:, 1]
        q = lambda v: f"median {np.median(v):7.4f} min {v.min():7.4f} max {v.max():7.4f} ms"
        print(f"repeat {rep}: {len(F)} frames, {F[:, 3].mean():.0f} matches, {F[:, 4].mean():.0f} candidate tracks with {F[:, 5].mean():.0f} observations a frame, {handed_out:.1f} measurement tracks handed out a frame | manageTracks {q(tot)} | "
              f"device call {q(dev)} | host list work {q(host)}", flush=True)
