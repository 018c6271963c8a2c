"""Cost of manageTracks on the device-resident track store (xk_trk_tracks_manage) on the workload of
tools/bench_track_manager.py: a window of N = 30 poses, 440 features (about 400 matches a frame), 20 persistent features,
min_track_length 5, 4 x 4 tiles on 640 x 480, the same synthetic stream from the same seed.  Every frame's call is timed on the host
with the steady clock around the C entry alone (it ends in its one wait; the arrays are allocated before the clock starts).  The first
--warmup frames fill the window and are left out; three repeats, each on a fresh store:
    python tools/bench_resident_tracks.py [--frames 120] [--warmup 40] [--repeats 3]
The kernels' own times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/bench_resident_tracks.py --repeats 1"""
import argparse, ctypes as C, os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=120)
ap.add_argument("--warmup", type=int, default=40)
ap.add_argument("--features", type=int, default=440)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
if not os.path.exists("/dev/kfd"):
    sys.exit("bench_resident_tracks: no GPU -- a time measured anywhere else says nothing")
from x_multi_agent_amd import engine, tracker
from x_multi_agent_amd.engine import c_dp, c_ip

W, H, N, N_SLAM, MIN_LEN, MAX_TRACKS = 640, 480, 30, 20, 5, 1024
K = (0.625 * W, 0.75 * H, 0.5 * W, 0.5 * H)
rng = np.random.default_rng(5)
n = args.features
xy = np.stack([rng.uniform(5, W - 5, n), rng.uniform(5, H - 5, n)], axis=1)
vel = rng.normal(scale=0.6, size=(n, 2)) + np.array([2.5, 0.4])          # a pan plus each feature's own parallax
score = rng.uniform(20, 250, n)
seen = np.ones(n, bool)
yaw, quats, frames = 0.0, [], []
for f in range(args.frames):                                             # the stream of bench_track_manager.py, draw for draw
    prev, was = xy.copy(), seen.copy()
    xy = xy + vel + rng.normal(scale=0.05, size=(n, 2))
    gone = (xy[:, 0] < 2) | (xy[:, 0] > W - 2) | (xy[:, 1] < 2) | (xy[:, 1] > H - 2)
    xy[gone] = np.stack([rng.uniform(5, 60, gone.sum()), rng.uniform(5, H - 5, gone.sum())], axis=1)
    seen = ~gone & (rng.uniform(size=n) > 0.04)
    yaw += 0.004
    quats.append([0.0, np.sin(yaw / 2), 0.0, np.cos(yaw / 2)])
    both = np.flatnonzero(was & seen & ~gone)
    both = both[np.argsort(-score[both], kind="stable")]
    rots = np.array([quats[max(0, g)] for g in range(f - N + 1, f + 1)], np.float64)
    frames.append((np.ascontiguousarray(prev[both]), np.ascontiguousarray(xy[both]), score[both].astype(np.int32), rots))

eng = engine.Engine(4, 0, 4)
mf = tracker.MatchFilter(eng, 512, K, 0.0)
k = tracker.Klt(eng, 0, W, H, (15, 15), 0, match_filter=mf)
cap_e, cap_o = MAX_TRACKS + 512, (MAX_TRACKS + 512) * 64
lost, claimed = np.zeros(MAX_TRACKS, np.int32), np.zeros(512, np.uint8)
ids, off, out_xy = np.zeros(cap_e, np.int64), np.zeros(cap_e + 1, np.int32), np.zeros((cap_o, 2))
for rep in range(args.repeats):
    k.tracks_setup(MAX_TRACKS, 4, 4, W, H, 0.05, 0.05)
    ms, counts = [], []
    for prev, cur, sc, rots in frames:
        o = tracker.TracksOut()
        o.cap_lost, o.cap_entries, o.cap_obs = MAX_TRACKS, cap_e, cap_o
        o.lost_slam_idxs, o.claimed = lost.ctypes.data_as(c_ip), claimed.ctypes.data_as(tracker.c_ub)
        o.ids, o.off, o.xy = ids.ctypes.data_as(tracker.c_lp), off.ctypes.data_as(c_ip), out_xy.ctypes.data_as(c_dp)
        a = (k.p, prev.ctypes.data_as(c_dp), cur.ctypes.data_as(c_dp), prev.ctypes.data_as(c_dp), cur.ctypes.data_as(c_dp), sc.ctypes.data_as(c_ip),
             C.c_int(len(sc)), rots.ctypes.data_as(c_dp), C.c_int(len(rots)), C.c_int(N), C.c_int(N_SLAM), C.c_int(MIN_LEN), None, None, C.byref(o))
        t0 = time.perf_counter_ns()
        rc = eng.L.xk_trk_tracks_manage(*a)
        ms.append((time.perf_counter_ns() - t0) * 1e-6)
        if rc != 0:
            sys.exit("bench_resident_tracks: xk_trk_tracks_manage failed: %d" % rc)
        counts.append((len(sc), o.n_candidates, o.n_candidate_obs, sum(o.n_list[:4])))
    v, c = np.array(ms[args.warmup:]), np.array(counts[args.warmup:], np.float64)
    print(f"repeat {rep}: {len(v)} frames, {c[:, 0].mean():.0f} matches, {c[:, 1].mean():.0f} candidate tracks with {c[:, 2].mean():.0f} observations a frame, "
          f"{c[:, 3].mean():.1f} measurement tracks handed out a frame | xk_trk_tracks_manage median {np.median(v):7.4f} min {v.min():7.4f} max {v.max():7.4f} ms",
          flush=True)
k.close()
mf.close()
eng.close()
