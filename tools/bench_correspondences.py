"""Cost of findCorrespondences as one call (xk_pr_find_correspondences) beside the chain of stage calls it
replaces, on the GPU box, in one process and alternating the two routes call by call:
    one call   Database.find_correspondences: one copy in, six launches, one result block out, one wait
    chain      knn_match -> ratio test -> essential_ransac -> good_matches with the mask -> classify: two round trips, two
               waits, the list work on the host
n_rec = n_cur = 100 and 300, 30 % wrong rows, n_hyp = 1024; >= 200 calls of each route after warm-up, every call between
two HIP events on the handle's stream, three repeats for the spread.  The chain's list work here is PYTHON (place.py), far
slower than the C++ mirror's: so the chain is reported twice, its two device entries alone and with the list work, and the
saving is stated against the device entries alone -- a lower bound.  Both routes must give the same `good` list.
    python tools/bench_correspondences.py [--calls 200] [--kernel-stats DIR]
--kernel-stats DIR: afterwards, one more run of this tool in a child process under rocprofv3 --kernel-trace --stats,
writing to DIR, and the per-kernel rows of its statistics."""
import argparse, glob, os, subprocess, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import torch
import correspond_np as cnp
from x_multi_agent_amd import engine, place, synth

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--n-hyp", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--kernel-stats", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_correspondences: no GPU -- a time measured anywhere else says nothing")


def make(n):
    rng = np.random.default_rng(70 + n)
    land = rng.permutation(n)
    rows = rng.choice(n, int(round(0.3 * n)), replace=False)
    wrong = {int(q): int(land[p]) for q, p in zip(rows, np.roll(rows, 1))}
    return cnp.make_case(n, n, land, wrong, (n // 3, n // 3, n // 3, n // 3), args.n_hyp, 50 + n, max_desc=512)


eng = engine.Engine(4, 0, 4)
db = place.Database(eng, synth.make_vocabulary(4, 2, 32, seed=8), 0.6, max_desc=512)
stream = torch.cuda.ExternalStream(eng.L.xk_stream(eng.h))


def one_call(c, seed):
    return db.find_correspondences(c["rec_desc"], c["rec_px"], c["cur_desc"], c["cur_px"], c["counts"], cnp.MIN_D, cnp.RATIO,
                                   c["K"], cnp.THR, args.n_hyp, seed)


def chain(c, seed, ev):
    """-> (good, classified); ev: three events, recorded before the match, after the essential filter's wait, at the end."""
    idx, dist = db.knn_match(c["rec_desc"], c["cur_desc"])
    cand = cnp.ratio_test(idx, dist)
    cp = np.array([c["cur_px"][t] for _, t in cand], np.float32)
    rp = np.array([c["rec_px"][q] for q, _ in cand], np.float32)
    ev[1].record(stream)                                       # (the gather above is list work: taken out below)
    mask, E, _ = db.essential_ransac(cp, rp, c["K"], cnp.THR, args.n_hyp, seed)
    ev[2].record(stream)
    good = place.good_matches(idx, dist, cnp.MIN_D, cnp.RATIO, inlier_mask=mask)
    return good, place.classify(good, *c["counts"])


def events(k):
    return [torch.cuda.Event(enable_timing=True) for _ in range(k)]


for n in (100, 300):
    c = make(n)
    for w in range(20):
        one_call(c, w)
        chain(c, w, events(3))
    rows = []
    for rep in range(args.repeats):
        eo, ec = [events(2) for _ in range(args.calls)], [events(4) for _ in range(args.calls)]
        for i in range(args.calls):                            # alternating: what disturbs one route disturbs the other
            eo[i][0].record(stream)
            got = one_call(c, i)
            eo[i][1].record(stream)
            ec[i][0].record(stream)
            good, cls = chain(c, i, ec[i])
            ec[i][3].record(stream)
        torch.cuda.synchronize()
        assert got["status"] == 0 and [tuple(m) for m in got["good"].tolist()] == good, "the routes disagree on the timed scene"
        assert [(cnp.KIND[k], a, b) for k, a, b in cls] == [tuple(m) for m in got["classified"].tolist()]
        one = sum(a.elapsed_time(b) for a, b in eo) / args.calls
        full = sum(e[0].elapsed_time(e[3]) for e in ec) / args.calls
        # the chain's device entries alone: the essential entry between its own two events, and the match entry timed by
        # itself below (inside the chain its events would also span the Python ratio test and gather)
        ess = sum(e[1].elapsed_time(e[2]) for e in ec) / args.calls
        ek = [events(2) for _ in range(args.calls)]
        for i in range(args.calls):
            ek[i][0].record(stream)
            db.knn_match(c["rec_desc"], c["cur_desc"])
            ek[i][1].record(stream)
        torch.cuda.synchronize()
        knn = sum(a.elapsed_time(b) for a, b in ek) / args.calls
        rows.append((one, knn + ess, full))
    r = np.array(rows)
    spread = lambda v: f"{np.median(v):7.4f} ms (min {v.min():.4f}, max {v.max():.4f})"
    print(f"n = {n:3d}, n_hyp = {args.n_hyp}, {args.calls} calls x {args.repeats} repeats, {len(good)} good matches")
    print(f"  one call                            {spread(r[:, 0])}")
    print(f"  chain, its two device entries alone {spread(r[:, 1])}")
    print(f"  chain with the Python list work     {spread(r[:, 2])}")
    print(f"  device entries alone - one call     {spread(r[:, 1] - r[:, 0])}   (lower bound of the saving)")
db.close()
eng.close()

if args.kernel_stats:
    os.makedirs(args.kernel_stats, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.kernel_stats, "--", sys.executable, os.path.abspath(__file__),
           "--calls", str(min(args.calls, 50)), "--repeats", "1", "--n-hyp", str(args.n_hyp)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit("rocprofv3 run failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    for path in sorted(glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)):
        print("per-kernel statistics,", path)
        for line in open(path):
            if line.startswith('"Name"') or "xk_" in line:
                print("  " + line.rstrip())
