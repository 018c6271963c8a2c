"""Cost of the essential-matrix RANSAC filter on the GPU box: milliseconds per xk_pr_essential_ransac call
(host buffers in and out, three launches, one synchronisation) at n = 100 and n = 300 with n_hyp = 1024, timed with HIP
events on the handle's stream over >= 200 calls after warm-up, and one core's time for the NumPy restatement beside it:
    python tools/bench_essential.py [--calls 200]"""
import argparse, os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import torch
import essential_np as enp
from x_multi_agent_amd import engine, place, synth

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--n-hyp", type=int, default=1024)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_essential: no GPU -- a time measured anywhere else says nothing")
eng = engine.Engine(4, 0, 4)
db = place.Database(eng, synth.make_vocabulary(4, 2, 32, seed=8), 0.6, max_desc=512)
stream = torch.cuda.ExternalStream(eng.L.xk_stream(eng.h))
for n in (100, 300):
    cur, rec, _, _, K = enp.make_scene(n, 0.4, 0.3, 50 + n)
    for w in range(20):
        db.essential_ransac(cur, rec, K, 1.0, args.n_hyp, w)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record(stream)
    for i in range(args.calls):
        mask, E, n_inl = db.essential_ransac(cur, rec, K, 1.0, args.n_hyp, i)
    ev1.record(stream)
    ev1.synchronize()
    wall = (time.perf_counter() - t0) / args.calls
    t0 = time.perf_counter()
    ref = enp.ransac(cur, rec, *K, 1.0, args.n_hyp, args.calls - 1)
    cpu = time.perf_counter() - t0
    assert np.array_equal(ref["mask"], mask), "device and restatement disagree on the timed scene"
    print(f"n = {n:3d}, n_hyp = {args.n_hyp}: {ev0.elapsed_time(ev1) / args.calls:7.3f} ms per call (HIP events), "
          f"{1e3 * wall:7.3f} ms host wall, {n_inl} inliers;  NumPy restatement, one core: {1e3 * cpu:8.1f} ms")
db.close()
eng.close()
