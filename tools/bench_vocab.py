"""Cost of training a vocabulary (xk_voc_train) on the GPU box: the descriptors are on the device before the
clock starts, the tree arrays are read afterwards; with the NumPy restatement (tests/vocab_np.py, one host core) beside it up
to --numpy-max descriptors:  python tools/bench_vocab.py [--sizes 10000,100000,1000000] [--numpy-max 100000] [--out FILE]"""
import argparse, json, os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import vocab_cases as vc
import vocab_np as vnp
from x_multi_agent_amd import engine, place

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="10000,100000,1000000")
ap.add_argument("--numpy-max", type=int, default=100000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

eng = engine.Engine(4, 0, 4)
rows = []
for n in [int(s) for s in args.sizes.split(",")]:
    d = vc.clustered(n, 32, centres=max(12, n // 50), seed=3)
    for k, L in ((4, 3), (10, 4)):
        tr = place.VocabularyTrainer(eng, k, L, 32, max_desc=n)
        tr.add(d)
        voc = tr.train(0, 100)                         # warm: buffers of every level exist afterwards
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter(); voc = tr.train(0, 100); ts.append(time.perf_counter() - t0)
        tr.close()
        oc = voc["outcome"]
        row = dict(n=n, k=k, L=L, ms=1e3 * float(np.median(ts)), n_nodes=oc["n_nodes"], n_words=oc["n_words"],
                   passes=oc["level_passes"], nodes=oc["level_nodes"], capped=oc["capped_nodes"], launches=oc["launches"],
                   host_waits=oc["host_waits"], numpy_ms=None)
        if n <= args.numpy_max:
            t0 = time.perf_counter(); ref = vnp.train(d, k, L, 0, 100); row["numpy_ms"] = 1e3 * (time.perf_counter() - t0)
            row["equal"] = bool(all(np.array_equal(voc[key], ref[key]) for key in ("desc", "children", "word_of_node", "node_of_word")))
        rows.append(row)
        print(f"N = {n:8d}  k = {k:2d} L = {L}  GPU path {row['ms']:9.2f} ms   nodes {oc['n_nodes']:6d} words {oc['n_words']:6d}  "
              f"passes {oc['level_passes']}  launches {oc['launches']:4d}  host waits {oc['host_waits']:3d}  capped {oc['capped_nodes']}"
              + (f"   NumPy restatement {row['numpy_ms']:10.1f} ms (equal: {row['equal']})" if row["numpy_ms"] is not None else ""),
              flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(rows, f)
eng.close()
