"""Cost of the range-facet / sun-angle rows (xk_stage_range, xk_stage_sun_angle): one staged update timed with xk_bench_staged (HIP events
on the handle's stream, averaged per update) with and without the rows, on BASELINE config 4 + sun and config 2 + range + sun.
Prints one JSON line per case.  bench.py is not involved.

    python tools/bench_aux_rows.py [--steps 200] [--warmup 20]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from x_multi_agent_amd import engine, synth  # noqa: E402


def _stage(eng, sc, rm, sun):
    eng.stage(sc)
    if rm is not None:
        eng.stage_range(rm["range"], rm["img_pt"], rm["facet"], rm["sigma_range"])
    if sun is not None:
        eng.stage_sun_angle(sun["q"], sun["x"], sun["y"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    for cfg, with_range in ((4, False), (2, True)):
        sc = synth.make_config(cfg)
        N, K, M = synth.CONFIGS[cfg]
        rm = synth.make_range(sc, (0, 1, 2)) if with_range else None
        sun = synth.make_sun(11)
        eng = engine.Engine(N, M, K)
        res = {"plain": [], "aux": []}
        for _ in range(a.repeats):               # interleaved: clock and neighbour drift hit both alike
            for key in ("plain", "aux"):
                _stage(eng, sc, rm if key == "aux" else None, sun if key == "aux" else None)
                t = eng.bench_staged(sc["sigma_img"], a.warmup, a.steps)
                res[key].append(t["total_ms"])
        eng.close()
        p, x = min(res["plain"]), min(res["aux"])
        print(json.dumps(dict(config=cfg, rows="range+sun" if with_range else "sun", n=15 + 6 * N + 3 * M, plain_ms=round(p, 4),
                              aux_ms=round(x, 4), delta_ms=round(x - p, 4), plain_all=res["plain"], aux_all=res["aux"])))


if __name__ == "__main__":
    main()
