"""host/examples/lmeds_main.cpp -- x::MatchFilter and x::Tracker under outlier_method 4 (cv::LMEDS), 8 (cv::RANSAC) and another
value -- against tracker.MatchFilter.filter_matches and tracker.Klt.frame under the same method: kept indices, coordinates, median
and sigma, bit for bit.  Every value but 4 is RANSAC, as before."""
import os
import subprocess

import numpy as np
import pytest

import fundamental_cases as fc
import fundamental_np as fnp
import klt_cases as kc
import lmeds_cases as lc
import tracker_frame_cases as tc

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(__file__), "..", "x_multi_agent_amd")


def example():
    exe = os.path.join(PKG, "xk_lmeds_example")
    if not os.path.exists(exe):
        from x_multi_agent_amd import build
        build.build_host()
    return exe, dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))


def test_cpp_match_filter_follows_the_method(tmp_path):
    exe, env = example()
    n, share, noise, n_hyp, scene_seed = lc.DISTORTED_CASES[0]
    seed = 4
    p, c, _ = fc.pair(n, share, noise, scene_seed, "general", lc.S_FOV)
    frac = (lc.K[0] / fnp.WIDTH, lc.K[1] / fnp.HEIGHT, lc.K[2] / fnp.WIDTH, lc.K[3] / fnp.HEIGHT)
    Kc = (fnp.WIDTH * frac[0], fnp.HEIGHT * frac[1], fnp.WIDTH * frac[2], fnp.HEIGHT * frac[3])
    eng = engine.Engine(4, 0, 4)
    mf = tracker.MatchFilter(eng, lc.MAX_MATCHES, Kc, lc.S_FOV)
    want = {}
    mf.outlier_method(lc.LMEDS)
    want[lc.LMEDS] = mf.filter_matches(p, c, fc.THR, n_hyp, seed) + (mf.fundamental_medians(0, 0)[1],)
    mf.outlier_method(lc.RANSAC)
    want[lc.RANSAC] = mf.filter_matches(p, c, fc.THR, n_hyp, seed) + (None,)
    mf.close()
    eng.close()
    assert 8 <= len(want[lc.LMEDS][1]) < n and 7 <= len(want[lc.RANSAC][1]) < n
    rows = "\n".join(f"{float(a[0])!r} {float(a[1])!r} {float(b[0])!r} {float(b[1])!r}" for a, b in zip(p, c))
    for method in (lc.LMEDS, lc.RANSAC, 2):                                   # 2: cv::FM_8POINT, RANSAC here as every other value
        fin = tmp_path / f"frame{method}.txt"
        fin.write_text(f"{frac[0]!r} {frac[1]!r} {frac[2]!r} {frac[3]!r} {lc.S_FOV!r} {fnp.WIDTH} {fnp.HEIGHT} {fc.THR!r} {n_hyp} {seed} "
                       f"{lc.MAX_MATCHES} {method}\n{n}\n{rows}\n")
        r = subprocess.run([exe, "filter", str(fin)], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = {line.split()[0]: line.split()[1:] for line in r.stdout.strip().splitlines()}
        mask, keep, pxy, cxy, last = want[lc.LMEDS if method == lc.LMEDS else lc.RANSAC]
        assert int(got["N"][0]) == len(keep) == int(mask.sum()), method
        assert [int(v) for v in got["I"]] == keep.tolist(), method
        m = np.array([float(v) for v in got["M"]]).reshape(-1, 4)
        assert m[:, :2].tobytes() == pxy.tobytes() and m[:, 2:].tobytes() == cxy.tobytes(), method
        if method == lc.LMEDS:
            assert got["L"][0] == "1" and (float(got["L"][1]), float(got["L"][2])) == last and last[1] > 0.0
        else:
            assert got["L"] == ["0", "0", "0"]


def test_cpp_tracker_follows_the_method(tmp_path):
    exe, env = example()
    sc = dict(tc.SCENES["walk"], describe=None)
    seq = sc["sequences"][0][:4]
    W, H = tc.W, tc.H
    frac = (kc.K_CHAIN[0] / W, kc.K_CHAIN[1] / H, kc.K_CHAIN[2] / W, kc.K_CHAIN[3] / H)
    Kc = (W * frac[0], H * frac[1], W * frac[2], H * frac[3])
    seed = 11
    paths = []
    for i, img in enumerate(seq):
        path = tmp_path / f"image{i}.raw"
        path.write_bytes(np.ascontiguousarray(img).tobytes())
        paths.append(str(path))
    eng = engine.Engine(4, 0, 4)
    try:
        for method in (lc.LMEDS, lc.RANSAC):
            mf = tracker.MatchFilter(eng, sc["max_matches"], Kc, 0.0)
            k = tracker.Klt(eng, 0, W, H, sc["win"], sc["max_level"], 30, 0.01, sc["min_eig_thr"], match_filter=mf)
            try:
                k.detect_setup(sc["threshold"], sc["non_max_supp"], sc["block_half_length"], sc["margin"], 32768)
                k.frame_setup(sc["n_feat_min"], sc["n_tiles_h"], sc["n_tiles_w"], sc["max_feat_per_tile"], sc["threshold_px"], sc["n_hyp"])
                k.outlier_method(method)                             # (Klt inherits it: the xk_trk is shared)
                frames, lasts = [], []
                for i, img in enumerate(seq):
                    frames.append(k.frame(img, seed=seed + i))
                    try:
                        lasts.append(mf.fundamental_medians(0, 0)[1])
                    except engine.XkError:
                        lasts.append(None)
            finally:
                k.close()
                mf.close()
            assert all(f["n_matches"] >= 8 for f in frames[1:])
            case = tmp_path / f"case{method}.txt"
            case.write_text(f"{frac[0]!r} {frac[1]!r} {frac[2]!r} {frac[3]!r} 0.0 {W} {H} {W} {sc['win'][0]} {sc['win'][1]} {sc['max_level']} "
                            f"{sc['min_eig_thr']!r} {sc['threshold']} {sc['non_max_supp']} {sc['block_half_length']} {sc['margin']} {sc['n_feat_min']} "
                            f"{sc['n_tiles_h']} {sc['n_tiles_w']} {sc['max_feat_per_tile']} {sc['threshold_px']!r} {sc['n_hyp']} {seed} "
                            f"{sc['max_matches']} {method}\n")
            r = subprocess.run([exe, "track", str(case)] + paths, capture_output=True, text=True, env=env, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            lines = r.stdout.strip().splitlines()
            assert len(lines) == 3 * len(seq)
            for i, (f, last) in enumerate(zip(frames, lasts)):
                out = {line.split()[0]: line.split()[1:] for line in lines[3 * i:3 * i + 3]}
                assert [int(v) for v in out["F"]] == [i] + [f[key] for key in tracker.FrameOut.COUNTS], (method, i)
                v = np.array([float(x) for x in out["C"]]).reshape(-1, 4)
                assert v[:, :2].tobytes() == f["cur_xy"].tobytes() and v[:, 2:].tobytes() == f["cur_dist_xy"].tobytes(), (method, i)
                if method == lc.LMEDS and i > 0:
                    assert last is not None and out["L"][0] == "1" and (float(out["L"][1]), float(out["L"][2])) == last, i
                else:
                    assert last is None and out["L"] == ["0", "0", "0"], (method, i)
    finally:
        eng.close()
