"""host/examples/klt_main.cpp -- x::FeatureTracker (Tracker::featureTracking, tracker.cpp:623-690) and x::MatchFilter behind it
on the C++ mirror -- against tracker.Klt and tracker.MatchFilter on the same scene written to temporary files: the tracked
pairs and the matches, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import klt_cases as kc

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(__file__), "..", "x_multi_agent_amd")


def test_cpp_feature_tracker(tmp_path):
    exe = os.path.join(PKG, "xk_klt_example")
    if not os.path.exists(exe):
        from x_multi_agent_amd import build
        build.build_host()
    name = "w21_odd_n255"                                       # odd size, a row stride beyond the width, points outside the frame
    sc = kc.SCENES[name]
    W, H = sc["size"]
    im1, im2 = kc.images(name)
    pts = kc.points(name)
    pts = pts[np.isfinite(pts).all(axis=1)]                     # (the text file carries no NaN)
    # x::Camera takes the intrinsics as fractions of the image size (camera.cpp:27-33): the same products here
    frac = (kc.K_CHAIN[0] / W, kc.K_CHAIN[1] / H, kc.K_CHAIN[2] / W, kc.K_CHAIN[3] / H)
    Kc = (W * frac[0], H * frac[1], W * frac[2], H * frac[3])
    ransac = dict(threshold_px=0.3, n_hyp=64, seed=3)

    eng = engine.Engine(4, 0, 4)
    mf = tracker.MatchFilter(eng, kc.MAX_FEATURES, Kc, 0.0)
    k = tracker.Klt(eng, kc.MAX_FEATURES, W, H, sc["win"], sc["max_level"], sc["max_iter"], sc["eps"], sc["thr"], match_filter=mf)
    k.push_image(im1)
    k.push_image(im2)
    got = k.track(pts)
    mask, keep, pxy, cxy = mf.filter_matches(got["kept_prev"], got["kept_cur"], **ransac)
    k.close()
    mf.close()
    eng.close()
    assert 7 <= len(keep) <= len(got["keep_idx"]) < len(pts)    # something was tracked, something dropped

    case, f1, f2, fp = tmp_path / "case.txt", tmp_path / "previous.raw", tmp_path / "current.raw", tmp_path / "points.txt"
    case.write_text(f"{frac[0]!r} {frac[1]!r} {frac[2]!r} {frac[3]!r} 0.0 {W} {H} {sc['stride']} {sc['win'][0]} {sc['win'][1]} {sc['max_level']} "
                    f"{sc['max_iter']} {sc['eps']!r} {sc['thr']!r} {ransac['threshold_px']!r} {ransac['n_hyp']} {ransac['seed']} {kc.MAX_FEATURES}\n")
    f1.write_bytes(im1.tobytes())
    f2.write_bytes(im2.tobytes())
    fp.write_text(f"{len(pts)}\n" + "\n".join(f"{float(a)!r} {float(b)!r}" for a, b in pts) + "\n")
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, str(case), str(f1), str(f2), str(fp)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {line.split()[0]: line.split()[1:] for line in r.stdout.strip().splitlines()}
    assert int(out["T"][0]) == len(got["keep_idx"])
    assert [int(v) for v in out["J"]] == got["keep_idx"].tolist()
    assert np.array([float(v) for v in out["C"]]).reshape(-1, 2).tobytes() == got["kept_cur"].tobytes()
    assert int(out["N"][0]) == len(keep) == int(mask.sum())
    assert [int(v) for v in out["I"]] == keep.tolist()
    m = np.array([float(v) for v in out["M"]]).reshape(-1, 4)
    assert m[:, :2].tobytes() == pxy.tobytes() and m[:, 2:].tobytes() == cxy.tobytes()
