"""host/examples/match_filter_main.cpp -- x::Camera and x::MatchFilter::filter, the outlier removal of Tracker::track
(tracker.cpp:233-293) on the C++ mirror -- against tracker.MatchFilter.filter_matches on the same generated frame: the
kept indices, their number and the undistorted coordinates of the matches, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import fundamental_cases as fc
import fundamental_np as fnp

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(__file__), "..", "x_multi_agent_amd")


def test_cpp_match_filter(tmp_path):
    exe = os.path.join(PKG, "xk_match_filter_example")
    if not os.path.exists(exe):
        from x_multi_agent_amd import build
        build.build_host()
    n, share, noise, n_hyp, scene_seed = fc.DISTORTED_CASE
    seed = 4
    p, c, _ = fc.pair(n, share, noise, scene_seed, "general", fc.S_FOV)
    # x::Camera takes the intrinsics as fractions of the image size (camera.cpp:27-33): the same products here
    frac = (fc.K[0] / fnp.WIDTH, fc.K[1] / fnp.HEIGHT, fc.K[2] / fnp.WIDTH, fc.K[3] / fnp.HEIGHT)
    Kc = (fnp.WIDTH * frac[0], fnp.HEIGHT * frac[1], fnp.WIDTH * frac[2], fnp.HEIGHT * frac[3])

    eng = engine.Engine(4, 0, 4)
    mf = tracker.MatchFilter(eng, fc.MAX_MATCHES, Kc, fc.S_FOV)
    mask, keep, pxy, cxy = mf.filter_matches(p, c, fc.THR, n_hyp, seed)
    mf.close()
    eng.close()
    assert 7 <= len(keep) < n                                  # something was kept and something removed

    fin = tmp_path / "frame.txt"
    rows = "\n".join(f"{float(a[0])!r} {float(a[1])!r} {float(b[0])!r} {float(b[1])!r}" for a, b in zip(p, c))
    fin.write_text(f"{frac[0]!r} {frac[1]!r} {frac[2]!r} {frac[3]!r} {fc.S_FOV!r} {fnp.WIDTH} {fnp.HEIGHT} {fc.THR!r} {n_hyp} {seed} "
                   f"{fc.MAX_MATCHES}\n{n}\n{rows}\n")
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, str(fin)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {line.split()[0]: line.split()[1:] for line in r.stdout.strip().splitlines()}
    assert int(got["N"][0]) == len(keep) == int(mask.sum())
    assert [int(v) for v in got["I"]] == keep.tolist()
    m = np.array([float(v) for v in got["M"]]).reshape(-1, 4)
    assert m[:, :2].tobytes() == pxy.tobytes() and m[:, 2:].tobytes() == cxy.tobytes()
    # x::Camera::undistort on the host (camera.cpp:69-87) against the restatement: the 1e-12 of test_gpu_fundamental
    u = np.array([float(v) for v in got["U"]])
    ref = fnp.undistort(p[:1], Kc, fc.S_FOV)[0]
    assert np.linalg.norm(u - ref) / np.linalg.norm(ref) <= 1e-12
