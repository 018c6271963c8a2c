"""host/examples/camera_models_main.cpp -- x::Camera::setDistortion and x::MatchFilter on the C++ mirror under a radial-tangential and
an equidistant lens -- against the device and the Python binding on the same frame: the host camera's undistortion within the bar of
tests/test_gpu_camera_models.py (same text as the device, csrc/xk_camera.h, but the host compiler contracts no multiply-adds), the
filter's kept indices and matches bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import camera_models_cases as cc
import camera_models_np as cnp
import fundamental_cases as fc
import fundamental_np as fnp

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(__file__), "..", "x_multi_agent_amd")


@pytest.mark.parametrize("case", [cc.FILTER_CASES[0], cc.FILTER_CASES[3]])
def test_cpp_camera_models(tmp_path, case):
    exe = os.path.join(PKG, "xk_camera_models_example")
    if not os.path.exists(exe):
        from x_multi_agent_amd import build
        build.build_host()
    name, n, share, noise, n_hyp, scene_seed = case
    model, k = cc.SETS[name]
    dp, dc = cc.filter_scene(name, n, share, noise, scene_seed)
    # x::Camera takes the intrinsics as fractions of the image size: the same products here
    frac = (cc.K[0] / fnp.WIDTH, cc.K[1] / fnp.HEIGHT, cc.K[2] / fnp.WIDTH, cc.K[3] / fnp.HEIGHT)
    Kc = (fnp.WIDTH * frac[0], fnp.HEIGHT * frac[1], fnp.WIDTH * frac[2], fnp.HEIGHT * frac[3])

    eng = engine.Engine(4, 0, 4)
    mf = tracker.MatchFilter(eng, cc.MAX_MATCHES, Kc, model=model, coeffs=k)
    mask, keep, pxy, cxy = mf.filter_matches(dp, dc, fc.THR, n_hyp, cc.FILTER_SEED)
    dev = mf.undistort(np.concatenate([dp, dc]))
    status = mf.undistort_status()
    mf.close()
    eng.close()
    assert 7 <= len(keep) < n

    fin = tmp_path / "frame.txt"
    rows = "\n".join(f"{float(a[0])!r} {float(a[1])!r} {float(b[0])!r} {float(b[1])!r}" for a, b in zip(dp, dc))
    fin.write_text(f"{frac[0]!r} {frac[1]!r} {frac[2]!r} {frac[3]!r} {fnp.WIDTH} {fnp.HEIGHT} {fc.THR!r} {n_hyp} {cc.FILTER_SEED} {cc.MAX_MATCHES}\n"
                   f"{model} {len(k)} {' '.join(repr(float(v)) for v in k)}\n{n}\n{rows}\n")
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, str(fin)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {line.split()[0]: line.split()[1:] for line in r.stdout.strip().splitlines()}
    # the device through the C ABI is the device through the binding
    d = np.array([float(v) for v in got["D"]]).reshape(-1, 2)
    assert d.tobytes() == dev.tobytes()
    assert (int(got["S"][0]), int(got["S"][1])) == status and status[0] == 0
    # x::Camera::undistort against the device, and against the restatement
    h = np.array([float(v) for v in got["H"]]).reshape(-1, 2)
    assert all(int(v) == 1 for v in got["V"])
    ref, state, _, detj = cnp.undistort(np.concatenate([dp, dc]), Kc, model, k)
    bar = 1e-12 * max(1.0, 1.0 / float(np.nanmin(detj)))
    rel = lambda a, b: float((np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)).max())
    print(name, "host vs device", rel(h, dev), "host vs restatement", rel(h, ref), "bar", bar)
    assert rel(h, dev) <= bar and rel(h, ref) <= bar
    back = np.array([float(v) for v in got["R"]])
    assert np.linalg.norm(back - dp[0]) / np.linalg.norm(dp[0]) <= bar
    # x::MatchFilter: the binding's kept indices and matches, bit for bit
    assert int(got["N"][0]) == len(keep) == int(mask.sum())
    assert [int(v) for v in got["I"]] == keep.tolist()
    m = np.array([float(v) for v in got["M"]]).reshape(-1, 4)
    assert m[:, :2].tobytes() == pxy.tobytes() and m[:, 2:].tobytes() == cxy.tobytes()
