"""host/examples/photo_main.cpp -- x::FeatureTracker::setPhotometric / calibrate (Tracker::calibrateImage, tracker.cpp:761-858)
between pushImage and track on the C++ mirror -- on the per-frame scene of tests/photo_cases.py written to temporary files: the
detected features and their intensities, the kept count, the support and the corrected image against the restatement
tests/photo_np.py, the gains within the measured tolerance, and the tracking that follows (on the corrected image) against
tracker.Klt, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import photo_cases as pc
import photo_np as pnp

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(__file__), "..", "x_multi_agent_amd")


def fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data.tobytes():
        h = ((h ^ b) * 0x100000001b3) & ((1 << 64) - 1)
    return h


def test_cpp_photometric_calibration(tmp_path):
    exe = os.path.join(PKG, "xk_photo_example")
    if not os.path.exists(exe):
        from x_multi_agent_amd import build
        build.build_host()
    q = pc.FRAME
    W, H = q["size"]
    im1, im2 = pc.frame_images()
    xy, val = pc.frame_features()
    n_hyp = min(len(xy), 64)                                    # the mirror evaluates min(features, n_hyp) hypotheses
    ref = pnp.calibrate(dict(ring=[(1.0, 0.0)], done=False), im1, im2, xy, val, n_hyp, q["ransac_seed"], q["kernel_size"], q["eps_gap"],
                        q["eps_base"], pc.frame_klt())
    # (one hypothesis more than the case test_photo_np.py verifies: its conditions are checked here, it is cheap)
    assert ref["ransac"]["margin"] >= pc.MARGIN and ref["support"] > ref["ransac"]["runner_up"]

    stride = W + 5
    bufs = []
    for im in (im1, im2):
        b = np.full((H, stride), 0xA5, np.uint8)
        b[:, :W] = im
        bufs.append(b)
    case, f1, f2 = tmp_path / "case.txt", tmp_path / "previous.raw", tmp_path / "current.raw"
    case.write_text(f"{W} {H} {stride} {q['win'][0]} {q['win'][1]} {q['max_level']} {q['max_iter']} {q['eps']!r} {q['min_eig_thr']!r} "
                    f"{q['threshold']} {q['b']} {q['margin']} {q['kernel_size']} {q['eps_gap']!r} {q['eps_base']!r} 64 {q['ransac_seed']} 64\n")
    f1.write_bytes(bufs[0].tobytes())
    f2.write_bytes(bufs[1].tobytes())
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, str(case), str(f1), str(f2)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {line.split()[0]: line.split()[1:] for line in r.stdout.strip().splitlines()}
    print(r.stdout[:400])

    assert int(out["D"][0]) == len(xy)
    P = np.array([float(v) for v in out["P"]]).reshape(-1, 3)
    assert np.array_equal(P[:, :2], xy.astype(np.float64)) and P[:, 2].tobytes() == val.tobytes()
    est, kept, support = (int(v) for v in out["E"])
    assert est == 1 and kept == len(ref["keep_idx"]) and support == ref["support"]
    G = np.array([float(v) for v in out["G"]])
    assert pc.close(G[0], ref["a_rel"]) and pc.close(G[1], ref["b_rel"]) and pc.close(G[2:], ref["frame_ab"])
    corrected = pnp.correct(im2, G[4], G[5])                    # with the pair the device reports
    assert [int(v) for v in out["S"]] == [fnv1a(corrected), fnv1a(im2)]

    eng = engine.Engine(4, 0, 4)                                # the tracking that follows, through the Python binding
    k = tracker.Klt(eng, 64, W, H, q["win"], q["max_level"], q["max_iter"], q["eps"], q["min_eig_thr"])
    try:
        k.push_image(im1)
        k.push_image(corrected)
        got = k.track(xy)
    finally:
        k.close()
        eng.close()
    assert int(out["T"][0]) == len(got["keep_idx"]) and [int(v) for v in out["J"]] == got["keep_idx"].tolist()
    Cm = np.array([float(v) for v in out["C"]]).reshape(-1, 3)
    assert Cm[:, :2].tobytes() == got["kept_cur"].tobytes()
    raw_int = pnp.intensity(im2, np.trunc(got["kept_cur"]).astype(np.int64), q["kernel_size"])[0]
    assert Cm[:, 2].tobytes() == raw_int.tobytes()              # track() fills the intensity from the RAW current image
