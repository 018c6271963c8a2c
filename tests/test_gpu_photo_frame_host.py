"""host/examples/photo_tracker_main.cpp -- the photometric x::Tracker (Tracker::track with calibrateImage) on the C++ mirror -- against
tracker.Klt.photo_frame on the gain_walk scene written to temporary files: the counts, the calibration's outcome, the origins and
the intensities of every frame exactly, and the checksum over the bytes of every match."""
import os
import struct
import subprocess

import numpy as np
import pytest

import klt_cases as kc
import photo_frame_cases as pc

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(__file__), "..", "x_multi_agent_amd")


def fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def checksum(f):
    """As photo_tracker_main.cpp: per match, the previous feature's x y x_dist y_dist, the current one's, both intensities, the score,
    the tiles and the descriptor."""
    out = bytearray()
    for i in range(f["n_matches"]):
        out += struct.pack("<8d", *f["prev_xy"][i], *f["prev_dist_xy"][i], *f["cur_xy"][i], *f["cur_dist_xy"][i])
        out += struct.pack("<2d", f["prev_intensity"][i], f["cur_intensity"][i])
        out += struct.pack("<5i", int(f["score"][i]), *(int(v) for v in f["tiles"][i]))
        out += f["desc"][i].tobytes()
    return fnv1a(bytes(out))


def test_cpp_photo_tracker(tmp_path):
    exe = os.path.join(PKG, "xk_photo_tracker_example")
    if not os.path.exists(exe):
        from x_multi_agent_amd import build
        build.build_host()
    sc = pc.SCENES["gain_walk"]
    seq, d = sc["sequences"][0], sc["describe"]
    W, H = pc.W, pc.H
    # x::Camera takes the intrinsics as fractions of the image size (camera.cpp:27-33): the same products here
    frac = (kc.K_CHAIN[0] / W, kc.K_CHAIN[1] / H, kc.K_CHAIN[2] / W, kc.K_CHAIN[3] / H)
    Kc = (W * frac[0], H * frac[1], W * frac[2], H * frac[3])
    seed, seed_photo, threshold_photo = 11, 23, 12

    eng = engine.Engine(4, 0, 4)
    mf = tracker.MatchFilter(eng, sc["max_matches"], Kc, 0.0)
    k = tracker.Klt(eng, 0, W, H, sc["win"], sc["max_level"], 30, 0.01, sc["min_eig_thr"], match_filter=mf)
    k.detect_setup(sc["threshold"], sc["non_max_supp"], sc["block_half_length"], max(sc["margin"], d["edge"]), 32768)
    k.describe_setup(d["centroid"], -1.0, d["edge"], None, sc["max_matches"])
    k.frame_setup(sc["n_feat_min"], sc["n_tiles_h"], sc["n_tiles_w"], sc["max_feat_per_tile"], sc["threshold_px"], sc["n_hyp"])
    k.photo_setup(sc["kernel_size"], sc["eps_gap"], sc["eps_base"], sc["n_hyp_photo"])
    k.photo_frame_setup(sc["n_hyp_photo"], threshold_photo)
    frames = [k.photo_frame(img, seed=seed + i, seed_photo=seed_photo + i) for i, img in enumerate(seq)]
    k.close()
    mf.close()
    eng.close()
    assert all(f["estimated"] and f["n_matches"] >= 7 for f in frames[1:]) and any(f["redetected"] for f in frames[2:])

    case = tmp_path / "case.txt"
    case.write_text(f"{frac[0]!r} {frac[1]!r} {frac[2]!r} {frac[3]!r} 0.0 {W} {H} {W} {sc['win'][0]} {sc['win'][1]} {sc['max_level']} "
                    f"{sc['min_eig_thr']!r} {sc['threshold']} {sc['non_max_supp']} {sc['block_half_length']} {sc['margin']} {sc['n_feat_min']} "
                    f"{sc['n_tiles_h']} {sc['n_tiles_w']} {sc['max_feat_per_tile']} {sc['threshold_px']!r} {sc['n_hyp']} {seed} "
                    f"{sc['max_matches']} 1 {d['centroid']} {d['edge']} {sc['kernel_size']} {sc['eps_gap']!r} {sc['eps_base']!r} "
                    f"{sc['n_hyp_photo']} {threshold_photo} {seed_photo}\n")
    paths = []
    for i, img in enumerate(seq):
        p = tmp_path / f"image{i}.raw"
        p.write_bytes(np.ascontiguousarray(img).tobytes())
        paths.append(str(p))
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, str(case)] + paths, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 5 * len(seq)
    for i, f in enumerate(frames):
        out = {line.split()[0]: line.split()[1:] for line in lines[5 * i:5 * i + 5]}
        assert [int(v) for v in out["F"]] == [i] + [f[key] for key in tracker.FrameOut.COUNTS], i
        g = out["G"]
        assert [int(v) for v in g[:4]] == [f["n_cal_kept"], int(f["estimated"]), int(f["done"]), f["support"]], i
        gains = np.array([float(v) for v in g[4:]])
        assert gains.tobytes() == np.concatenate([[f["a_rel"], f["b_rel"]], f["frame_ab"]]).tobytes(), i
        assert [int(v) for v in out["O"]] == f["origin"].tolist(), i
        v = np.array([float(x) for x in out["I"]]).reshape(-1, 2)
        assert v[:, 0].tobytes() == f["prev_intensity"].tobytes() and v[:, 1].tobytes() == f["cur_intensity"].tobytes(), i
        assert int(out["X"][0], 16) == checksum(f), i
