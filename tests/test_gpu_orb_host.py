"""host/examples/describe_main.cpp -- detection with description on the C++ mirror (x::FeatureTracker::setDescription / detect /
describe / track, x::TrackedFeature's descriptor) and the descriptors' way through x::Database::knnMatch -- against tracker.Klt +
place.Database driven from Python on the same images written to temporary files: every printed list, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import orb_cases as oc

from x_multi_agent_amd import engine, place, tracker

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(__file__), "..", "x_multi_agent_amd")
WIN, MAX_LEVEL = (15, 15), 2


def _ints(a):
    return " ".join(str(int(x)) for x in np.asarray(a).ravel())


def python_loop(ims, W, H, hp, pattern, voc):
    """The loop of describe_main.cpp -> {(tag, frame): rows} with the printed numbers per item."""
    out = {}
    eng = engine.Engine(4, 0, 4)
    k = tracker.Klt(eng, hp["max_features"], W, H, WIN, MAX_LEVEL)
    db = place.Database(eng, voc, 0.0, max_desc=hp["max_desc"])
    k.detect_setup(hp["threshold"], hp["nms"], hp["b"], max(hp["m"], hp["edge"]), hp["max_candidates"])   # (what setDescription makes of the margin)
    k.describe_setup(hp["orientation"], hp["angle"], hp["edge"], pattern, hp["max_desc"])

    def detected(which=1):
        d = k.detect(which)
        r = k.describe(d["xy"], which)
        assert np.array_equal(r["keep_idx"], np.arange(len(d["xy"])))
        return d, r, np.concatenate([d["xy"], d["score"][:, None], r["desc"]], axis=1).astype(np.float64)

    k.push_image(ims[0])
    d1, r1, out["D", 1] = detected()
    k.push_image(ims[1])
    g = k.track(d1["xy"].astype(np.float32))
    out["T", 2] = np.concatenate([d1["xy"][g["keep_idx"]].astype(np.float64), g["kept_cur"], r1["desc"][g["keep_idx"]].astype(np.float64)], axis=1)
    s = k.describe(d1["xy"] + np.array(oc.SHIFT, np.int32), 1)
    out["S", 2] = np.concatenate([s["keep_idx"][:, None], s["desc"]], axis=1).astype(np.float64)
    out["D", 2] = detected()[2]
    idx, dist = db.knn_match(s["desc"], r1["desc"])
    out["K", 2] = np.stack([idx[:, 0], dist[:, 0], idx[:, 1], dist[:, 1]], axis=1).astype(np.float64)
    db.close()
    k.close()
    eng.close()
    return out, s["keep_idx"]


@pytest.mark.parametrize("pattern", ["default", "corners"])
def test_cpp_detection_description_and_matching(tmp_path, pattern):
    exe = os.path.join(PKG, "xk_describe_example")
    if not os.path.exists(exe):
        from x_multi_agent_amd import build
        build.build_host()
    hp = oc.HOST
    ims = oc.shifted_pair()
    H, W = ims[0].shape
    pat = None if pattern == "default" else oc.corner_pattern()
    voc = place.load_vocabulary()
    ref, inside = python_loop(ims, W, H, hp, pat, voc)

    # the pair does what it is there for: features on both images, most of them tracked, the shifted ones matched to themselves
    assert len(ref["D", 1]) > 20 and len(ref["D", 2]) > 20 and len(ref["T", 2]) > 10
    assert 20 < len(ref["S", 2]) < len(ref["D", 1])
    assert np.array_equal(ref["K", 2][:, 0], inside) and not ref["K", 2][:, 1].any() and np.all(ref["K", 2][:, 3] > 0)

    case = tmp_path / "case.txt"
    case.write_text(f"0.75 1.0 0.5 0.5 0.0 {W} {H} {W} {WIN[0]} {WIN[1]} {MAX_LEVEL} 30 0.01 0.003 {hp['max_features']} {hp['threshold']} {hp['nms']} "
                    f"{hp['b']} {hp['m']} {hp['max_candidates']} {hp['orientation']} {hp['angle']!r} {hp['edge']} {hp['max_desc']} {oc.SHIFT[0]} "
                    f"{oc.SHIFT[1]} " + ("0" if pat is None else "256 " + _ints(pat)) + "\n")
    vfile = tmp_path / "vocabulary.txt"
    vfile.write_text("\n".join([f"{int(voc['k'])} {int(voc['L'])} {voc['desc'].shape[0]} {voc['children'].shape[1]} 32 {len(voc['node_of_word'])}",
                                _ints(voc["desc"]), _ints(voc["children"]), _ints(voc["word_of_node"]), _ints(voc["node_of_word"])]) + "\n")
    files = []
    for i, im in enumerate(ims):
        p = tmp_path / f"image{i + 1}.raw"
        p.write_bytes(np.ascontiguousarray(im).tobytes())
        files.append(str(p))
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, str(case), str(vfile)] + files, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.strip().splitlines():
        w = line.split()
        got[w[0], int(w[1])] = (int(w[2]), np.array([float(v) for v in w[3:]], np.float64))
    assert sorted(got) == sorted(ref)
    for key, rows in ref.items():
        n, flat = got[key]
        assert n == len(rows), key
        assert flat.tobytes() == np.ascontiguousarray(rows, np.float64).ravel().tobytes(), key
