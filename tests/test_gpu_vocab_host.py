"""The C++ mirror x::VocabularyTrainer (host/include/x/place_recognition/database.h) driven through its example binary on a
descriptor file written here, against the NumPy restatement tests/vocab_np.py."""
import os
import subprocess

import numpy as np
import pytest

import vocab_cases as vc
import vocab_np as vnp

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(__file__), "..", "x_multi_agent_amd")


def _ints(a):
    return " ".join(str(int(x)) for x in np.asarray(a).ravel())


def test_cpp_vocabulary_trainer(tmp_path):
    exe = os.path.join(PKG, "xk_vocab_train_example")
    if not os.path.exists(exe):
        from x_multi_agent_amd import build
        build.build_host()
    k, L, seed, max_iter = 3, 3, 5, 100
    d = vc.clustered(400, 32, seed=21)
    pieces = (d[:100], d[100:101], d[101:])
    fin = tmp_path / "case.txt"
    fin.write_text("\n".join([f"{k} {L} 32 {seed} {max_iter} {len(pieces)}"] + [f"{len(p)} {_ints(p)}" for p in pieces]) + "\n")
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, str(fin)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {line.split(" ", 1)[0]: np.array(line.split()[1:], np.int64) for line in r.stdout.strip().splitlines()}
    ref = vnp.train(d, k, L, seed=seed, max_iter=max_iter)
    n_nodes, n_words = len(ref["desc"]), len(ref["node_of_word"])
    assert list(got["V"]) == [k, L, n_nodes, k, 32, n_words]
    assert np.array_equal(got["D"].reshape(n_nodes, 32), ref["desc"])
    assert np.array_equal(got["C"].reshape(n_nodes, k), ref["children"])
    assert np.array_equal(got["W"], ref["word_of_node"]) and np.array_equal(got["N"], ref["node_of_word"])
    levels, capped = int(got["O"][0]), int(got["O"][1])
    assert capped == ref["capped_nodes"] == 0 and levels == L
    assert list(got["O"][4::2]) == ref["nodes"] and list(got["O"][5::2]) == ref["passes"]
