"""xk_voc_* (DBoW3::Vocabulary::create on the device) against the NumPy restatement tests/vocab_np.py, array
for array: everything is integer work, so the comparison is equality.  The restatement itself is pinned by
tests/test_vocab_np.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import vocab_cases as vc
import vocab_np as vnp
from oracle import ref_pr
from x_multi_agent_amd import engine, place

pytestmark = pytest.mark.gpu
ARRAYS = ("desc", "children", "word_of_node", "node_of_word")


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(4, 0, 4, device=0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _data(name):
    if name == "repeated":
        return vc.repeated(40, 10, 32)
    n, B = name
    return vc.clustered(n, B, seed=n + B)


@functools.lru_cache(maxsize=None)
def _ref(name, k, L, seed=0, max_iter=100):
    return vnp.train(_data(name), k, L, seed=seed, max_iter=max_iter)


def _same(got, ref):
    assert got["desc"].shape == ref["desc"].shape, (got["desc"].shape, ref["desc"].shape)
    for key in ("k", "L"):
        assert int(got[key]) == int(ref[key])
    for key in ARRAYS:
        assert np.array_equal(got[key], ref[key]), key
    oc = got["outcome"]
    assert oc["capped_nodes"] == ref["capped_nodes"]
    assert oc["level_passes"] == ref["passes"] and oc["level_nodes"] == ref["nodes"]
    assert oc["n_nodes"] == len(ref["desc"]) and oc["n_words"] == len(ref["node_of_word"])
    # one wait per association pass of a level, one per level for its result (<= k), and the named allowance
    assert oc["host_waits"] <= sum(p + int(got["k"]) for p in oc["level_passes"][:oc["levels"]]) + place.VOC_WAIT_SLACK
    assert oc["launches"] > 0 or len(ref["desc"]) == 1


# N = 5000, k = 2, L = 1: a root over 20 workgroups -- the running sum and the pick across workgroups
# (40 x 10 repeated): zero dist_sum, fewer than k children, ties everywhere
@pytest.mark.parametrize("name,k,L", [((300, 32), 3, 2), ((600, 32), 3, 4), ((2000, 32), 4, 3), ((5000, 32), 2, 1),
                                      ((300, 16), 3, 2), ((300, 64), 3, 2), ("repeated", 4, 3)])
def test_parity_with_the_restatement(eng, name, k, L):
    d = _data(name)
    got = place.train_vocabulary(eng, d, k, L, seed=0, max_iter=100)
    ref = _ref(name, k, L)
    _same(got, ref)
    assert got["outcome"]["capped_nodes"] == 0
    vc.check_dbow3_numbering(got)
    if name == "repeated":
        assert (got["children"][got["children"][:, 0] >= 0] < 0).any()      # some inner node has fewer than k children


@pytest.mark.parametrize("n", [3, 1])
def test_trivial_root(eng, n):
    d = _data((300, 32))[:n]
    got = place.train_vocabulary(eng, d, 4, 2)
    _same(got, vnp.train(d, 4, 2))
    assert np.array_equal(got["desc"][1:], d) and got["outcome"]["level_passes"] == [0, 0]
    assert list(got["children"][0][:n]) == list(range(1, n + 1))


def test_seeds_and_repeatability(eng):
    d = _data((300, 32))
    a = place.train_vocabulary(eng, d, 3, 2, seed=0)
    b = place.train_vocabulary(eng, d, 3, 2, seed=7)
    again = place.train_vocabulary(eng, d, 3, 2, seed=0)
    _same(b, _ref((300, 32), 3, 2, seed=7))
    assert not np.array_equal(a["desc"], b["desc"])
    for key in ARRAYS:
        assert np.array_equal(a[key], again[key]), key


def test_add_in_pieces_and_clear(eng):
    d = _data((300, 32))
    tr = place.VocabularyTrainer(eng, 3, 2, 32, max_desc=300)
    for piece in (d[:7], d[7:150], d[150:]):
        tr.add(piece)
    assert len(tr) == 300
    _same(tr.train(0, 100), _ref((300, 32), 3, 2))
    tr.clear()
    assert len(tr) == 0
    tr.add(d[:100])
    _same(tr.train(0, 100), vnp.train(d[:100], 3, 2))                   # the handle trains again after a clear
    tr.close()


def test_iteration_cap(eng):
    d = _data((300, 32))
    got = place.train_vocabulary(eng, d, 3, 2, seed=0, max_iter=1)
    assert got["outcome"]["capped_nodes"] > 0
    _same(got, _ref((300, 32), 3, 2, 0, 1))
    _same(place.train_vocabulary(eng, d, 3, 2, seed=0, max_iter=2), _ref((300, 32), 3, 2, 0, 2))


def test_trained_tree_feeds_the_database(eng):
    voc = place.train_vocabulary(eng, _data((2000, 32)), 4, 3)
    db = place.Database(eng, voc, 0.6, max_desc=256)
    fresh = vc.clustered(200, 32, seed=99)
    rv = ref_pr.Vocabulary(voc)
    assert np.array_equal(db.compute_vlad(fresh), ref_pr.compute_vlad(rv, fresh))
    db.close()
    # a ragged tree: leaves above depth L, fewer than k children
    voc = place.train_vocabulary(eng, _data("repeated"), 4, 3)
    db = place.Database(eng, voc, 0.6, max_desc=256)
    assert np.array_equal(db.compute_vlad(fresh), ref_pr.compute_vlad(ref_pr.Vocabulary(voc), fresh))
    db.close()


def test_savez_round_trip(eng, tmp_path):
    voc = place.train_vocabulary(eng, _data((300, 32)), 3, 2)
    path = tmp_path / "voc.npz"
    np.savez(path, **{key: voc[key] for key in ("k", "L") + ARRAYS})
    back = place.load_vocabulary(path=str(path))
    for key in ARRAYS:
        assert np.array_equal(back[key], voc[key])


def test_status_codes(eng):
    L = eng.L
    p = C.c_void_p()
    bad = [(1, 2, 32, 10), (17, 2, 32, 10), (3, 0, 32, 10), (3, 9, 32, 10), (3, 2, 30, 10), (3, 2, 68, 10), (3, 2, 0, 10),
           (3, 2, 32, 0)]
    for k, Lv, B, m in bad:
        assert L.xk_voc_create(eng.h, k, Lv, B, m, C.byref(p)) == 1, (k, Lv, B, m)
    assert L.xk_voc_create(None, 3, 2, 32, 10, C.byref(p)) == 1
    assert L.xk_voc_create(eng.h, 3, 2, 32, 10, None) == 1
    assert L.xk_voc_create(eng.h, 16, 8, 32, 10, C.byref(p)) == 6          # 16^8 x 32 bytes > 64 MB
    assert L.xk_voc_create(eng.h, 4, 2, 32, 10, C.byref(p)) == 0
    d = np.ascontiguousarray(_data((300, 32))[:11])
    dp = d.ctypes.data_as(place.c_ub)
    oc = place.XkVocOutcome()
    desc = np.zeros((64, 32), np.uint8)
    assert L.xk_voc_get(p, desc.ctypes.data_as(place.c_ub), None, None, None) == 1      # before a training
    assert L.xk_voc_train(p, C.c_ulong(0), 0, C.byref(oc)) == 1                         # max_iter < 1
    assert L.xk_voc_train(None, C.c_ulong(0), 10, C.byref(oc)) == 1
    # no descriptors: the root alone, which xk_pr_create refuses
    assert L.xk_voc_train(p, C.c_ulong(0), 10, C.byref(oc)) == 0
    assert (oc.n_nodes, oc.n_words, oc.levels, oc.host_waits) == (1, 0, 0, 0)
    assert L.xk_voc_get(p, desc.ctypes.data_as(place.c_ub), None, None, None) == 0 and not desc.any()
    with pytest.raises(engine.XkError):
        place.Database(eng, dict(k=4, L=2, desc=np.zeros((1, 32), np.uint8), children=np.full((1, 4), -1, np.int32),
                                 word_of_node=np.full(1, -1, np.int32), node_of_word=np.zeros(0, np.int32)), 0.6)
    assert L.xk_voc_add(p, dp, 11) == 6 and L.xk_voc_count(p) == 0                      # beyond max_desc: nothing appended
    assert L.xk_voc_add(p, dp, -1) == 1 and L.xk_voc_add(p, None, 3) == 1 and L.xk_voc_add(None, dp, 3) == 1
    assert L.xk_voc_add(p, dp, 6) == 0 and L.xk_voc_add(p, None, 0) == 0 and L.xk_voc_count(p) == 6
    assert L.xk_voc_add(p, dp, 5) == 6 and L.xk_voc_count(p) == 6
    assert L.xk_voc_clear(None) == 1 and L.xk_voc_count(None) == 0
    assert L.xk_voc_train(p, C.c_ulong(0), 10, None) == 0                               # the outcome is optional
    L.xk_voc_destroy(p)
    L.xk_voc_destroy(None)
