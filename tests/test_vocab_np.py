"""The restatement tests/vocab_np.py without a GPU: the mean rule, the tie rule of the association, seeding that stops on
duplicates, DBoW3's node numbering on an example worked out here, and the property that ties training to use -- every
training descriptor descends (ref_pr.Vocabulary.transform) to the leaf the training put it in.  This pins the oracle that
tests/test_gpu_vocab.py compares xk_voc_train with."""
import numpy as np
import pytest

import vocab_cases as vc
import vocab_np as vnp
from oracle import ref_pr


def _row(*bytes_):
    return np.array(bytes_, np.uint8)


def test_mean_rule():
    c = _row(0xAA, 0x55)
    # an even group: a bit with count n/2 is set (count >= n/2 + n%2 = 2 of 4)
    g = np.array([[0xF0, 0x01], [0xF0, 0x01], [0x0F, 0x00], [0x0F, 0x00]], np.uint8)
    assert np.array_equal(vnp.mean_value(g, c), _row(0xFF, 0x01))
    # odd groups: 2 of 3 needed (3/2 + 1), 3 of 5
    g = np.array([[0x80, 0x01], [0x80, 0x00], [0x00, 0x00]], np.uint8)
    assert np.array_equal(vnp.mean_value(g, c), _row(0x80, 0x00))
    g = np.array([[0x01, 0xFF]] * 2 + [[0x00, 0x0F]] * 3, np.uint8)
    assert np.array_equal(vnp.mean_value(g, c), _row(0x00, 0x0F))
    g = np.array([[0x01, 0xFF]] * 3 + [[0x00, 0x0F]] * 2, np.uint8)
    assert np.array_equal(vnp.mean_value(g, c), _row(0x01, 0xFF))
    # an empty group keeps its centre, a group of one copies its descriptor
    assert np.array_equal(vnp.mean_value(np.zeros((0, 2), np.uint8), c), c)
    assert np.array_equal(vnp.mean_value(np.array([[0x12, 0x34]], np.uint8), c), _row(0x12, 0x34))
    # MSB first inside a byte (bit 7 - i%8 of byte i/8): bit index 0 is 0x80 of byte 0
    g = np.array([[0x80, 0x00]] * 2, np.uint8)
    assert np.unpackbits(vnp.mean_value(g, c))[0] == 1


def test_association_ties_go_to_the_lowest_index():
    d = np.array([[0x0F], [0xFF], [0x00], [0x3C]], np.uint8)
    centres = np.array([[0x00], [0xFF], [0x00]], np.uint8)
    # 0x0F: 4 / 4 / 4 -> 0;  0xFF: 8 / 0 / 8 -> 1;  0x00: 0 / 8 / 0 -> 0 (not 2);  0x3C: 4 / 4 / 4 -> 0
    assert list(vnp.associate(d, centres)) == [0, 1, 0, 0]
    assert list(vnp.associate(d, centres[::-1])) == [0, 1, 0, 0]      # (0x00, 0xFF, 0x00 reversed is itself)
    assert list(vnp.associate(d, np.array([[0xFF], [0x00]], np.uint8))) == [0, 0, 1, 0]


def test_seeding_stops_on_duplicates():
    a, b = [0x00, 0x00, 0x00, 0x00], [0xFF, 0xFF, 0x00, 0x01]
    d = np.array([a, b, a, a, b, b, a, b], np.uint8)
    for seed in range(8):
        picks = vnp.seed_centres(d, 4, vnp.node_key(seed, 0))
        assert len(picks) == 2                                          # dist_sum is 0 once both values are centres
        assert sorted(map(tuple, d[picks])) == sorted([tuple(a), tuple(b)])
        assert picks[0] == vnp.sm(vnp.node_key(seed, 0)) % 8
    voc = vnp.train(d, 4, 2, seed=3)
    # root: two children; each child holds four equal descriptors (<= k): trivial, one child per descriptor
    assert voc["children"].shape == (11, 4) and list(voc["children"][0]) == [1, 2, -1, -1]
    assert list(voc["children"][1]) == [3, 4, 5, 6] and list(voc["children"][2]) == [7, 8, 9, 10]
    assert voc["capped_nodes"] == 0 and voc["passes"] == [2, 0] and voc["nodes"] == [1, 2]


def _first_and_second(d, key):
    """The two seeds of a k = 2 node, by hand: plain Python on the definition."""
    n = len(d)
    first = vnp.sm(key) % n
    dist = [bin(int.from_bytes(bytes(d[i] ^ d[first]), "big")).count("1") for i in range(n)]
    cut = 1 + vnp.sm(key + 1) % sum(dist)
    run = 0
    for i in range(n):
        run += dist[i]
        if run >= cut:
            return first, i
    raise AssertionError


def test_numbering_on_a_worked_example():
    """Seven descriptors, k = 2, L = 2.  Two far-apart values A-ish (a, a2, a, a2) and B-ish (b, b, b2), interleaved.
    Root: the seeds fall into different groups for the seed used (asserted), so the first association is A | B and
    the means are the majorities a | a2 (ties set) and b; the second association is the same: 2 passes.  Each child then
    splits its group: the second seed must be the other value (equal values have distance 0), so the children are the two
    values in the order the seeding draws them.  Ids: root 0; its block 1, 2; then 1's block 3, 4; then 2's block 5, 6."""
    a, a2 = _row(0x00, 0x00, 0x00, 0x00), _row(0x00, 0x00, 0x00, 0x07)
    b, b2 = _row(0xFF, 0xFF, 0xFF, 0xF0), _row(0xFF, 0xFF, 0x1F, 0xF0)
    d = np.stack([a, b, a2, b, a, b2, a2])
    in_a = np.array([1, 0, 1, 0, 1, 0, 1], bool)
    k, L, seed = 2, 2, 1
    f, s = _first_and_second(d, vnp.node_key(seed, 0))
    assert in_a[f] != in_a[s], "choose another seed: the example needs the root's seeds in different groups"
    groups = [d[in_a], d[~in_a]] if in_a[f] else [d[~in_a], d[in_a]]
    means = [a | a2, b] if in_a[f] else [b, a | a2]
    want = [np.zeros(4, np.uint8)] + means
    for c, g in enumerate(groups):
        f2, s2 = _first_and_second(g, vnp.node_key(seed, c + 1))       # path code 0 (k+1) + c + 1
        assert not np.array_equal(g[f2], g[s2])
        want += [g[f2], g[s2]]
    voc = vnp.train(d, k, L, seed=seed)
    assert np.array_equal(voc["desc"], np.stack(want))
    assert np.array_equal(voc["children"], [[1, 2], [3, 4], [5, 6], [-1, -1], [-1, -1], [-1, -1], [-1, -1]])
    assert list(voc["word_of_node"]) == [-1, -1, -1, 0, 1, 2, 3] and list(voc["node_of_word"]) == [3, 4, 5, 6]
    assert voc["passes"] == [2, 2] and voc["nodes"] == [1, 2] and voc["capped_nodes"] == 0
    vc.check_dbow3_numbering(voc)


@pytest.mark.parametrize("n,k,L,B", [(300, 3, 2, 32), (600, 3, 4, 32), (300, 4, 3, 16), (3, 4, 2, 32), (1, 3, 2, 32)])
def test_training_descriptors_descend_to_their_leaves(n, k, L, B):
    d = vc.clustered(n, B, seed=n + k)
    voc = vnp.train(d, k, L, seed=2, max_iter=100)
    assert voc["capped_nodes"] == 0
    assert max(voc["passes"]) <= 20              # (the prototype of the definition needed at most 7 on such data)
    vc.check_dbow3_numbering(voc)
    ch = voc["children"]
    assert len(voc["node_of_word"]) <= k ** L
    rv = ref_pr.Vocabulary(voc)
    for i in range(0, n, max(1, n // 150)):
        leaf = int(voc["leaf_of_desc"][i])
        assert ch[leaf][0] < 0
        assert rv.transform(d[i]) == voc["word_of_node"][leaf], i


def test_depth_first_differs_from_level_order():
    """With L = 3 the block of node 1's children comes before node 2's grandchildren only in depth-first numbering."""
    voc = vnp.train(vc.clustered(400, 32, seed=9), 3, 3, seed=4)
    vc.check_dbow3_numbering(voc)
    ch = voc["children"]
    first = ch[1]
    assert first[0] == 4 and ch[first[0]][0] == first[0] + int((first >= 0).sum())   # 1's block, then its first child's block


def test_cap_and_seed():
    d = vc.clustered(300, 32, seed=1)
    capped = vnp.train(d, 3, 2, seed=0, max_iter=1)
    assert capped["capped_nodes"] > 0 and capped["passes"][0] == 1
    # with one pass the root's children are its seeds: training descriptors themselves
    for c in capped["children"][0]:
        assert any(np.array_equal(capped["desc"][c], row) for row in d)
    a, b = vnp.train(d, 3, 2, seed=0), vnp.train(d, 3, 2, seed=1)
    assert not np.array_equal(a["desc"], b["desc"])
    again = vnp.train(d, 3, 2, seed=0)
    assert all(np.array_equal(a[key], again[key]) for key in ("desc", "children", "word_of_node", "node_of_word"))


def test_empty_training_set_gives_the_root_alone():
    voc = vnp.train(np.zeros((0, 32), np.uint8), 4, 3)
    assert voc["desc"].shape == (1, 32) and voc["children"].shape == (1, 4) and len(voc["node_of_word"]) == 0
