"""Training sets shared by tests/test_vocab_np.py and the GPU tests of xk_voc_*: clustered binary descriptors in the
style of synth.make_descriptors / observe_descriptors, and a structural check of DBoW3's node numbering."""
import numpy as np


def clustered(n, desc_bytes=32, centres=12, noise=0.08, seed=5):
    """n descriptors: one of `centres` random centres each, XOR bit noise (every bit flipped with probability `noise`)."""
    rng = np.random.default_rng(seed)
    cen = rng.integers(0, 256, size=(centres, desc_bytes), dtype=np.uint8)
    which = rng.integers(0, centres, size=n)
    flips = np.packbits(rng.random((n, desc_bytes * 8)) < noise, axis=1)
    return np.bitwise_xor(cen[which], flips)


def repeated(distinct=40, times=10, desc_bytes=32, seed=6):
    """`distinct` random descriptors, each `times` times, interleaved: zero dist_sum deep in the tree, fewer than k
    children, ties everywhere."""
    base = np.random.default_rng(seed).integers(0, 256, size=(distinct, desc_bytes), dtype=np.uint8)
    return np.tile(base, (times, 1))


def check_dbow3_numbering(voc):
    """Vocabulary.cpp:361-393 and :496-515 as properties of the arrays: a node's children are one block of consecutive
    ids; ids are handed out by appending a node's block and then descending into its children in order; words are the
    leaves in id order, root excluded."""
    ch = np.asarray(voc["children"])
    n = len(ch)
    nxt = [1]

    def walk(i):
        kids = [int(c) for c in ch[i] if c >= 0]
        assert all(c < 0 for c in ch[i][len(kids):]), "children are not -1 padded at the end"
        assert kids == list(range(nxt[0], nxt[0] + len(kids))), (i, kids, nxt[0])
        nxt[0] += len(kids)
        for c in kids:
            if ch[c][0] >= 0:
                walk(c)

    walk(0)
    assert nxt[0] == n
    leaves = [i for i in range(1, n) if ch[i][0] < 0]
    assert list(voc["node_of_word"]) == leaves
    won = np.full(n, -1, np.int32)
    won[leaves] = np.arange(len(leaves))
    assert np.array_equal(voc["word_of_node"], won)
