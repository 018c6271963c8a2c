"""TEST INFRASTRUCTURE -- NumPy restatement of DBoW3's vocabulary training for binary descriptors, recursive as the
reference is, written from third_party/DBow3/src/Vocabulary.cpp:157-186 (create), :233-394 (HKmeansStep), :409-491
(initiateClustersKMpp), :496-515 (createWords) and DescManip.cpp:26-75 (meanValue, binary branch).  A plain helper like
tests/orb_np.py: what tests/test_gpu_vocab.py compares xk_voc_train with, array for array.

Two substitutions against the reference, both shared with the device:
  sampler        rand() -> the counter-based splitmix64 finaliser sm() of csrc/xk_ransac.hip.h.  A node has a path code p
                 (0 for the root, p (k+1) + c + 1 for its c-th child) and a key K = sm(seed ^ sm(p)); its first centre is
                 descriptor sm(K) mod n, its j-th later centre the first descriptor whose inclusive running sum of
                 min_dist reaches cut = 1 + sm(K + j) mod dist_sum.
  iteration cap  at most max_iter association passes per node; a node that reaches the cap keeps its latest association
                 and the centres that association was computed against, and counts in capped_nodes.
Everything is integer arithmetic."""
import numpy as np

_M64 = (1 << 64) - 1
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def sm(z):
    """splitmix64's finaliser (xk_ransac_mix)."""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def node_key(seed, path):
    return sm((seed & _M64) ^ sm(path))


def distances(d, centre):
    """Hamming distance of every row of d [n, B] to centre [B] (DescManip::distance, binary branch)."""
    return _POP8[np.bitwise_xor(d, centre[None, :])].sum(axis=1)


def mean_value(group, centre):
    """DescManip::meanValue (DescManip.cpp:26-75): an empty group leaves the centre as it is, a group of one copies its
    descriptor, otherwise bit i is set iff its count >= n/2 + n%2 (bit 7 - i%8 of byte i/8: unpackbits' order)."""
    n = len(group)
    if n == 0:
        return centre.copy()
    if n == 1:
        return group[0].copy()
    counts = np.unpackbits(group, axis=1).astype(np.int64).sum(axis=0)
    return np.packbits(counts >= n // 2 + n % 2)


def seed_centres(d, k, key):
    """initiateClustersKMpp (Vocabulary.cpp:409-491) with the seeded sampler -> list of row indices (at most k)."""
    n = len(d)
    picks = [sm(key) % n]
    min_dist = distances(d, d[picks[0]])
    while len(picks) < k:
        min_dist = np.minimum(min_dist, distances(d, d[picks[-1]]))
        dist_sum = int(min_dist.sum())
        if dist_sum == 0:
            break
        cut = 1 + sm(key + len(picks)) % dist_sum
        picks.append(int(np.searchsorted(np.cumsum(min_dist), cut, side="left")))
    return picks


def associate(d, centres):
    """Nearest centre of every row, strict '<' over the centres in order: the lowest index wins ties."""
    dist = np.stack([distances(d, c) for c in centres], axis=1)
    return np.argmin(dist, axis=1)              # (argmin returns the first minimum)


def kmeans_node(d, k, key, max_iter):
    """The clustering of one node with more than k descriptors (HKmeansStep's while loop) -> (centres [c, B],
    association [n], passes, capped)."""
    centres = d[seed_centres(d, k, key)].copy()
    last, passes = None, 0
    while True:
        if last is not None:
            centres = np.stack([mean_value(d[last == c], centres[c]) for c in range(len(centres))])
        cur = associate(d, centres)
        passes += 1
        if last is not None and np.array_equal(cur, last):
            return centres, cur, passes, False
        if passes >= max_iter:
            return centres, cur, passes, True
        last = cur


def train(desc, k, L, seed=0, max_iter=100):
    """Vocabulary::create on desc [N, B] uint8 -> dict with the arrays place.load_vocabulary returns (k, L, desc, children,
    word_of_node, node_of_word) plus: passes [L] (most association passes of a node at each level), nodes [L] (nodes split at
    each level, trivial ones included), capped_nodes, leaf_of_desc [N] (the node each training descriptor ended in)."""
    desc = np.ascontiguousarray(desc, np.uint8)
    N, B = desc.shape
    node_desc, children = [np.zeros(B, np.uint8)], [[]]
    passes, nodes = [0] * L, [0] * L
    out = dict(capped=0)
    leaf_of_desc = np.zeros(N, np.int64)

    def step(parent, idx, level, path):
        if len(idx) == 0:
            return
        d = desc[idx]
        nodes[level - 1] += 1
        if len(idx) <= k:                       # trivial case: one cluster per feature
            centres, assoc = d.copy(), np.arange(len(idx))
        else:
            centres, assoc, n_pass, capped = kmeans_node(d, k, node_key(seed, path), max_iter)
            passes[level - 1] = max(passes[level - 1], n_pass)
            out["capped"] += int(capped)
        ids = []
        for c in range(len(centres)):           # the children are appended as one block
            ids.append(len(node_desc))
            node_desc.append(centres[c])
            children.append([])
            children[parent].append(ids[-1])
        for c, i in enumerate(ids):
            leaf_of_desc[idx[assoc == c]] = i
        if level < L:
            for c, i in enumerate(ids):         # then depth first, only into children with more than one descriptor
                sub = idx[assoc == c]
                if len(sub) > 1:
                    step(i, sub, level + 1, path * (k + 1) + c + 1)

    step(0, np.arange(N), 1, 0)
    n_nodes = len(node_desc)
    ch = np.full((n_nodes, k), -1, np.int32)
    for i, c in enumerate(children):
        ch[i, :len(c)] = c
    word_of_node = np.full(n_nodes, -1, np.int32)
    leaves = [i for i in range(1, n_nodes) if not children[i]]      # createWords: leaves in id order, root excluded
    word_of_node[leaves] = np.arange(len(leaves))
    return dict(k=np.int32(k), L=np.int32(L), desc=np.stack(node_desc), children=ch, word_of_node=word_of_node,
                node_of_word=np.array(leaves, np.int32), passes=passes, nodes=nodes, capped_nodes=out["capped"],
                leaf_of_desc=leaf_of_desc)
