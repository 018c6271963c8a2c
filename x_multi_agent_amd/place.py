"""Place-recognition request filter and keyframe store on the device -- ctypes binding of the xk_pr_* entry
points (include/xk.h), and the training of the vocabulary they consume (xk_voc_*: DBoW3's Vocabulary::create).  Mirrors the reference's `Database` / `VLAD` / `Keyframe`
(src/x/place_recognition/{database,vlad,keyframe}.cpp) and the matching front half of
`PlaceRecognition::findCorrespondences` (place_recognition.cpp:137-390).

No fallback: everything numeric runs in libxk.so's HIP kernels; the host part here is the same bookkeeping the
reference does on the host (ratio test, duplicate removal, MSCKF / SLAM / OPP classification) -- the stage-by-stage
path.  Database.find_correspondences is findCorrespondences as one device call, list work included."""
import ctypes as C
import os

import numpy as np

from .engine import XkError, c_dp, c_ip

c_ub = C.POINTER(C.c_ubyte)
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def load_vocabulary(name="visual", path=None):
    """A DBoW3 vocabulary as unpacked arrays (k, L, desc, children, word_of_node, node_of_word).
    path: an .npz a deployment unpacked from its own Vocabulary/*.yaml (tools in tests/golden/make_vocab_fixture.py);
    default: the package's own copy of the reference's vocabulary `name` (Vocabulary/<name>_voc_3_4_dbow3.yaml),
    x_multi_agent_amd/data/vocab_<name>.npz."""
    return dict(np.load(path if path else os.path.join(DATA, f"vocab_{name}.npz")))


XK_VOC_MAX_LEVELS = 8
# Host waits a training may take beyond one per association pass and k per level (it takes one per level there: the
# level's result): none today; the allowance covers an entry and an exit wait.
VOC_WAIT_SLACK = 2


class XkVocOutcome(C.Structure):
    """xk_voc_outcome of include/xk.h."""
    _fields_ = [("n_nodes", C.c_int), ("n_words", C.c_int), ("levels", C.c_int), ("level_nodes", C.c_int * XK_VOC_MAX_LEVELS),
                ("level_passes", C.c_int * XK_VOC_MAX_LEVELS), ("capped_nodes", C.c_int), ("launches", C.c_int),
                ("host_waits", C.c_int)]


class XkPrCorrOut(C.Structure):
    """xk_pr_corr_out of include/xk.h."""
    _fields_ = [("status", C.c_int), ("n_candidates", C.c_int), ("n_inliers", C.c_int), ("winner", C.c_int), ("n_good", C.c_int),
                ("n_classified", C.c_int), ("launches", C.c_int), ("E", C.c_double * 9)]


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a, a.ctypes.data_as(c_ub)


class Database:
    """x::Database on one agent's GPU: the keyframes (payload, tracks, descriptors, VLAD) live in HBM."""

    def __init__(self, eng, voc, pr_score_thr, payload_doubles=0, tracks_doubles=0, max_desc=1024):
        self.eng, self.L = eng, eng.L
        self.thr = float(pr_score_thr)
        self.k, self.Lv = int(voc["k"]), int(voc["L"])
        desc, dp = _u8(voc["desc"])
        ch = np.ascontiguousarray(voc["children"], np.int32)
        won = np.ascontiguousarray(voc["word_of_node"], np.int32)
        now = np.ascontiguousarray(voc["node_of_word"], np.int32)
        self.desc_bytes = desc.shape[1]
        self.p = C.c_void_p()
        rc = self.L.xk_pr_create(eng.h, C.c_int(self.k), C.c_int(self.Lv), C.c_int(desc.shape[0]), C.c_int(ch.shape[1]),
                                 C.c_int(self.desc_bytes), dp, ch.ctypes.data_as(c_ip), won.ctypes.data_as(c_ip),
                                 now.ctypes.data_as(c_ip), C.c_int(len(now)), C.c_long(payload_doubles),
                                 C.c_long(tracks_doubles), C.c_int(max_desc), C.byref(self.p))
        if rc != 0:
            raise XkError(rc, "xk_pr_create", (self.L.xk_last_error(eng.h) or b"").decode())
        self.vlad_bytes = int(self.L.xk_pr_vlad_bytes(self.p))
        self.clusters = self.vlad_bytes // self.desc_bytes
        self.max_desc = max_desc

    def close(self):
        if self.p:
            self.L.xk_pr_destroy(self.p)
            self.p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise XkError(rc, what, (self.L.xk_last_error(self.eng.h) or b"").decode())

    def __len__(self):
        return int(self.L.xk_pr_size(self.p))

    def compute_vlad(self, descriptors):
        """VLAD::computeVLAD -> uint8 [clusters, desc_bytes]."""
        d, dp = _u8(np.asarray(descriptors, np.uint8).reshape(-1, self.desc_bytes))
        out = np.zeros(self.vlad_bytes, np.uint8)
        self._chk(self.L.xk_pr_compute_vlad(self.p, dp, C.c_int(d.shape[0]), out.ctypes.data_as(c_ub)), "xk_pr_compute_vlad")
        return out.reshape(self.clusters, self.desc_bytes)

    def add_keyframe(self, descriptors, payload_ptr=None, tracks_ptr=None, tag=0):
        d, dp = _u8(np.asarray(descriptors, np.uint8).reshape(-1, self.desc_bytes))
        pp = C.cast(C.c_void_p(payload_ptr), c_dp) if payload_ptr else None
        tp = C.cast(C.c_void_p(tracks_ptr), c_dp) if tracks_ptr else None
        self._chk(self.L.xk_pr_add_keyframe(self.p, dp, C.c_int(d.shape[0]), pp, tp, C.c_long(tag)), "xk_pr_add_keyframe")

    def find_candidate(self, uav_id, query_vlad):
        """Database::findCandidate -> (index or -1, score, tag)."""
        q, qp = _u8(np.asarray(query_vlad, np.uint8).ravel())
        if q.size != self.vlad_bytes:
            raise ValueError("query VLAD has the wrong size")
        idx, sc, tag = C.c_int(-1), C.c_double(0.0), C.c_long(-1)
        self._chk(self.L.xk_pr_find_candidate(self.p, C.c_int(uav_id), qp, C.c_double(self.thr), C.byref(idx), C.byref(sc),
                                              C.byref(tag)), "xk_pr_find_candidate")
        return idx.value, sc.value, tag.value

    def keyframe(self, index, want_descriptors=False):
        """-> dict(payload_ptr, tracks_ptr, n_desc, tag[, descriptors]) of the stored keyframe (device pointers)."""
        pp, tp = c_dp(), c_dp()
        nd, tag = C.c_int(0), C.c_long(0)
        buf = np.zeros((self.max_desc, self.desc_bytes), np.uint8) if want_descriptors else None
        self._chk(self.L.xk_pr_keyframe(self.p, C.c_int(index), C.byref(pp), C.byref(tp), C.byref(nd), C.byref(tag),
                                        buf.ctypes.data_as(c_ub) if want_descriptors else None), "xk_pr_keyframe")
        out = dict(payload_ptr=C.cast(pp, C.c_void_p).value, tracks_ptr=C.cast(tp, C.c_void_p).value, n_desc=nd.value,
                   tag=tag.value)
        if want_descriptors:
            out["descriptors"] = buf[:nd.value].copy()
        return out

    def copy_keyframe(self, index, payload_dst_ptr=None, tracks_dst_ptr=None):
        """The stored keyframe's payload / tracks into caller-owned DEVICE buffers (the response's send buffer)."""
        pp = C.cast(C.c_void_p(payload_dst_ptr), c_dp) if payload_dst_ptr else None
        tp = C.cast(C.c_void_p(tracks_dst_ptr), c_dp) if tracks_dst_ptr else None
        self._chk(self.L.xk_pr_copy_keyframe(self.p, C.c_int(index), pp, tp), "xk_pr_copy_keyframe")

    def knn_match(self, query, train):
        """BFMatcher(NORM_HAMMING).knnMatch(query, train, 2) -> (idx [nq,2], dist [nq,2])."""
        q, qp = _u8(np.asarray(query, np.uint8).reshape(-1, self.desc_bytes))
        t, tp = _u8(np.asarray(train, np.uint8).reshape(-1, self.desc_bytes))
        idx = np.full((q.shape[0], 2), -1, np.int32)
        dist = np.zeros((q.shape[0], 2), np.int32)
        self._chk(self.L.xk_pr_knn_match(self.p, qp, C.c_int(q.shape[0]), tp, C.c_int(t.shape[0]), idx.ctypes.data_as(c_ip),
                                         dist.ctypes.data_as(c_ip)), "xk_pr_knn_match")
        return idx, dist

    def essential_ransac(self, cur_xy, rec_xy, K, threshold_px=1.0, n_hyp=1024, seed=0):
        """cv::findEssentialMat(current, received, K, RANSAC, 0.99, threshold_px, mask) of findCorrespondences
        (place_recognition.cpp:269-281) on the device: cur_xy / rec_xy [n, 2] pixels of the good matches, K = (fx, fy,
        cx, cy) or a 3 x 3 camera matrix -> (mask uint8 [n], E [3, 3] with rec^T E cur = 0, n_inliers).  All n_hyp
        hypotheses are evaluated; the mask is what good_matches takes as inlier_mask."""
        K = np.asarray(K, np.float64)
        fx, fy, cx, cy = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else K.ravel()
        cur = np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2)
        rec = np.ascontiguousarray(rec_xy, np.float32).reshape(-1, 2)
        if len(cur) != len(rec):
            raise ValueError("cur_xy and rec_xy differ in length")
        n = len(cur)
        mask, E, ninl = np.zeros(max(n, 1), np.uint8), np.zeros(9), C.c_int(0)
        c_fp = C.POINTER(C.c_float)
        self._chk(self.L.xk_pr_essential_ransac(self.p, cur.ctypes.data_as(c_fp), rec.ctypes.data_as(c_fp), C.c_int(n), C.c_double(fx),
                                                C.c_double(fy), C.c_double(cx), C.c_double(cy), C.c_double(threshold_px),
                                                C.c_int(n_hyp), C.c_ulong(seed), mask.ctypes.data_as(c_ub), E.ctypes.data_as(c_dp),
                                                C.byref(ninl)), "xk_pr_essential_ransac")
        return mask[:n], E.reshape(3, 3), ninl.value

    def essential_hypotheses(self, first, count):
        """What the last essential_ransac left for hypotheses first ... first+count-1 -> (n_cand [count], E [count, 10, 3, 3]
        of unit Frobenius norm, inliers [count, 10]): the runners-up, and what the solver-level test compares."""
        nc = np.zeros(max(count, 1), np.int32)
        E = np.zeros((max(count, 1), 10, 3, 3))
        inl = np.zeros((max(count, 1), 10), np.int32)
        self._chk(self.L.xk_pr_essential_hypotheses(self.p, C.c_int(first), C.c_int(count), nc.ctypes.data_as(c_ip), E.ctypes.data_as(c_dp),
                                                    inl.ctypes.data_as(c_ip)), "xk_pr_essential_hypotheses")
        return nc[:count], E[:count], inl[:count]

    def find_correspondences(self, rec_desc, rec_xy, cur_desc, cur_xy, counts, min_distance, ratio_thr, K, threshold_px=1.0,
                             n_hyp=1024, seed=0):
        """PlaceRecognition::findCorrespondences (place_recognition.cpp:137-385, non-GT branch) in one call
        (xk_pr_find_correspondences): rec_* the received keyframe (query side), cur_* the current features (train side),
        descriptors [n, desc_bytes] and float32 pixels [n, 2] in MSCKF | SLAM | OPP order; counts = (n_cur_msckf,
        n_cur_slam, n_rec_msckf, n_rec_slam); K as for essential_ransac.  -> dict(status, n_candidates, n_inliers, winner,
        E [3, 3], good [n_good, 2] (query, train), classified [n_classified, 3] (kind 0...3 as x::MatchKind, current,
        received), launches).  The lists are empty for every non-zero status."""
        K = np.asarray(K, np.float64)
        fx, fy, cx, cy = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else K.ravel()
        rd, rdp = _u8(np.asarray(rec_desc, np.uint8).reshape(-1, self.desc_bytes))
        cd, cdp = _u8(np.asarray(cur_desc, np.uint8).reshape(-1, self.desc_bytes))
        rx = np.ascontiguousarray(rec_xy, np.float32).reshape(-1, 2)
        cx_ = np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2)
        if len(rx) != len(rd) or len(cx_) != len(cd):
            raise ValueError("descriptors and pixels of a side differ in length")
        n_rec, n_cur = len(rd), len(cd)
        ncm, ncs, nrm, nrs = (int(c) for c in counts)
        out = XkPrCorrOut()
        good = np.zeros((max(n_rec, 1), 2), np.int32)
        cls = np.zeros((max(n_rec, 1), 3), np.int32)
        c_fp = C.POINTER(C.c_float)
        self._chk(self.L.xk_pr_find_correspondences(
            self.p, rdp, rx.ctypes.data_as(c_fp), C.c_int(n_rec), cdp, cx_.ctypes.data_as(c_fp), C.c_int(n_cur), C.c_int(ncm),
            C.c_int(ncs), C.c_int(nrm), C.c_int(nrs), C.c_double(min_distance), C.c_double(ratio_thr), C.c_double(fx), C.c_double(fy),
            C.c_double(cx), C.c_double(cy), C.c_double(threshold_px), C.c_int(n_hyp), C.c_ulong(seed), C.byref(out),
            good.ctypes.data_as(c_ip), cls.ctypes.data_as(c_ip)), "xk_pr_find_correspondences")
        self._corr_last = (n_rec, out.n_candidates)       # what find_correspondences_stage sizes and cuts its arrays by
        return dict(status=out.status, n_candidates=out.n_candidates, n_inliers=out.n_inliers, winner=out.winner,
                    E=np.array(out.E, np.float64).reshape(3, 3), good=good[:out.n_good].copy(),
                    classified=cls[:out.n_classified].copy(), launches=out.launches)

    def find_correspondences_stage(self):
        """What the last find_correspondences passed between its stages -> dict(candidates [n_candidates, 2] (query, train),
        mask uint8 [n_rec] (the essential filter's, zero past the candidates), remove_ids [n_remove])."""
        n_rec, n_cand = getattr(self, "_corr_last", (0, 0))
        n = max(n_rec, 1)
        cand, mask, rem, nrem = np.zeros((n, 2), np.int32), np.zeros(n, np.uint8), np.zeros(n, np.int32), C.c_int(0)
        self._chk(self.L.xk_pr_find_correspondences_stage(self.p, cand.ctypes.data_as(c_ip), mask.ctypes.data_as(c_ub),
                                                          rem.ctypes.data_as(c_ip), C.byref(nrem)), "xk_pr_find_correspondences_stage")
        return dict(candidates=cand[:n_cand].copy(), mask=mask[:n_rec].copy(), remove_ids=rem[:nrem.value].copy())


def good_matches(idx, dist, min_distance, ratio_thr, inlier_mask=None):
    """Host half of findCorrespondences (place_recognition.cpp:252-301): distance + ratio test on the device's
    2-NN result, optional RANSAC inlier mask (Database.essential_ransac produces it), duplicate removal."""
    good = []
    for q in range(len(idx)):
        if idx[q, 1] < 0:
            continue
        d0, d1 = np.float32(dist[q, 0]), np.float32(dist[q, 1])
        if d0 < min_distance and d0 < d1 * ratio_thr:
            good.append((q, int(idx[q, 0])))
    if not good:
        return []
    if inlier_mask is not None:
        good = [m for m, keep in zip(good, inlier_mask) if keep]
    remove_ids = []
    for i in range(len(good)):
        for j in range(i, len(good)):
            if i != j and (good[i][0] == good[j][0] or good[i][1] == good[j][1]):
                remove_ids.append(j)
                break
    corr = 0
    for r in remove_ids:
        pos = r - corr
        if 0 <= pos < len(good):
            del good[pos]
        corr += 1
    return good


def classify(good, n_cur_msckf, n_cur_slam, n_rec_msckf, n_rec_slam):
    """place_recognition.cpp:311-388: which kind of collaborative match each (received, current) pair is."""
    max_cur_msckf, max_cur_slam = n_cur_msckf, n_cur_msckf + n_cur_slam
    max_rec_msckf, max_rec_slam = n_rec_msckf, n_rec_msckf + n_rec_slam
    out = []
    for q, t in good:
        if q < max_rec_msckf and t >= max_cur_slam:
            out.append(("msckf", t - max_cur_slam, q))
        if max_rec_msckf <= q < max_rec_slam:
            if max_cur_msckf <= t < max_cur_slam:
                out.append(("slam", t - max_cur_msckf, q - max_rec_msckf))
            if t >= max_cur_slam:
                out.append(("opp_slam", t - max_cur_slam, q - max_rec_msckf))
        if q >= max_rec_slam and t >= max_cur_slam:
            out.append(("opp_opp", t - max_cur_slam, q - max_rec_slam))
    return out


class VocabularyTrainer:
    """DBoW3's Vocabulary::create on one agent's GPU (xk_voc_*): add descriptor rows in any number of pieces, then train.
    The tree is bit-defined by (descriptors in the order added, k, L, seed, max_iter): DESIGN 3.15."""

    def __init__(self, eng, k, L, desc_bytes=32, max_desc=1 << 16):
        self.eng, self.L = eng, eng.L
        self.k, self.Lv, self.desc_bytes, self.max_desc = int(k), int(L), int(desc_bytes), int(max_desc)
        self.p = C.c_void_p()
        rc = self.L.xk_voc_create(eng.h, C.c_int(self.k), C.c_int(self.Lv), C.c_int(self.desc_bytes), C.c_int(self.max_desc),
                                  C.byref(self.p))
        if rc != 0:
            raise XkError(rc, "xk_voc_create", (self.L.xk_last_error(eng.h) or b"").decode())

    def close(self):
        if self.p:
            self.L.xk_voc_destroy(self.p)
            self.p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise XkError(rc, what, (self.L.xk_last_error(self.eng.h) or b"").decode())

    def __len__(self):
        return int(self.L.xk_voc_count(self.p))

    def add(self, descriptors):
        d, dp = _u8(np.asarray(descriptors, np.uint8).reshape(-1, self.desc_bytes))
        self._chk(self.L.xk_voc_add(self.p, dp, C.c_int(d.shape[0])), "xk_voc_add")

    def clear(self):
        self._chk(self.L.xk_voc_clear(self.p), "xk_voc_clear")

    def train(self, seed=0, max_iter=100):
        """-> the dict load_vocabulary returns (k, L, desc, children, word_of_node, node_of_word) plus `outcome`: n_nodes,
        n_words, levels, level_nodes, level_passes, capped_nodes, launches, host_waits."""
        oc = XkVocOutcome()
        self._chk(self.L.xk_voc_train(self.p, C.c_ulong(seed), C.c_int(max_iter), C.byref(oc)), "xk_voc_train")
        desc = np.zeros((oc.n_nodes, self.desc_bytes), np.uint8)
        ch = np.full((oc.n_nodes, self.k), -1, np.int32)
        won = np.full(oc.n_nodes, -1, np.int32)
        now = np.zeros(oc.n_words, np.int32)
        self._chk(self.L.xk_voc_get(self.p, desc.ctypes.data_as(c_ub), ch.ctypes.data_as(c_ip), won.ctypes.data_as(c_ip),
                                    now.ctypes.data_as(c_ip)), "xk_voc_get")
        outcome = dict(n_nodes=oc.n_nodes, n_words=oc.n_words, levels=oc.levels, level_nodes=list(oc.level_nodes)[:self.Lv],
                       level_passes=list(oc.level_passes)[:self.Lv], capped_nodes=oc.capped_nodes, launches=oc.launches,
                       host_waits=oc.host_waits)
        return dict(k=np.int32(self.k), L=np.int32(self.Lv), desc=desc, children=ch, word_of_node=won, node_of_word=now,
                    outcome=outcome)


def train_vocabulary(eng, descriptors, k, L, seed=0, max_iter=100, max_desc=None):
    """Vocabulary::create(training_features, k, L) on the device -> the dict of VocabularyTrainer.train.  It goes straight
    into Database(eng, voc, ...) and, without `outcome`, into np.savez."""
    d = np.ascontiguousarray(descriptors, np.uint8)
    if d.ndim != 2:
        raise ValueError("descriptors must be [n, desc_bytes]")
    tr = VocabularyTrainer(eng, k, L, d.shape[1], max_desc if max_desc else max(len(d), 1))
    try:
        tr.add(d)
        return tr.train(seed, max_iter)
    finally:
        tr.close()
