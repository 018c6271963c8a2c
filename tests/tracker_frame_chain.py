"""What tests/test_gpu_tracker_frame.py and tools/bench_tracker_frame.py share: a tracker with a scene's setups (Rig), its sequences
through xk_trk_frame (run_frames), and the same frames through the CHAIN of the stage entries driven through the host (Chain,
run_chain) as host/examples/klt_main.cpp drives them and as every caller did before xk_trk_frame: push, track, the overflow pass on
the host (FeatureTracker::removeOverflow), detect, describe, track, filter_matches."""
import numpy as np

import fast_np as fastnp
import klt_cases as kc
import tracker_frame_cases as tc
import tracker_frame_np as tnp

from x_multi_agent_amd import engine, tracker

ARRAYS = ("prev_xy", "cur_xy", "prev_dist_xy", "cur_dist_xy", "score", "origin", "tiles", "desc")


class Rig:
    """A MatchFilter and a Klt on one xk_trk with a scene's setups; frame=False: without the frame setup (the chain's side)."""

    def __init__(self, eng, sc, frame=True):
        self.sc = sc
        self.mf = tracker.MatchFilter(eng, sc["max_matches"], sc.get("K", kc.K_CHAIN), 0.0)
        try:
            self.k = k = tracker.Klt(eng, 0, sc.get("width", tc.W), sc.get("height", tc.H), sc["win"], sc["max_level"], sc["max_iter"], sc["eps"], sc["min_eig_thr"], match_filter=self.mf)
            k.detect_setup(sc["threshold"], sc["non_max_supp"], sc["block_half_length"], sc["margin"], sc["max_candidates"])
            d = sc["describe"]
            if d is not None:
                k.describe_setup(d["centroid"], d["angle_deg"], d["edge"], None, d["max_desc"])
            if frame:
                self.frame_setup()
        except Exception:
            self.close()
            raise

    def frame_setup(self):
        sc = self.sc
        self.k.frame_setup(sc["n_feat_min"], sc["n_tiles_h"], sc["n_tiles_w"], sc["max_feat_per_tile"], sc["threshold_px"], sc["n_hyp"])

    def close(self):
        if getattr(self, "k", None) is not None:
            self.k.close()
        self.mf.close()


def run_frames(rig, sequences):
    """Every sequence through xk_trk_frame (a reset before each after the first) -> per sequence, per frame: the frame's dict with
    `features` (the resident list after it), or the XkError."""
    out = []
    for si, seq in enumerate(sequences):
        if si:
            rig.k.frame_reset()
        frames = []
        for i, img in enumerate(seq):
            try:
                r = rig.k.frame(img, seed=tc.SEED + i)
                r["features"] = rig.k.frame_features()
            except engine.XkError as e:
                r = e
            frames.append(r)
        out.append(frames)
    return out


class Chain:
    """Tracker::track strung through the host over the stage entries, as the callers of the parent commit do it."""

    def __init__(self, rig):
        self.rig, self.sc, self.features = rig, rig.sc, None
        self.grid = fastnp.TileGrid(self.sc.get("width", tc.W), self.sc.get("height", tc.H), self.sc["n_tiles_h"], self.sc["n_tiles_w"], self.sc["max_feat_per_tile"])

    def _detect(self, which, old_xy, counts):
        k = self.rig.k
        try:
            d = k.detect(which, old_xy)
        except engine.XkError as e:
            counts["n_candidates"], counts["n_accepted"] = e.n_candidates, e.n_found
            e.counts = counts
            raise
        counts["n_candidates"], counts["n_accepted"] = d["n_candidates"], len(d["xy"])
        desc = np.zeros((len(d["xy"]), 32), np.uint8)
        if self.sc["describe"] is not None:
            try:
                o = k.describe(d["xy"], which)
            except engine.XkError as e:
                e.counts = counts
                raise
            assert len(o["keep_idx"]) == len(d["xy"])
            desc = o["desc"]
        return d["xy"].astype(np.float64), d["score"], desc

    def frame(self, img, seed):
        k, mf, sc = self.rig.k, self.rig.mf, self.sc
        counts = dict(n_tracked=0, n_left=0, redetected=0, n_candidates=0, n_accepted=0, n_new_tracked=0, n_matches=0)
        feats, self.features = self.features, None
        k.push_image(img)
        if feats is None:
            xy, score, desc = self._detect(1, None, counts)
            self.features = dict(dist_xy=xy, score=score, desc=desc)
            return dict(counts, **{a: None for a in ARRAYS})
        r = k.track(feats["dist_xy"].astype(np.float32))
        keep = r["keep_idx"]
        prev, cur = feats["dist_xy"][keep], r["kept_cur"]
        score, desc, origin = feats["score"][keep], feats["desc"][keep], keep.astype(np.int32)
        counts["n_tracked"] = len(keep)
        stay, tiles_prev, tiles_cur = fastnp.remove_overflow(self.grid, prev.tolist(), cur.tolist())    # FeatureTracker::removeOverflow
        stay = np.asarray(stay, np.int64)
        tiles = np.array([tiles_prev[i] + tiles_cur[i] for i in stay], np.int32).reshape(-1, 4)
        prev, cur, score, desc, origin = prev[stay], cur[stay], score[stay], desc[stay], origin[stay]
        counts["n_left"] = len(stay)
        if len(stay) < sc["n_feat_min"]:
            counts["redetected"] = 1
            nxy, nscore, ndesc = self._detect(0, prev, counts)
            r2 = k.track(nxy.astype(np.float32))
            k2 = r2["keep_idx"]
            counts["n_new_tracked"] = len(k2)
            ntiles = np.array([self.grid.tile(*nxy[j]) + tnp.NEW_TILE for j in k2], np.int32).reshape(-1, 4)
            prev, cur = np.concatenate([prev, nxy[k2]]), np.concatenate([cur, r2["kept_cur"]])
            score, desc = np.concatenate([score, nscore[k2]]), np.concatenate([desc, ndesc[k2]])
            origin, tiles = np.concatenate([origin, -(k2.astype(np.int32) + 1)]), np.concatenate([tiles, ntiles])
        try:
            mask, m, pxy, cxy = mf.filter_matches(prev, cur, sc["threshold_px"], sc["n_hyp"], seed)
        except engine.XkError as e:
            e.counts = counts
            raise
        counts["n_matches"] = len(m)
        self.features = dict(dist_xy=cur[m], score=score[m], desc=desc[m])
        return dict(counts, prev_xy=pxy, cur_xy=cxy, prev_dist_xy=prev[m], cur_dist_xy=cur[m], score=score[m], origin=origin[m],
                    tiles=tiles[m], desc=desc[m])


def run_chain(rig, sequences):
    out = []
    for seq in sequences:
        c = Chain(rig)
        frames = []
        for i, img in enumerate(seq):
            try:
                r = c.frame(img, tc.SEED + i)
                r["features"] = c.features
            except engine.XkError as e:
                r = e
            frames.append(r)
        out.append(frames)
    return out
