"""What tests/test_gpu_photo_frame.py and tools/bench_photo_frame.py share: a tracker with a photometric scene's setups (PhotoRig),
its sequences through xk_trk_photo_frame (run_frames), and the same frames through the CHAIN of the stage entries driven through
the host (PhotoChain, run_chain) as every caller of a PHOTOMETRIC_CALI build did before xk_trk_photo_frame: push_image,
photo_calibrate, track, photo_intensity, the overflow pass on the host, detect, photo_intensity, describe, track, photo_intensity,
filter_matches -- and detect_setup with threshold_photo once a calibrate reports an estimate (tracker.cpp:848).  The chain uses only
entries that exist without the photometric frame."""
import numpy as np

import fast_np as fastnp
import photo_frame_cases as pc
import tracker_frame_chain as tfc
import tracker_frame_np as tnp

from x_multi_agent_amd import engine

ARRAYS = tfc.ARRAYS + ("prev_intensity", "cur_intensity")
CAL = ("n_cal_kept", "estimated", "done", "support", "a_rel", "b_rel", "frame_ab")


class PhotoRig(tfc.Rig):
    """tracker_frame_chain.Rig with the scene's photometric setups; frame=False: without the two frame setups (the chain's side)."""

    def __init__(self, eng, sc, frame=True):
        super().__init__(eng, sc, frame=False)
        try:
            self.photo_setup()
            if frame:
                self.frame_setup()
                self.k.photo_frame_setup(sc["n_hyp_photo"], sc["threshold_photo"])
        except Exception:
            self.close()
            raise

    def photo_setup(self):
        sc = self.sc
        self.k.photo_setup(sc["kernel_size"], sc["eps_gap"], sc["eps_base"], sc["photo_max_hyp"])
        sp = sc["spatial"]
        if sp is not None:
            self.k.photo_spatial_setup(sp["div"], sp["coverage_thr"], sp["max_count"], sp["max_rows"])


def state_of(rig):
    """What both sides must agree on after a frame beyond its outputs: the ring, both planes of the current image, the spatial rows."""
    k = rig.k
    s = dict(ring=k.photo_params(), working=k.level(1, 0)[0], raw=k.photo_raw(1))
    if rig.sc["spatial"] is not None:
        s["sp_status"] = k.photo_spatial_status()
        s["sp_rows"] = k.photo_spatial_rows()
    return s


def run_frames(rig, sequences, state=True):
    """Every sequence through xk_trk_photo_frame (a frame reset before each after the first; the photometric state carries over)
    -> per sequence, per frame: the frame's dict with `features` (the resident list and its intensities after it) and `state`, or the
    XkError (with .state)."""
    out = []
    for si, seq in enumerate(sequences):
        if si:
            rig.k.frame_reset()
        frames = []
        for i, img in enumerate(seq):
            try:
                r = rig.k.photo_frame(img, seed=pc.SEED + i, seed_photo=pc.SEED_PHOTO + i)
                r["features"] = dict(rig.k.frame_features(), intensity=rig.k.photo_frame_intensities())
                if state:
                    r["state"] = state_of(rig)
            except engine.XkError as e:
                r = e
                if state:
                    r.state = state_of(rig)
            frames.append(r)
        out.append(frames)
    return out


class PhotoChain:
    """Tracker::track of a PHOTOMETRIC_CALI build strung through the host over the stage entries."""

    def __init__(self, rig):
        self.rig, self.sc, self.features, self.switched = rig, rig.sc, None, False
        self.grid = fastnp.TileGrid(pc.W, pc.H, self.sc["n_tiles_h"], self.sc["n_tiles_w"], self.sc["max_feat_per_tile"])

    def _detect(self, which, old_xy, counts):
        """detect, the accepted features' intensities on the working plane at their integer pixels, describe."""
        k = self.rig.k
        try:
            d = k.detect(which, old_xy)
        except engine.XkError as e:
            counts["n_candidates"], counts["n_accepted"] = e.n_candidates, e.n_found
            e.counts = counts
            raise
        counts["n_candidates"], counts["n_accepted"] = d["n_candidates"], len(d["xy"])
        value = k.photo_intensity(d["xy"], which, 1)[0].copy()
        desc = np.zeros((len(d["xy"]), 32), np.uint8)
        if self.sc["describe"] is not None:
            try:
                o = k.describe(d["xy"], which)
            except engine.XkError as e:
                e.counts = counts
                raise
            assert len(o["keep_idx"]) == len(d["xy"])
            desc = o["desc"]
        return d["xy"].astype(np.float64), d["score"], desc, value

    def _cur_intensity(self, kept_cur):
        return self.rig.k.photo_intensity(np.trunc(kept_cur).astype(np.int32), 1, 0)[0].copy()        # the RAW current plane, tracker.cpp:666

    def frame(self, img, seed, seed_photo):
        k, mf, sc = self.rig.k, self.rig.mf, self.sc
        counts = dict(n_tracked=0, n_left=0, redetected=0, n_candidates=0, n_accepted=0, n_new_tracked=0, n_matches=0)
        cal = dict(n_cal_kept=0, estimated=False, support=0, a_rel=1.0, b_rel=0.0, frame_ab=np.zeros(4))
        feats, self.features = self.features, None
        k.push_image(img)
        if feats is None:
            xy, score, desc, value = self._detect(1, None, counts)
            self.features = dict(dist_xy=xy, score=score, desc=desc, intensity=value)
            return dict(counts, **cal, **{a: None for a in ARRAYS})
        R = len(feats["dist_xy"])
        c = k.photo_calibrate(feats["dist_xy"].astype(np.float32), feats["intensity"], max(1, min(R, sc["n_hyp_photo"])), seed_photo)
        cal = dict(n_cal_kept=len(c["keep_idx"]), estimated=c["estimated"], support=c["support"], a_rel=c["a_rel"], b_rel=c["b_rel"],
                   frame_ab=c["frame_ab"])
        if c["estimated"] and sc["threshold_photo"] >= 0 and not self.switched:                      # tracker.cpp:848
            k.detect_setup(sc["threshold_photo"], sc["non_max_supp"], sc["block_half_length"], sc["margin"], sc["max_candidates"])
            self.switched = True
        r = k.track(feats["dist_xy"].astype(np.float32))
        keep = r["keep_idx"]
        prev, cur = feats["dist_xy"][keep], r["kept_cur"]
        score, desc, origin = feats["score"][keep], feats["desc"][keep], keep.astype(np.int32)
        ip, ic = feats["intensity"][keep], self._cur_intensity(cur)
        counts["n_tracked"] = len(keep)
        stay, tiles_prev, tiles_cur = fastnp.remove_overflow(self.grid, prev.tolist(), cur.tolist())    # FeatureTracker::removeOverflow
        stay = np.asarray(stay, np.int64)
        tiles = np.array([tiles_prev[i] + tiles_cur[i] for i in stay], np.int32).reshape(-1, 4)
        prev, cur, score, desc, origin, ip, ic = prev[stay], cur[stay], score[stay], desc[stay], origin[stay], ip[stay], ic[stay]
        counts["n_left"] = len(stay)
        try:
            if len(stay) < sc["n_feat_min"]:
                counts["redetected"] = 1
                nxy, nscore, ndesc, nint = self._detect(0, prev, counts)
                r2 = k.track(nxy.astype(np.float32))
                k2 = r2["keep_idx"]
                counts["n_new_tracked"] = len(k2)
                ntiles = np.array([self.grid.tile(*nxy[j]) + tnp.NEW_TILE for j in k2], np.int32).reshape(-1, 4)
                prev, cur = np.concatenate([prev, nxy[k2]]), np.concatenate([cur, r2["kept_cur"]])
                score, desc = np.concatenate([score, nscore[k2]]), np.concatenate([desc, ndesc[k2]])
                origin, tiles = np.concatenate([origin, -(k2.astype(np.int32) + 1)]), np.concatenate([tiles, ntiles])
                ip, ic = np.concatenate([ip, nint[k2]]), np.concatenate([ic, self._cur_intensity(r2["kept_cur"])])
            try:
                mask, m, pxy, cxy = mf.filter_matches(prev, cur, sc["threshold_px"], sc["n_hyp"], seed)
            except engine.XkError as e:
                e.counts = counts
                raise
        except engine.XkError as e:
            e.calibration = cal
            raise
        counts["n_matches"] = len(m)
        self.features = dict(dist_xy=cur[m], score=score[m], desc=desc[m], intensity=ic[m])
        return dict(counts, **cal, prev_xy=pxy, cur_xy=cxy, prev_dist_xy=prev[m], cur_dist_xy=cur[m], score=score[m], origin=origin[m],
                    tiles=tiles[m], desc=desc[m], prev_intensity=ip[m], cur_intensity=ic[m])


def run_chain(rig, sequences, state=True):
    out = []
    c = PhotoChain(rig)
    for seq in sequences:
        c.features = None
        frames = []
        for i, img in enumerate(seq):
            try:
                r = c.frame(img, pc.SEED + i, pc.SEED_PHOTO + i)
                r["features"] = c.features
                if state:
                    r["state"] = state_of(rig)
            except engine.XkError as e:
                r = e
                if state:
                    r.state = state_of(rig)
            frames.append(r)
        out.append(frames)
    return out
