"""xk_trk_frame and xk_trk_photo_frame under a radial-tangential lens (xk_trk_camera_model): four frames of the `walk`
scene of tests/tracker_frame_cases.py (and of `gain_walk` of tests/photo_frame_cases.py) with the EUROC coefficients on the scene's
camera.  The frame fills its undistortion from the xk_trk as the stage entries do, so the frames' result blocks equal, byte for byte,
the same frames chained through the stage entries under the same model; and the lens is really applied: the undistorted pixels are
more than a pixel away from those of an s = 0 run."""
import numpy as np
import pytest

import camera_models_cases as cc
import photo_frame_cases as pc
import photo_frame_chain as pch
import tracker_frame_cases as tc
import tracker_frame_chain as tfc

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
COUNTS = tracker.FrameOut.COUNTS
N_FRAMES = 4


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(4, 0, 4)
    yield e
    e.close()


def run(eng, rig_type, sc, runner, euroc, frame=True, **kw):
    rig = rig_type(eng, sc, frame=frame)
    try:
        if euroc:
            rig.mf.camera_model(*cc.EUROC)
        out = runner(rig, [sc["sequences"][0][:N_FRAMES]], **kw)[0]
        return out, rig.mf.undistort_status()
    finally:
        rig.close()


def same_blocks(got, ref, arrays, feature_keys):
    matches = 0
    for fi, (g, r) in enumerate(zip(got, ref)):
        assert not isinstance(g, Exception) and not isinstance(r, Exception), (fi, g, r)
        for key in COUNTS:
            if key in r:
                assert g[key] == r[key], (fi, key)
        for key in arrays:
            if r[key] is not None:
                assert g[key].tobytes() == r[key].tobytes(), (fi, key)
        for key in feature_keys:
            assert g["features"][key].tobytes() == r["features"][key].tobytes(), (fi, key)
        matches += g["n_matches"]
    assert matches >= 3 * 7                                     # every frame past the first kept something


def bend(frames):
    """The largest distance of a match's undistorted pixel from its distorted one over the frames."""
    worst = 0.0
    for f in frames[1:]:
        for und, dist in ((f["prev_xy"], f["prev_dist_xy"]), (f["cur_xy"], f["cur_dist_xy"])):
            if len(und):
                worst = max(worst, float(np.linalg.norm(und - dist, axis=1).max()))
    return worst


def test_frame_equals_the_chain_under_the_model(eng):
    sc = tc.SCENES["walk"]
    got, status = run(eng, tfc.Rig, sc, tfc.run_frames, True)
    ref, _ = run(eng, tfc.Rig, sc, tfc.run_chain, True, frame=False)
    assert len(got) == len(ref) == N_FRAMES
    same_blocks(got, ref, tfc.ARRAYS, ("dist_xy", "score", "desc"))
    assert status[0] == 0 and 1 <= status[1] <= 20              # the last frame's undistortion: every point valid
    # an s = 0 run leaves the pixels where they are (up to the pinhole arithmetic); under the lens they move by more than a pixel
    plain, plain_status = run(eng, tfc.Rig, sc, tfc.run_frames, False)
    print("bend [px]: EUROC", bend(got), "s = 0", bend(plain))
    assert plain_status == (0, 0)
    assert bend(plain) <= 1e-9 and bend(got) > 1.0
    # the same distorted pixel, kept by both runs, undistorts more than a pixel apart
    apart = 0.0
    for g, p in zip(got[1:], plain[1:]):
        at = {d.tobytes(): u for d, u in zip(p["cur_dist_xy"], p["cur_xy"])}
        for d, u in zip(g["cur_dist_xy"], g["cur_xy"]):
            if d.tobytes() in at:
                apart = max(apart, float(np.linalg.norm(u - at[d.tobytes()])))
    print("same feature, EUROC against s = 0 [px]:", apart)
    assert apart > 1.0


def test_photo_frame_equals_the_chain_under_the_model(eng):
    sc = pc.SCENES["gain_walk"]
    got, status = run(eng, pch.PhotoRig, sc, pch.run_frames, True, state=False)
    ref, _ = run(eng, pch.PhotoRig, sc, pch.run_chain, True, frame=False, state=False)
    assert len(got) == len(ref) == N_FRAMES
    same_blocks(got, ref, pch.ARRAYS, ("dist_xy", "score", "desc", "intensity"))
    for g, r in zip(got, ref):
        for key in pch.CAL:
            if key in g and key in r:
                assert np.asarray(g[key], np.float64).tobytes() == np.asarray(r[key], np.float64).tobytes(), key
    assert status[0] == 0 and status[1] >= 1
    assert bend(got) > 1.0
