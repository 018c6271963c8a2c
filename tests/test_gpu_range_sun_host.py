"""The host-side C++ mirror with range and sun readings: x::Ekf -> Updater::update -> VioUpdater::constructUpdate stages the rows under the
reference's conditions (vio_updater.cpp:358, :386), with the IMU attitude as the sun rows' quaternion, and marks each reading used (:380,
:402), so that in the IEKF loop (updater.cpp:99-110) only the first pass carries them.  Covariance owned by the State (the host stacks
xk_aux_rows under the downloaded T_H) or resident on the device.  Against tests/aux_rows_np.py composed with oracle.ref_np."""
import os
import subprocess

import numpy as np
import pytest

import aux_rows_np as A
from helpers import rel
from x_multi_agent_amd import synth

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(__file__), "..", "x_multi_agent_amd")
R = A.R


def _state(sc, sun, seed):
    N, M = sc["n_poses_max"], len(sc["slam_anchor_idxs"])
    npz = len(sc["G_p_C"])
    rng = np.random.default_rng(seed)
    q = np.zeros((N, 4)); q[:, 3] = 1.0; q[:npz] = sc["C_q_G"]
    p = np.zeros((N, 3)); p[:npz] = sc["G_p_C"]
    return dict(p=rng.normal(size=3), v=rng.normal(size=3), q=np.asarray(sun["q"], float), b_w=0.01 * rng.normal(size=3),
                b_a=0.1 * rng.normal(size=3), p_array=p.ravel(), q_array=q.ravel(), f_array=sc["slam_feat"][:3 * M].copy())


def _oracle_iekf(sc, st, rm, sun, iekf_iter):
    """Updater::update's loop with constructUpdate re-reading the window / features from the state corrected so far; the range / sun
    rows only in the first pass (the measurement's timestamp is -1 after it), the sun rows at the state's IMU attitude."""
    n, npz = sc["P"].shape[0], len(sc["G_p_C"])
    s = {k: np.array(v, float, copy=True) for k, v in st.items()}
    ctot = np.zeros(n)
    Pn = sc["P"].copy()
    for it in range(iekf_iter):
        last = it == iekf_iter - 1
        scx = dict(sc)
        scx["C_q_G"] = s["q_array"].reshape(-1, 4)[:npz].copy()
        scx["G_p_C"] = s["p_array"].reshape(-1, 3)[:npz].copy()
        scx["slam_feat"] = s["f_array"].copy()
        sx = None if it > 0 else dict(q=s["q"].copy(), x=sun["x"], y=sun["y"])
        o = A.stacked_update(scx, range_meas=rm if it == 0 else None, sun=sx)
        Pn, corr = R.apply_update(sc["P"], o["h"], o["res"], o["r_diag"], ctot, last)
        s = R.state_correct(s, corr)
        ctot = ctot + corr
        if it == 0:
            first = o
    return dict(P=Pn, state=s, inlier=o["msckf"]["inlier"], first=first)


def _run(tmp_path, sc, st, rm, sun, iekf_iter, resident):
    exe = os.path.join(PKG, "xk_host_example")
    if not os.path.exists(exe):
        from x_multi_agent_amd import build
        build.build_host()
    N, M, K = sc["n_poses_max"], len(sc["slam_anchor_idxs"]), len(sc["trk_off"]) - 1
    n = sc["P"].shape[0]
    parts = [np.array([N, M, K, len(sc["G_p_C"]), sc["sigma_img"]], float), st["q_array"], st["p_array"],
             np.diff(sc["trk_off"]).astype(float), sc["obs_xy"].ravel(), st["f_array"], sc["slam_anchor_idxs"].astype(float),
             sc["slam_z_last"].ravel(), sc["slam_track_sizes"].astype(float), np.asfortranarray(sc["P"]).ravel(order="F")]
    fin, fout, fcore, faux = (str(tmp_path / f) for f in ("in.bin", "out.bin", "core.bin", "aux.bin"))
    np.concatenate(parts).astype("<f8").tofile(fin)
    np.concatenate([st["p"], st["v"], st["q"], st["b_w"], st["b_a"]]).astype("<f8").tofile(fcore)
    aux = [0.0] * 8 if rm is None else [1.0, rm["range"], rm["img_pt"][0], rm["img_pt"][1], *map(float, rm["facet"]), rm["sigma_range"]]
    aux += [0.0, 0.0, 0.0] if sun is None else [1.0, sun["x"], sun["y"]]
    np.array(aux, "<f8").tofile(faux)
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, fin, fout, str(iekf_iter), str(int(resident)), fcore, faux], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(fout, dtype="<f8")
    at = n * n
    got = dict(P=out[:at].reshape(n, n, order="F"), p_array=out[at:at + 3 * N], q_array=out[at + 3 * N:at + 7 * N],
               f_array=out[at + 7 * N:at + 7 * N + 3 * M])
    at += 7 * N + 3 * M
    got["inlier"] = out[at:at + K].astype(int)
    dyn = out[at + K:at + K + 16]
    got.update(p=dyn[0:3], v=dyn[3:6], q=dyn[6:10], b_w=dyn[10:13], b_a=dyn[13:16])
    return got


CASES = {
    "compressed": lambda: synth.make_scenario(8, 30, 6, seed=9901, err_scale=0.3),    # 403 rows > n + 1: every row sigma_img^2
    "uncompressed": lambda: synth.make_scenario(8, 3, 6, seed=9902, err_scale=0.3),   # 54 rows: sigma_range^2, var_sun
}


@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("iekf_iter", [1, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_frame_through_the_cpp_mirror(tmp_path, name, iekf_iter, resident):
    sc = CASES[name]()
    rm, sun = synth.make_range(sc, (0, 2, 5)), synth.make_sun(991, err_deg=2.0)
    st = _state(sc, sun, 17)
    exp = _oracle_iekf(sc, st, rm, sun, iekf_iter)
    assert exp["first"]["range_inlier"] and exp["first"]["did_qr"] == (name == "compressed")
    got = _run(tmp_path, sc, st, rm, sun, iekf_iter, resident)
    assert np.array_equal(got["inlier"], exp["inlier"].astype(int))
    assert rel(got["P"], exp["P"]) <= 1e-8, rel(got["P"], exp["P"])
    for k in ("p", "v", "q", "b_w", "b_a", "p_array", "q_array", "f_array"):
        assert rel(got[k], exp["state"][k]) <= 1e-8, k
    # the rows mattered: without them the posterior is elsewhere
    o = A.stacked_update(sc)
    if iekf_iter == 1:
        assert rel(got["P"], R.apply_update(sc["P"], o["h"], o["res"], o["r_diag"])[0]) > 1e-6
