"""Independent NumPy restatement of the range-facet row (RangeUpdate::processRangedFacet, range_update.cpp:61-270) and the sun-sensor
rows (SolarUpdate::processSunAngle, solar_update.cpp:36-94), and of their place in VioUpdater::constructUpdate (vio_updater.cpp:352-423)
-> applyQRDecomposition (:487-512) -> Updater::applyUpdate.  Composes with oracle.ref_np, which stays as it is."""
import numpy as np

from oracle import ref_np as R

K_CORE = 15
RAD2DEG = 57.2957795130
CHI2_1_090 = 2.705543454095404               # boost quantile(chi_squared(1), 0.9), range_update.cpp:250-251
# solar_update.cpp:47-56: S_q_I written (w, x, y, z), G_sun, var_sun (deg^2)
SUN_CALIB = np.array([0.360346005598587, -0.063338979194957, 0.007502445522018, 0.930635612981541,
                      -0.29385515271891938, -0.55080445540063927, 0.78119370269565391, 10000 * 0.01777777777])


def _wxyz_to_xyzw(q):
    return np.array([q[1], q[2], q[3], q[0]], float)


def facet_points(C_q_G, G_p_C, feat, anchor_idxs, facet):
    """Cartesian world positions of the three facet features (range_update.cpp:76-105)."""
    out = []
    for fid in facet:
        al, be, rh = feat[3 * fid:3 * fid + 3]
        a = int(anchor_idxs[fid])
        out.append(1.0 / rh * R.quat_to_rot(C_q_G[a]) @ np.array([al, be, 1.0]) + np.asarray(G_p_C[a], float))
    return out


def range_hat(C_q_G, G_p_C, feat, anchor_idxs, facet, img_pt):
    f = facet_points(C_q_G, G_p_C, feat, anchor_idxs, facet)
    Rn, pn = R.quat_to_rot(C_q_G[-1]), np.asarray(G_p_C[-1], float)
    Gn = np.cross(f[0] - f[1], f[2] - f[1])
    l = np.array([img_pt[0], img_pt[1], 1.0])
    return float((f[1] - pn) @ Gn) / float(l @ (Rn.T @ Gn))


def range_blocks(C_q_G, G_p_C, feat, anchor_idxs, facet, img_pt, n_poses_max):
    """The 11 Jacobian blocks of the range row (range_update.cpp:147-230) as [(first column, 3-vector)], in the reference's order."""
    N = n_poses_max
    f = facet_points(C_q_G, G_p_C, feat, anchor_idxs, facet)
    Rn, pn = R.quat_to_rot(C_q_G[-1]), np.asarray(G_p_C[-1], float)
    Gn = np.cross(f[0] - f[1], f[2] - f[1])
    l = np.array([img_pt[0], img_pt[1], 1.0])
    a = float((f[1] - pn) @ Gn)
    b = float(l @ (Rn.T @ Gn))
    pos = len(C_q_G) - 1
    blocks = [(K_CORE + 3 * pos, -1.0 / b * Gn),
              (K_CORE + 3 * (N + pos), a / b ** 2 * (Gn @ Rn @ R.skew(l)))]
    G_p_r = a / b * Rn @ l + pn
    bary = (f[0] + f[1] + f[2]) / 3.0
    edges = [f[2] - f[1], f[0] - f[2], f[1] - f[0]]
    for j, fid in enumerate(facet):
        al, be, rh = feat[3 * fid:3 * fid + 3]
        an = int(anchor_idxs[fid])
        Ra = R.quat_to_rot(C_q_G[an])
        Jf = 1.0 / b * (Gn / 3.0 + np.cross(edges[j], bary - G_p_r))
        mat = np.eye(3)
        mat[0, 2], mat[1, 2], mat[2, 2] = -al / rh, -be / rh, -1.0 / rh
        blocks += [(K_CORE + 3 * an, Jf),
                   (K_CORE + 3 * (N + an), -1.0 / rh * Jf @ Ra @ R.skew([al, be, 1.0])),
                   (K_CORE + 3 * (2 * N + fid), 1.0 / rh * Jf @ Ra @ mat)]
    return blocks


def range_update(C_q_G, G_p_C, feat, anchor_idxs, facet, img_pt, range_m, P, n_poses_max, sigma_range):
    """RangeUpdate (range_update.cpp:25-270): (h [n], res, r_diag, gamma, inlier).  A gated-out row is a zero row, residual 0,
    variance 1 (the constructor's initial values, :26-30)."""
    n = P.shape[1]
    h = np.zeros(n)
    for c, v in range_blocks(C_q_G, G_p_C, feat, anchor_idxs, facet, img_pt, n_poses_max):
        h[c:c + 3] += v                                   # accumulated: an anchor may be the current pose or another anchor's
    r = range_m - range_hat(C_q_G, G_p_C, feat, anchor_idxs, facet, img_pt)
    var = sigma_range ** 2
    gamma = r * r / float(h @ P @ h + var)
    if gamma < CHI2_1_090:
        return h, r, var, gamma, True
    return np.zeros(n), 0.0, 1.0, gamma, False


def sun_angles_hat(q_xyzw, calib=None):
    c = SUN_CALIB if calib is None else np.asarray(calib, float)
    Rs = R.quat_to_rot(_wxyz_to_xyzw(c[:4]))
    g = c[4:7] / np.linalg.norm(c[4:7])
    s = Rs.T @ R.quat_to_rot(q_xyzw).T @ g
    s = s / np.linalg.norm(s)
    return RAD2DEG * np.array([np.arctan2(s[0], s[2]), np.arctan2(s[1], s[2])])


def sun_update(q_xyzw, x_angle, y_angle, n, calib=None):
    """SolarUpdate (solar_update.cpp:25-94): (h [2 x n], res [2], var_sun).  Only columns 6..8 (kIdxQ) are non-zero."""
    c = SUN_CALIB if calib is None else np.asarray(calib, float)
    Rs = R.quat_to_rot(_wxyz_to_xyzw(c[:4]))
    Rq = R.quat_to_rot(q_xyzw)
    g = c[4:7] / np.linalg.norm(c[4:7])
    s = Rs.T @ Rq.T @ g
    s = s / np.linalg.norm(s)
    res = np.array([x_angle, y_angle]) - sun_angles_hat(q_xyzw, c)
    d0, d1 = s[0] ** 2 + s[2] ** 2, s[1] ** 2 + s[2] ** 2
    mat = np.array([[s[2] / d0, 0.0, -s[0] / d0], [0.0, s[2] / d1, -s[1] / d1]])
    h = np.zeros((2, n))
    h[:, 6:9] = RAD2DEG * mat @ Rs.T @ R.skew(Rq.T @ g)
    return h, res, float(c[7])


def stacked_update(sc, range_meas=None, sun=None, P=None, msckf_slam_tracks=None):
    """constructUpdate (vio_updater.cpp:267-423) with the range / sun rows + applyQRDecomposition + applyUpdate, composed from
    oracle.ref_np.  range_meas: dict(range, img_pt, facet, sigma_range); sun: dict(q, x, y[, calib]).
    Returns dict(P, correction, did_qr, range_inlier, range_gamma, h_aux, res_aux, r_aux, ...)."""
    P = sc["P"] if P is None else P
    n = P.shape[0]
    N, sig = sc["n_poses_max"], sc["sigma_img"]
    Cq, Gp = sc["C_q_G"], sc["G_p_C"]
    tracks = [sc["obs_xy"][sc["trk_off"][k]:sc["trk_off"][k + 1]] for k in range(len(sc["trk_off"]) - 1)]
    if tracks:
        jac, res, cov, info = R.msckf_update(tracks, Cq, Gp, P, N, sig)
    else:
        jac, res, cov, info = np.zeros((0, n)), np.zeros(0), np.zeros(0), dict(inlier=np.zeros(0, np.int32))
    out = dict(msckf=info)
    if msckf_slam_tracks:
        jm, rm, cm, minfo, _ = R.msckf_slam_update(msckf_slam_tracks, Cq, Gp, P, N, sig)
        jac, res, cov = np.vstack([jac, jm]), np.concatenate([res, rm]), np.concatenate([cov, cm])
    M = len(sc["slam_anchor_idxs"]) if "slam_anchor_idxs" in sc else 0
    if M:
        js, rs, cs, sinfo = R.slam_update(sc["slam_track_sizes"], sc["slam_z_last"], Cq, Gp, sc["slam_feat"],
                                          sc["slam_anchor_idxs"], P, N, sig)
        jac, res, cov = np.vstack([jac, js]), np.concatenate([res, rs]), np.concatenate([cov, cs])
        out["slam"] = sinfo
    ha, ra, va = [], [], []
    if range_meas is not None:
        h, r, v, g, ok = range_update(Cq, Gp, sc["slam_feat"], sc["slam_anchor_idxs"], range_meas["facet"], range_meas["img_pt"],
                                      range_meas["range"], P, N, range_meas["sigma_range"])
        ha.append(h[None, :]); ra.append([r]); va.append([v])
        out.update(range_inlier=ok, range_gamma=g)
    if sun is not None:
        h, r, v = sun_update(sun["q"], sun["x"], sun["y"], n, sun.get("calib"))
        ha.append(h); ra.append(r); va.append([v, v])
    if ha:
        jac = np.vstack([jac] + ha)
        res = np.concatenate([res] + [np.asarray(x, float) for x in ra])
        cov = np.concatenate([cov] + [np.asarray(x, float) for x in va])
    h, r, cv, did = R.apply_qr_decomposition(jac, res, cov, sig)
    naux = sum(x.shape[0] for x in ha)
    out.update(h=h, res=r, r_diag=cv)
    out.update(did_qr=did, rows_total=jac.shape[0], h_aux=jac[jac.shape[0] - naux:], res_aux=res[len(res) - naux:],
               r_aux=(np.full(naux, sig ** 2) if did else cov[len(cov) - naux:]))
    if h.shape[0] > 0:
        Pn, corr = R.apply_update(P, h, r, cv)
    else:
        Pn, corr = P.copy(), np.zeros(n)
    out.update(P=Pn, correction=corr)
    return out
