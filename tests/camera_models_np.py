"""NumPy restatement of the tracker's camera models (xk_trk_camera_model), written from the definition and not from the
device code: the forward map and its Newton inverse of the radial-tangential and the equidistant model, vectorised over points.

Everything is fp64 on conditioned coordinates x = (u - cx)/fx, y = (v - cy)/fy; results go back to pixels as x fx + cx, y fy + cy.
K = (fx, fy, cx, cy).  Model 0 (FOV) is fundamental_np.undistort / distort and is not restated again.

undistort returns (xy, state, steps, detj): per point the undistorted pixel, CONVERGED or INVALID, the Newton steps taken and the
derivative at the solution (det J for the radial-tangential model, d theta_d / d theta for the equidistant one; nan where there is
none).  An invalid point keeps its distorted pixel."""
import numpy as np

FOV, RADTAN, EQUIDISTANT = 0, 1, 2
CONVERGED, INVALID = 0, 1
MAX_STEPS = 20
RADTAN_TOL = 1e-28
EQUI_TOL = 1e-14
EQUI_RMIN = 1e-8


def _coeffs(model, coeffs):
    k = [float(v) for v in coeffs]
    if model == RADTAN:
        assert len(k) in (4, 5)
        return k + [0.0] * (5 - len(k))
    assert model == EQUIDISTANT and len(k) == 4
    return k


def _plane(xy, K):
    fx, fy, cx, cy = K
    p = np.asarray(xy, np.float64).reshape(-1, 2)
    return (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy


def _pixels(x, y, K):
    fx, fy, cx, cy = K
    return np.stack([x * fx + cx, y * fy + cy], axis=1)


def radtan_forward(k, x, y):
    k1, k2, p1, p2, k3 = k
    r2 = x * x + y * y
    g = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return x * g + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x), y * g + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y


def radtan_jacobian(k, x, y):
    """[[dxd/dx, dxd/dy], [dyd/dx, dyd/dy]] as four arrays."""
    k1, k2, p1, p2, k3 = k
    r2 = x * x + y * y
    g = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    dg = k1 + r2 * (2.0 * k2 + 3.0 * k3 * r2)                 # dg / d(r^2); d(r^2)/dx = 2x
    a = g + 2.0 * x * x * dg + 2.0 * p1 * y + 6.0 * p2 * x
    b = 2.0 * x * y * dg + 2.0 * p1 * x + 2.0 * p2 * y
    d = g + 2.0 * y * y * dg + 6.0 * p1 * y + 2.0 * p2 * x
    return a, b, b, d


def equi_theta_d(k, th):
    t2 = th * th
    return th * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))


def equi_dtheta_d(k, th):
    t2 = th * th
    return 1.0 + t2 * (3.0 * k[0] + t2 * (5.0 * k[1] + t2 * (7.0 * k[2] + t2 * 9.0 * k[3])))


def distort(xy, K, model, coeffs):
    """Undistorted pixels [n, 2] -> distorted pixels [n, 2]."""
    k = _coeffs(model, coeffs)
    x, y = _plane(xy, K)
    if model == RADTAN:
        xd, yd = radtan_forward(k, x, y)
        return _pixels(xd, yd, K)
    r = np.sqrt(x * x + y * y)
    scale = np.ones(len(r))
    big = r > EQUI_RMIN
    scale[big] = equi_theta_d(k, np.arctan(r[big])) / r[big]
    return _pixels(x * scale, y * scale, K)


def undistort(dist_xy, K, model, coeffs):
    k = _coeffs(model, coeffs)
    d = np.asarray(dist_xy, np.float64).reshape(-1, 2)
    xd, yd = _plane(d, K)
    n = len(xd)
    state = np.full(n, INVALID, np.int32)
    steps = np.zeros(n, np.int32)
    detj = np.full(n, np.nan)
    live = np.ones(n, bool)                                   # still iterating
    with np.errstate(all="ignore"):
        if model == RADTAN:
            x, y = xd.copy(), yd.copy()
            for it in range(MAX_STEPS):
                i = np.flatnonzero(live)
                if not len(i):
                    break
                a, b, c, e = radtan_jacobian(k, x[i], y[i])
                det = a * e - b * c
                ok = det > 0.0                                # (false for a NaN)
                live[i[~ok]] = False                          # folded: invalid, the loop ends
                i, a, b, c, e, det = i[ok], a[ok], b[ok], c[ok], e[ok], det[ok]
                fx_, fy_ = radtan_forward(k, x[i], y[i])
                rx, ry = fx_ - xd[i], fy_ - yd[i]
                dx, dy = -(e * rx - b * ry) / det, -(a * ry - c * rx) / det
                x[i] += dx
                y[i] += dy
                steps[i] = it + 1
                conv = dx * dx + dy * dy <= RADTAN_TOL * (1.0 + x[i] * x[i] + y[i] * y[i])
                state[i[conv]] = CONVERGED
                live[i[conv]] = False
            a, b, c, e = radtan_jacobian(k, x, y)
            detj = np.where(state == CONVERGED, a * e - b * c, np.nan)
        else:
            rd = np.sqrt(xd * xd + yd * yd)
            small = rd <= EQUI_RMIN
            state[small] = CONVERGED
            live[small] = False
            live[~(rd == rd)] = False                         # (a NaN radius: invalid)
            th = rd.copy()
            for it in range(MAX_STEPS):
                i = np.flatnonzero(live)
                if not len(i):
                    break
                der = equi_dtheta_d(k, th[i])
                ok = der > 0.0
                live[i[~ok]] = False
                i, der = i[ok], der[ok]
                dth = -(equi_theta_d(k, th[i]) - rd[i]) / der
                th[i] += dth
                steps[i] = it + 1
                inside = (th[i] > 0.0) & (th[i] < np.pi / 2)
                live[i[~inside]] = False
                conv = inside & (np.abs(dth) <= EQUI_TOL * (1.0 + np.abs(th[i])))
                state[i[conv]] = CONVERGED
                live[i[conv]] = False
            scale = np.ones(n)
            big = (state == CONVERGED) & ~small
            scale[big] = np.tan(th[big]) / rd[big]
            x, y = xd * scale, yd * scale
            detj = np.where(big, equi_dtheta_d(k, th), np.where(small, 1.0, np.nan))
    out = _pixels(x, y, K)
    bad = (state != CONVERGED) | ~np.isfinite(out).all(axis=1)
    state[bad] = INVALID
    out[bad] = d[bad]
    detj[bad] = np.nan
    return out, state, steps, detj
