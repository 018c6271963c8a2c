"""NumPy restatement of the spatial photometric map (csrc/xk_photo_spatial.hip.h): the statement of DESIGN 3.17 and of the
comment in include/xk.h, written from that statement and from the behaviour of IRPhotoCalib (irPhotoCalib.cpp:162-210,
:314-420), containing none of its text.  fp64 throughout, one rounding per operation where the statement says so (the rows' b,
the ordered sums of c); the two solves are the same Jacobi-preconditioned conjugate gradients the device runs, with NumPy's own
summation order -- the device is compared with the DENSE solutions below, not with these iterates.
tests/test_photo_spatial_np.py verifies this file without a GPU."""
import numpy as np

import photo_np as pnp

TOL = 1.0e-13
N_MAX = 2048


# ---- the grid ----
def grid(width, height, div):
    """-> dict of w, h, div, cw, ch, cells."""
    cw, ch = width // div, height // div
    return dict(w=width, h=height, div=div, cw=cw, ch=ch, cells=cw * ch)


def cell(g, x, y):
    """The cell of pixel (x, y), or -1: outside the image, or in the remainder column / row (x // div >= cw, y // div >= ch)."""
    x, y = int(x), int(y)
    if x < 0 or y < 0 or x >= g["w"] or y >= g["h"]:
        return -1
    cx, cy = x // g["div"], y // g["div"]
    if cx >= g["cw"] or cy >= g["ch"]:
        return -1
    return cy * g["cw"] + cx


# ---- accumulation (irPhotoCalib.cpp:162-202) ----
def new_state(g):
    return dict(count=np.zeros(g["cells"], np.int32), coverage=np.zeros(g["cells"], np.uint8), sid_hist=[], sid_cur=[], b=[], dropped=0)


def add(state, g, ring, groups, frame_back, max_count, max_rows):
    """One ProcessCurrentFrame worth of rows.  ring: the parameter ring AFTER the frame's gains (list or array of (a, b)); groups: list
    of (pix_hist [n, 2], pix_cur [n, 2], o_hist [n], o_cur [n]); state is changed in place."""
    ring = np.asarray(ring, np.float64).reshape(-1, 2)
    last = len(ring) - 1
    for (ph, pc, oh, oc), fb in zip(groups, frame_back):
        if not 1 <= fb <= last:
            raise ValueError("frame_back outside 1 ... ring size - 1")
        a_hc, b_hc = pnp.relative_gains(ring[last - fb][0], ring[last - fb][1], ring[last][0], ring[last][1])
        gain = np.float64(a_hc) - np.float64(b_hc)
        ph, pc = np.asarray(ph).reshape(-1, 2), np.asarray(pc).reshape(-1, 2)
        oh, oc = np.asarray(oh, np.float64), np.asarray(oc, np.float64)
        bv = (oc * gain - oh) + np.float64(b_hc)            # elementwise: one rounding per operation
        for j in range(len(ph)):
            sh, sc = cell(g, ph[j][0], ph[j][1]), cell(g, pc[j][0], pc[j][1])
            if sh < 0 or sc < 0:
                continue
            if sh == sc or state["count"][sh] > max_count:  # (the history cell alone is tested, as in the reference)
                continue
            state["coverage"][sh] = 1
            state["coverage"][sc] = 1
            if len(state["b"]) < max_rows:
                state["sid_hist"].append(sh), state["sid_cur"].append(sc), state["b"].append(bv[j])
            else:
                state["dropped"] += 1
            state["count"][sc] += 1
            state["count"][sh] += 1
    return state


def status(state, g, coverage_thr):
    covered = int(state["coverage"].sum())
    return dict(rows=len(state["b"]), covered=covered, cells=g["cells"], dropped=state["dropped"],
                ready=bool(float(covered) / float(g["cells"]) > float(np.float32(coverage_thr))))


def rows(state):
    return np.array(state["sid_hist"], np.int32), np.array(state["sid_cur"], np.int32), np.array(state["b"], np.float64)


# ---- numbering and the normal equations ----
def number(coverage):
    """Covered cells in ascending cell id -> (var_of_cell int32 [cells] with -1 where not covered, cell_of_var int32 [n])."""
    cov = np.asarray(coverage) != 0
    cell_of_var = np.flatnonzero(cov).astype(np.int32)
    var_of_cell = np.full(len(cov), -1, np.int32)
    var_of_cell[cell_of_var] = np.arange(len(cell_of_var), dtype=np.int32)
    return var_of_cell, cell_of_var


def normal(sid_hist, sid_cur, b, var_of_cell, n):
    """L = A^T A (exact integers, as fp64) and c = A^T b with every entry summed in ascending row order; a row is +1 at the current
    cell's variable and -1 at the history cell's."""
    vh, vc = var_of_cell[sid_hist], var_of_cell[sid_cur]
    L = np.zeros((n, n), np.int64)
    np.add.at(L, (vh, vc), -1)
    np.add.at(L, (vc, vh), -1)
    np.add.at(L, (vh, vh), 1)
    np.add.at(L, (vc, vc), 1)
    c = np.zeros(n)
    idx = np.stack([vc, vh], axis=1).ravel()
    val = np.stack([b, -b], axis=1).ravel()
    np.add.at(c, idx, val)                                   # unbuffered, in index order: row 0's terms, then row 1's, ...
    return L.astype(np.float64), c


def design(sid_hist, sid_cur, var_of_cell, n):
    """The dense A of the rows [rows, n]."""
    A = np.zeros((len(sid_hist), n))
    r = np.arange(len(sid_hist))
    A[r, var_of_cell[sid_cur]] = 1.0
    A[r, var_of_cell[sid_hist]] = -1.0
    return A


# ---- Jacobi-preconditioned conjugate gradients ----
def pcg(A, rhs, diag, cap=None, tol=TOL):
    """-> dict of x, iterations, converged, residual (|r| / |rhs|).  From x = 0; stops when |r|^2 < tol^2 |rhs|^2 or after cap (2 n)
    iterations.  A variable with diag 0 keeps x = 0."""
    n = len(rhs)
    cap = 2 * n if cap is None else cap
    prec = lambda r: np.where(diag > 0, r / np.where(diag > 0, diag, 1.0), 0.0)
    x, r = np.zeros(n), np.array(rhs, np.float64)
    bb = float(r @ r)
    if bb == 0.0:
        return dict(x=x, iterations=0, converged=True, residual=0.0)
    thr = tol * tol * bb
    z = prec(r)
    p, rz, rr = z.copy(), float(r @ z), bb
    it, conv = 0, False
    while it < cap:
        q = A @ p
        alpha = rz / float(p @ q)
        x = x + alpha * p
        r = r - alpha * q
        rr = float(r @ r)
        it += 1
        if rr < thr:
            conv = True
            break
        z = prec(r)
        rz1 = float(r @ z)
        p = z + (rz1 / rz) * p
        rz = rz1
    return dict(x=x, iterations=it, converged=conv, residual=float(np.sqrt(rr / bb)))


def dense_ls(A, b, deg):
    """D^-1/2 pinv(A D^-1/2) b: the least-squares solution with sum deg_i x_i = 0 on every connected component, which is what
    the preconditioned iteration from zero selects.  deg 0 (an isolated variable): x = 0."""
    s = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
    return s * (np.linalg.pinv(A * s[None, :], rcond=1e-10) @ b)


# ---- the Gaussian process ----
def hyper(gp_length=5.0, gp_sigma_f=0.01, gp_sigma_n=0.01):
    """(1 / (2 l^2), sf^2, sn^2) in fp64 from the float values of the hyperparameters."""
    l, sf, sn = (float(np.float32(v)) for v in (gp_length, gp_sigma_f, gp_sigma_n))
    return 1.0 / (2.0 * l * l), sf * sf, sn * sn


def cov(g, cells_a, cells_b, hyp):
    inv2l2, sf2, _ = hyp
    ax, ay = np.asarray(cells_a) % g["cw"], np.asarray(cells_a) // g["cw"]
    bx, by = np.asarray(cells_b) % g["cw"], np.asarray(cells_b) // g["cw"]
    d2 = (ax[:, None] - bx[None, :]) ** 2 + (ay[:, None] - by[None, :]) ** 2
    return sf2 * np.exp(-d2.astype(np.float64) * inv2l2)


def gp_matrix(g, cell_of_var, hyp):
    return cov(g, cell_of_var, cell_of_var, hyp) + hyp[2] * np.eye(len(cell_of_var))


def predict(g, cell_of_var, alpha, hyp):
    """coarse float32 [ch, cw]: the GP mean at every cell."""
    Ks = cov(g, np.arange(g["cells"]), cell_of_var, hyp)
    return (Ks @ alpha).astype(np.float32).reshape(g["ch"], g["cw"])


def upsample(g, coarse):
    """PS[y][x] = coarse[min(y // div, ch - 1)][min(x // div, cw - 1)], float32 [h, w]."""
    yy = np.minimum(np.arange(g["h"]) // g["div"], g["ch"] - 1)
    xx = np.minimum(np.arange(g["w"]) // g["div"], g["cw"] - 1)
    return np.ascontiguousarray(np.asarray(coarse, np.float32)[yy][:, xx])


# ---- EstimateSpatialParameters (irPhotoCalib.cpp:314-420) ----
def estimate(state, g, hyp=None, cap=None, dense=False):
    """-> dict of n, var_of_cell, cell_of_var, L, c, x, alpha, coarse, ps, converged, ls, gp (the two pcg records).  dense = True: the
    two solves by dense factorisations instead (dense_ls, numpy.linalg.solve): what the device is compared with."""
    hyp = hyper() if hyp is None else hyp
    sh, sc, b = rows(state)
    if len(b) == 0:
        raise ValueError("no row accumulated")
    var_of_cell, cell_of_var = number(state["coverage"])
    n = len(cell_of_var)
    if n > N_MAX:
        raise ValueError("more covered cells than n_max")
    L, c = normal(sh, sc, b, var_of_cell, n)
    deg = np.diag(L).copy()
    K = gp_matrix(g, cell_of_var, hyp)
    out = dict(n=n, var_of_cell=var_of_cell, cell_of_var=cell_of_var, L=L, c=c, K=K, deg=deg)
    if dense:
        x = dense_ls(design(sh, sc, var_of_cell, n), b, deg)
        alpha = np.linalg.solve(K, x)
        out.update(x=x, alpha=alpha, converged=True, ls=None, gp=None)
    else:
        ls = pcg(L, c, deg, cap)
        out.update(x=ls["x"], ls=ls, gp=None, alpha=None, converged=False)
        if ls["converged"]:
            gp = pcg(K, ls["x"], np.full(n, hyp[1] + hyp[2]), cap)
            out.update(gp=gp, alpha=gp["x"], converged=gp["converged"])
    if out["converged"]:
        out["coarse"] = predict(g, cell_of_var, out["alpha"], hyp)
        out["ps"] = upsample(g, out["coarse"])
    return out
