"""CPU yardstick of the covariance-intersection weight search (not a test): NumPy only.

    minimise  -log det(sum_i w_i M_i)   over   sum_i w_i = 1,  w_i >= LB,      M_i = H_i P_i^-1 H_i^T

by an active-set Newton iteration.  dtype=np.longdouble runs the same arithmetic in extended precision (no LAPACK call
in the loop), which is how the test measures what float64 rounding does to the weights."""
import numpy as np

LB = 1e-4


def info(P, H):
    """M = H P^-1 H^T through the Cholesky factor of P (float64)."""
    X = np.linalg.solve(np.linalg.cholesky(P), H.T)
    return X.T @ X


def _inv(A):                                    # Gauss-Jordan: plain arithmetic, so it keeps longdouble
    n = len(A)
    G = np.concatenate([A, np.eye(n, dtype=A.dtype)], axis=1)
    for k in range(n):
        G[k] = G[k] / G[k, k]
        for r in range(n):
            if r != k:
                G[r] = G[r] - G[r, k] * G[k]
    return G[:, n:]


def logdet(Ms, w):
    return float(np.linalg.slogdet(np.tensordot(np.asarray(w, float), np.asarray(Ms, float), 1))[1])


def grad(Ms, w, dtype=np.float64):
    """g_i = tr(A^-1 M_i) at A = sum w_i M_i."""
    Ms = np.asarray(Ms, dtype)
    Ai = _inv(np.tensordot(np.asarray(w, dtype), Ms, 1))
    return np.array([np.sum(Ai * M) for M in Ms])


def solve(Ms, w0=None, dtype=np.float64, tol=1e-10, cap=50):
    """-> (w, iterations).  Free coordinates F, the rest sit on LB; lam = multiplier of sum w = 1."""
    Ms = np.asarray(Ms, dtype)
    k1 = len(Ms)
    w = np.full(k1, 1.0 / k1, dtype) if w0 is None else np.asarray(w0, dtype).copy()
    lb = dtype(LB)
    for it in range(cap + 1):
        Ai = _inv(np.tensordot(w, Ms, 1))
        B = np.array([Ai @ M for M in Ms])
        g = np.array([np.trace(b) for b in B])
        Hs = np.array([[np.sum(bi * bj.T) for bj in B] for bi in B])
        free = w > lb
        lam = (w[free] @ g[free]) / w[free].sum()
        free |= g > lam * (1 + tol)                                     # release
        lam = (w[free] @ g[free]) / w[free].sum()
        if np.abs(g[free] - lam).max() <= tol * lam:
            return w, it
        while True:                                                     # Newton step on F, sum d = 0
            F = np.flatnonzero(free)
            K = np.zeros((len(F) + 1, len(F) + 1), dtype)
            K[:-1, :-1], K[:-1, -1], K[-1, :-1] = Hs[np.ix_(F, F)], 1, 1
            d = (_inv(K) @ np.append(g[F], dtype(0)))[:-1]
            block = (w[F] <= lb) & (d < 0)
            if not block.any():
                break
            free[F[block]] = False
        neg = d < 0
        alpha = min(dtype(1), ((w[F][neg] - lb) / -d[neg]).min()) if neg.any() else dtype(1)
        w[F] = np.maximum(w[F] + alpha * d, lb)
        r = F[np.argmax(w[F])]
        w[r] += 1 - w.sum()
    raise RuntimeError("ci_weights_ref.solve: no convergence")
