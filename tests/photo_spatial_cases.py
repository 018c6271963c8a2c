"""The cases of the spatial photometric map (tests/test_photo_spatial_np.py on the CPU, tests/test_gpu_photo_spatial*.py on the
device): the smallest shapes at which each piece can go wrong, generated from seeds, with the restatement's measured figures and
the bars the device is held to recorded below.

    basic            96 x 64, div 16: 24 cells
    cells48          64 x 48, div 8: 48 cells, 3 of them never touched (n = 45)
    blocks160        128 x 80, div 8: 160 cells -- more unknowns than one row block of the matrix-vector product, two chunks of the scan
    remainder        70 x 50, div 16: 4 x 3 cells, a remainder column (x >= 64) and row (y >= 48): the skip rule and the clamp
    two_components   96 x 64, div 16, no row between the left and the right half: the per-component gauge
    cap              max_count 40, 300 points in two calls: the cap of cell 0 is crossed at point 41 of a chunk, that of cell 7 by the
                     last point of a chunk
    same_cell        every point has sh == sc: no row
    overflow         max_rows 100 is exceeded
    frame_back       three groups, frame_back 1, 2, 3, on a ring of four distinct pairs
"""
import functools

import numpy as np

import photo_spatial_np as snp

MAX_COUNT, MAX_ROWS, THR = 500, 4096, 0.9
EST = {
    "basic": dict(size=(96, 64), div=16, n=(300, 300), seed=11),
    "cells48": dict(size=(64, 48), div=8, n=(500, 500), seed=12, exclude=(5, 20, 47)),
    "blocks160": dict(size=(128, 80), div=8, n=(512, 448, 448), seed=13),
    "remainder": dict(size=(70, 50), div=16, n=(300, 200), seed=14),
    "two_components": dict(size=(96, 64), div=16, n=(300, 300), seed=15, split=3),
}
CAP = dict(size=(96, 64), div=16, max_count=40, A=0, B=7)


def smooth_map(g, seed):
    """A smooth map, one value per cell (float64 [cells]): what the rows are generated from."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 2.0 * np.pi, 2)
    cx, cy = np.arange(g["cells"]) % g["cw"], np.arange(g["cells"]) // g["cw"]
    return 0.05 * np.sin(2.1 * cx / g["cw"] + p[0]) * np.cos(1.7 * cy / g["ch"] + p[1]) + 0.02 * cx / g["cw"]


def points(name):
    """The calls of an EST case: a list of (pix_hist, pix_cur, o_hist, o_cur), one group each.  Noise-free: with the identity
    pair the row of a point reads m[sc] - m[sh] up to the rounding of the intensities."""
    q = EST[name]
    g = snp.grid(q["size"][0], q["size"][1], q["div"])
    m = smooth_map(g, q["seed"])
    rng = np.random.default_rng(q["seed"])
    excl, split = set(q.get("exclude", ())), q.get("split")
    calls = []
    for n in q["n"]:
        ph, pc = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
        j = 0
        while j < n:
            h = rng.integers(0, [g["w"], g["h"]])
            c = h + rng.integers(-2 * g["div"], 2 * g["div"] + 1, 2)
            if rng.random() < 0.03:
                c = h + rng.integers(-200, 201, 2)                   # now and then far outside the image
            sh, sc = snp.cell(g, *h), snp.cell(g, *c)
            if sh in excl or sc in excl:
                continue
            if split is not None and sh >= 0 and sc >= 0 and (sh % g["cw"] < split) != (sc % g["cw"] < split):
                continue
            ph[j], pc[j] = h, c
            j += 1
        base = rng.uniform(0.2, 0.7, n)
        cell_h = np.array([snp.cell(g, *v) for v in ph])
        cell_c = np.array([snp.cell(g, *v) for v in pc])
        oh = base + np.where(cell_h >= 0, m[np.maximum(cell_h, 0)], 0.0)
        oc = base + np.where(cell_c >= 0, m[np.maximum(cell_c, 0)], 0.0)
        calls.append((ph, pc, oh, oc))
    return g, m, calls


def pixel_of(g, s, dx=5, dy=7):
    return (s % g["cw"]) * g["div"] + dx, (s // g["cw"]) * g["div"] + dy


def cap_calls():
    """Two calls of 150 points.  Call 1: points 0 ... 86 have their history pixel in cell A, 87 ... 149 in cell B, the current pixels
    in cells 8 ... 23.  count[A] passes max_count = 40 with point 40 (the 41st), inside the first chunk of 64; count[B] with point
    127, the last of the second chunk.  Call 2: a seeded mix of A, B and every other cell."""
    g = snp.grid(CAP["size"][0], CAP["size"][1], CAP["div"])
    rng = np.random.default_rng(21)
    sh1 = np.where(np.arange(150) < 87, CAP["A"], CAP["B"])
    sc1 = 8 + np.arange(150) % 16
    sh2 = rng.choice([CAP["A"], CAP["B"], 12] + list(range(24)), 150)
    sc2 = (sh2 + 1 + rng.integers(0, 23, 150)) % 24
    calls = []
    for sh, sc in ((sh1, sc1), (sh2, sc2)):
        ph = np.array([pixel_of(g, s) for s in sh], np.int32)
        pc = np.array([pixel_of(g, s, 3, 2) for s in sc], np.int32)
        calls.append((ph, pc, rng.uniform(0.2, 0.7, len(sh)), rng.uniform(0.2, 0.7, len(sh))))
    return g, calls


def same_cell_call():
    g = snp.grid(96, 64, 16)
    rng = np.random.default_rng(22)
    ph = rng.integers(0, [96, 64], (70, 2)).astype(np.int32)
    pc = (ph // 16) * 16 + rng.integers(0, 16, (70, 2)).astype(np.int32)    # another pixel of the same cell
    return g, (ph, pc, rng.uniform(0.2, 0.7, 70), rng.uniform(0.2, 0.7, 70))


# pairs the tests put into the ring through exact gain data o = p (a - b) + b, and the groups of the frame_back case
RING_PAIRS = ((1.04, 0.01), (0.97, -0.02), (1.08, 0.03))


def frame_back_groups():
    g, _, calls = points("basic")
    return g, [tuple(v[:100 + 7 * i] for v in calls[i % 2]) for i in range(3)], (1, 2, 3)


def rel(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def restated(name):
    """An EST case through the restatement with the identity ring -> (g, m, state, iterative estimate, dense estimate)."""
    g, m, calls = points(name)
    st = snp.new_state(g)
    for c in calls:
        snp.add(st, g, [(1.0, 0.0), (1.0, 0.0)], [c], [1], MAX_COUNT, MAX_ROWS)
    return g, m, st, snp.estimate(st, g), snp.estimate(st, g, dense=True)


def measure(name):
    """What the restatement gives on a case: iterations, its error against the dense solutions, the condition numbers, the bars."""
    g, m, st, it, de = restated(name)
    deg = it["deg"]
    s = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
    ev = np.linalg.eigvalsh(it["L"] * s[:, None] * s[None, :])
    ev = ev[ev > 1e-9 * ev.max()]
    cond_l, cond_k = float(ev.max() / ev.min()), float(np.linalg.cond(it["K"]))
    e = dict(x=rel(it["x"], de["x"]), alpha=rel(it["alpha"], de["alpha"]), coarse=rel(it["coarse"], de["coarse"]))
    return dict(n=it["n"], rows=len(st["b"]), ls_it=it["ls"]["iterations"], gp_it=it["gp"]["iterations"], cond_l=cond_l, cond_k=cond_k,
                err=e, bar=bars(e, cond_l, cond_k))


def bars(err, cond_l, cond_k):
    """The bar per quantity: the larger of 10 x the restatement's own error against the dense solution (another summation order,
    exp differing in the last place) and the conditioning's share.  x: cond(L) 1e-13, the stopping tolerance amplified by the
    (gauge-reduced) condition number of the preconditioned Laplacian.  alpha = K^-1 x: cond(K) (that of x, plus 1e-13 of its own).
    coarse = K* alpha, a float: 2^-23 for the cast, plus cond(K) times alpha's (|K*| |d alpha| <= lmax(K) bar |alpha| and
    |alpha| <= |x| / lmin(K))."""
    bx = max(10.0 * err["x"], cond_l * 1e-13)
    ba = max(10.0 * err["alpha"], cond_k * (cond_l + 1.0) * 1e-13)
    bc = max(10.0 * err["coarse"], 2.0 ** -23 + cond_k * cond_k * (cond_l + 1.0) * 1e-13)
    return dict(x=bx, alpha=ba, coarse=bc)


# measure(name) as run on the CPU when the cases were written (errors and condition numbers rounded up): tests/test_photo_spatial_np.py
# checks that the restatement still gives these sizes, iteration counts within 2 and errors inside the bars; the device tests take
# their bars from here (bar(name)), so they do not move with what any run gives.
RECORDED = {
    "basic": dict(n=24, rows=318, ls_it=18, gp_it=10, cond_l=5.01, cond_k=21.7,
                  err=dict(x=1.4e-14, alpha=2.8e-14, coarse=0.0)),
    "cells48": dict(n=45, rows=636, ls_it=23, gp_it=13, cond_l=11.5, cond_k=35.1,
                    err=dict(x=3.9e-14, alpha=8.4e-14, coarse=0.0)),
    "blocks160": dict(n=160, rows=1080, ls_it=45, gp_it=24, cond_l=51.4, cond_k=76.4,
                      err=dict(x=1.5e-14, alpha=1.3e-13, coarse=0.0)),
    "remainder": dict(n=12, rows=178, ls_it=11, gp_it=8, cond_l=2.55, cond_k=12.2,
                      err=dict(x=1.2e-15, alpha=5.8e-14, coarse=0.0)),
    "two_components": dict(n=24, rows=283, ls_it=16, gp_it=10, cond_l=2.59, cond_k=21.7,
                           err=dict(x=4.4e-14, alpha=5.1e-14, coarse=0.0)),
}


def bar(name):
    r = RECORDED[name]
    return bars(r["err"], r["cond_l"], r["cond_k"])
