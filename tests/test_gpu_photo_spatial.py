"""xk_trk_photo_spatial_* (csrc/xk_photo_spatial.hip.h) through tracker.Klt and the C ABI, against the NumPy restatement
tests/photo_spatial_np.py on the cases of tests/photo_spatial_cases.py.  Exact: rows, counts, coverage, covered, ready, dropped,
var_of_cell and L; b and c byte for byte; the upsampled map against the device's own coarse map; the correction after an
install, bit for bit; two estimates on the same rows.  x, alpha and coarse are held to the DENSE NumPy solutions within the bars
recorded in the cases file, never to the device's own iteration.  tests/test_photo_spatial_np.py verifies the restatement and
the cases without a GPU."""
import ctypes as C

import numpy as np
import pytest

import photo_cases as pc
import photo_np as pnp
import photo_spatial_cases as sc
import photo_spatial_np as snp

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
c_ub, c_fp = tracker.c_ub, tracker.c_fp
c_ip, c_dp = engine.c_ip, engine.c_dp
XK_EINVAL, XK_ECAPACITY = 1, 6


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(4, 0, 4)
    yield e
    e.close()


def make(eng, size, div, max_features=512, max_count=sc.MAX_COUNT, max_rows=sc.MAX_ROWS, pairs=sc.RING_PAIRS[:1]):
    """A Klt of that size with a photo setup, a spatial setup and the pairs put into the ring -> (k, the device's ring)."""
    k = tracker.Klt(eng, max_features, size[0], size[1], (5, 5), 1)
    k.photo_setup(30, 0.0, 0.0, 64)
    k.photo_spatial_setup(div, sc.THR, max_count, max_rows)
    put_ring(k, pairs)
    return k, k.photo_params()


def put_ring(k, pairs):
    p = np.linspace(0.1, 0.9, 64)
    for a, b in pairs:                                                           # exact data of the pair: every point an inlier
        assert k.photo_gains(p * (a - b) + b, p, (1,), 8, 1)["support"][0] == 64


def same_accumulation(k, st, g):
    """Status, rows, counts and coverage of the device against the restated state, exactly; b byte for byte."""
    got, ref = k.photo_spatial_status(), snp.status(st, g, sc.THR)
    for key in ("rows", "covered", "cells", "ready", "dropped"):
        assert got[key] == ref[key], (key, got, ref)
    r = k.photo_spatial_rows()
    sh, sc_, b = snp.rows(st)
    assert np.array_equal(r["sid_hist"], sh) and np.array_equal(r["sid_cur"], sc_)
    assert r["b"].tobytes() == b.tobytes()
    assert np.array_equal(r["counts"], st["count"]) and np.array_equal(r["coverage"], st["coverage"])


# ---- accumulation and estimate, case by case ----
@pytest.mark.parametrize("name", list(sc.EST))
def test_rows_and_estimate_against_the_restatement(eng, name):
    q = sc.EST[name]
    g, _, calls = sc.points(name)
    k, ring = make(eng, q["size"], q["div"])
    try:
        st = snp.new_state(g)
        for c in calls:
            k.photo_spatial_add(*c, (1,))
            snp.add(st, g, ring, [c], [1], sc.MAX_COUNT, sc.MAX_ROWS)
            same_accumulation(k, st, g)
        assert k.photo_spatial_status()["state"] == "accumulating"
        it, de, bar = snp.estimate(st, g), snp.estimate(st, g, dense=True), sc.bar(name)
        out = k.photo_spatial_estimate(install=False)
        s = k.photo_spatial_stage()
        err = {key: sc.rel(s[key], de[key]) for key in ("x", "alpha", "coarse")}
        print(name, out, "restated iterations", it["ls"]["iterations"], it["gp"]["iterations"], "error against the dense solutions", err,
              "bars", bar)
        assert out["converged"] and out["n"] == it["n"] == sc.RECORDED[name]["n"]
        assert np.array_equal(s["var_of_cell"], it["var_of_cell"])
        assert np.array_equal(s["L"], it["L"])                                   # integers: exactly
        assert s["c"].tobytes() == it["c"].tobytes()                             # ascending row order: the same additions
        for key in ("x", "alpha", "coarse"):
            assert err[key] <= bar[key], (key, err[key], bar[key])
        assert np.array_equal(s["ps"], snp.upsample(g, s["coarse"]))             # the device's own coarse map, upsampled
        assert abs(out["ls_iterations"] - it["ls"]["iterations"]) <= 2 and abs(out["gp_iterations"] - it["gp"]["iterations"]) <= 2
        assert out["ls_residual"] < snp.TOL and out["gp_residual"] < snp.TOL
        out2 = k.photo_spatial_estimate(install=False)                           # the same rows again: the same bytes
        s2 = k.photo_spatial_stage()
        assert out2 == out
        for key in s:
            assert s2[key].tobytes() == s[key].tobytes(), key
        st_after = k.photo_spatial_status()
        assert st_after["state"] == "accumulating" and st_after["rows"] == len(st["b"])
    finally:
        k.close()


def test_install_corrects_with_the_map_and_stops_accumulation(eng):
    q = sc.EST["remainder"]                                                      # 70 x 50: the clamp is in the installed map
    g, _, calls = sc.points("remainder")
    rng = np.random.default_rng(5)
    im = rng.integers(0, 256, (q["size"][1], q["size"][0]), dtype=np.uint8)
    k, ring = make(eng, q["size"], q["div"])
    try:
        k.push_image(im)
        for c in calls:
            k.photo_spatial_add(*c, (1,))
        rows = k.photo_spatial_rows()
        out = k.photo_spatial_estimate(install=True)
        assert out["converged"] and k.photo_spatial_status()["state"] == "estimated"
        ps = k.photo_spatial_stage()["ps"]
        assert np.abs(ps).max() > 1e-3                                           # (a map that changes pixels)
        a, b = ring[-1]
        k.photo_correct(1)
        ref = pnp.correct(im, float(a), float(b), ps)
        assert not np.array_equal(ref, pnp.correct(im, float(a), float(b)))
        assert np.array_equal(k.level(1, 0)[0], ref)                             # bit for bit
        k.photo_spatial_add(*calls[0], (1,))                                     # accumulation has stopped: nothing moves
        again = k.photo_spatial_rows()
        for key in rows:
            assert again[key].tobytes() == rows[key].tobytes(), key
        k.photo_spatial_reset()                                                  # back to accumulating, empty; the PS plane stays
        assert k.photo_spatial_status() == dict(rows=0, covered=0, cells=12, ready=False, dropped=0, state="accumulating")
        assert not k.photo_spatial_rows()["counts"].any()
        with pytest.raises(tracker.XkError) as e:
            k.photo_spatial_stage()
        assert e.value.status == XK_EINVAL
        k.photo_correct(1)
        assert np.array_equal(k.level(1, 0)[0], ref)
        k.photo_set_spatial(None)
        k.photo_correct(1)
        assert np.array_equal(k.level(1, 0)[0], pnp.correct(im, float(a), float(b)))
    finally:
        k.close()


def test_cap_crossing_same_cell_overflow(eng):
    g, calls = sc.cap_calls()
    k, ring = make(eng, sc.CAP["size"], sc.CAP["div"], max_count=sc.CAP["max_count"])
    try:
        st = snp.new_state(g)
        for c in calls:                                                          # the cap inside a chunk and on a chunk's boundary
            k.photo_spatial_add(*c, (1,))
            snp.add(st, g, ring, [c], [1], sc.CAP["max_count"], sc.MAX_ROWS)
            same_accumulation(k, st, g)
        assert len(st["b"]) > 82 and k.photo_spatial_rows(0, 82)["sid_hist"].tolist() == [sc.CAP["A"]] * 41 + [sc.CAP["B"]] * 41
    finally:
        k.close()
    g, call = sc.same_cell_call()
    k, ring = make(eng, (96, 64), 16)
    try:
        k.photo_spatial_add(*call, (1,))                                         # sh == sc throughout: no row, nothing covered
        assert k.photo_spatial_status() == dict(rows=0, covered=0, cells=24, ready=False, dropped=0, state="accumulating")
        with pytest.raises(tracker.XkError) as e:
            k.photo_spatial_estimate()
        assert e.value.status == XK_EINVAL
    finally:
        k.close()
    g, _, calls = sc.points("basic")
    k, ring = make(eng, (96, 64), 16, max_rows=100)
    try:
        st = snp.new_state(g)
        for c in calls:                                                          # the row list fills up in the first call
            k.photo_spatial_add(*c, (1,))
            snp.add(st, g, ring, [c], [1], sc.MAX_COUNT, 100)
            same_accumulation(k, st, g)
        assert st["dropped"] > 0 and k.photo_spatial_status()["dropped"] == st["dropped"]
        with pytest.raises(tracker.XkError) as e:
            k.photo_spatial_rows(0, 101)
        assert e.value.status == XK_EINVAL
        it = snp.estimate(st, g)
        out = k.photo_spatial_estimate(install=False)
        s = k.photo_spatial_stage()
        assert out["converged"] and np.array_equal(s["L"], it["L"]) and s["c"].tobytes() == it["c"].tobytes()
    finally:
        k.close()


def test_frame_back_on_a_ring_of_distinct_pairs(eng):
    g, groups, fb = sc.frame_back_groups()
    k, ring = make(eng, (96, 64), 16, pairs=sc.RING_PAIRS)
    try:
        assert len(ring) == 4 and len({tuple(r) for r in ring}) == 4
        st = snp.new_state(g)
        k.photo_spatial_add([v[0] for v in groups], [v[1] for v in groups], [v[2] for v in groups], [v[3] for v in groups], fb)
        snp.add(st, g, ring, groups, fb, sc.MAX_COUNT, sc.MAX_ROWS)
        same_accumulation(k, st, g)
        one = snp.new_state(g)                                                   # (the groups' rows differ with frame_back)
        snp.add(one, g, ring, groups, (1, 1, 1), sc.MAX_COUNT, sc.MAX_ROWS)
        assert snp.rows(one)[2].tobytes() != snp.rows(st)[2].tobytes()
        for bad in ((4, 1, 1), (1, 0, 1)):
            with pytest.raises(tracker.XkError) as e:
                k.photo_spatial_add([v[0] for v in groups], [v[1] for v in groups], [v[2] for v in groups], [v[3] for v in groups], bad)
            assert e.value.status == XK_EINVAL
        same_accumulation(k, st, g)                                              # a refused call adds nothing
    finally:
        k.close()


# ---- the per-frame call ----
def test_calibrate_accumulates_and_changes_no_output(eng):
    q = pc.FRAME
    im1, im2 = pc.frame_images()
    xy, val = pc.frame_features()
    div = 4
    g = snp.grid(q["size"][0], q["size"][1], div)
    res = []
    for spatial in (False, True):
        k = tracker.Klt(eng, 64, q["size"][0], q["size"][1], q["win"], q["max_level"], max_iter=q["max_iter"], eps=q["eps"],
                        min_eig_thr=q["min_eig_thr"])
        try:
            k.photo_setup(q["kernel_size"], q["eps_gap"], q["eps_base"], 64)
            if spatial:
                k.photo_spatial_setup(div, sc.THR, sc.MAX_COUNT, sc.MAX_ROWS)
            k.push_image(im1)
            k.push_image(im2)
            tr = k.track(xy)                                                     # (the working planes equal the raw ones still)
            r0 = k.photo_calibrate(xy[:3], val[:3], q["n_hyp"], q["ransac_seed"])
            if spatial:
                assert k.photo_spatial_status()["rows"] == 0                     # no estimate, no rows
            r = k.photo_calibrate(xy, val, q["n_hyp"], q["ransac_seed"])
            res.append((r0, r, k.photo_params(), [k.level(1, l) for l in range(k.levels() + 1)]))
            if not spatial:
                continue
            assert r["estimated"] and np.array_equal(tr["keep_idx"], r["keep_idx"])
            keep = r["keep_idx"]
            lists = (np.trunc(xy[keep]).astype(np.int32), np.trunc(tr["kept_cur"]).astype(np.int32), val[keep], r["intensity"])
            st = snp.new_state(g)
            snp.add(st, g, k.photo_params(), [lists], [1], sc.MAX_COUNT, sc.MAX_ROWS)
            print("calibrate: kept", len(keep), "rows", len(st["b"]), "covered", int(st["coverage"].sum()))
            assert len(st["b"]) >= 8                                             # (the shift moves features across cells of 4 pixels)
            same_accumulation(k, st, g)
            rows = k.photo_spatial_rows()
            k.photo_spatial_reset()                                              # the same lists through the explicit entry
            k.photo_spatial_add(*lists, (1,))
            again = k.photo_spatial_rows()
            for key in rows:
                assert again[key].tobytes() == rows[key].tobytes(), key
        finally:
            k.close()
    (a0, a, pa, la), (b0, b, pb, lb) = res
    for x, y in ((a0, b0), (a, b)):                                              # every existing output, byte for byte
        for key in x:
            assert np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes(), key
    assert pa.tobytes() == pb.tobytes()
    for x, y in zip(la, lb):
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes()


# ---- an estimate that does not converge (lab build: the iteration cap) ----
def test_no_convergence_installs_nothing_and_accumulation_goes_on():
    g, _, calls = sc.points("basic")
    lab = engine.LabEngine(4, 0, 4)
    try:
        rng = np.random.default_rng(6)
        im = rng.integers(0, 256, (64, 96), dtype=np.uint8)
        k, ring = make(lab, (96, 64), 16)
        try:
            k.push_image(im)
            k.photo_spatial_add(*calls[0], (1,))
            lab.set_option("photo_spatial_cap", 1)
            out = k.photo_spatial_estimate(install=True)
            print("capped", out)
            assert not out["converged"] and out["ls_iterations"] == 1 and out["gp_iterations"] == 0 and out["ls_residual"] > 1e-6
            st = k.photo_spatial_status()
            assert st["state"] == "failed-and-accumulating"
            a, b = ring[-1]
            k.photo_correct(1)
            assert np.array_equal(k.level(1, 0)[0], pnp.correct(im, float(a), float(b)))      # the PS plane is still zero
            k.photo_spatial_add(*calls[1], (1,))                                 # accumulation goes on
            assert k.photo_spatial_status()["rows"] > st["rows"]
            lab.set_option("photo_spatial_cap", 0)
            out = k.photo_spatial_estimate(install=True)
            assert out["converged"] and k.photo_spatial_status()["state"] == "estimated"
            k.photo_correct(1)
            assert np.array_equal(k.level(1, 0)[0], pnp.correct(im, float(a), float(b), k.photo_spatial_stage()["ps"]))
        finally:
            k.close()
    finally:
        lab.close()


# ---- arguments and lifetime ----
def test_arguments_and_lifetime(eng):
    L = eng.L
    k = tracker.Klt(eng, 512, 128, 80, (5, 5), 1)
    try:
        p = k.p
        i4, d = np.zeros(4096, np.int32), np.zeros(4096)
        ip, dp = i4.ctypes.data_as(c_ip), d.ctypes.data_as(c_dp)
        fbuf, ub = np.zeros(128 * 80, np.float32).ctypes.data_as(c_fp), np.zeros(4096, np.uint8).ctypes.data_as(c_ub)
        one, n1 = np.ones(1, np.int32).ctypes.data_as(c_ip), C.c_int(0)
        o = tracker.SpatialOutcome()

        def setup(div=16, thr=0.9, max_count=500, max_rows=64, l=5.0, sf=0.01, sn=0.01):
            return L.xk_trk_photo_spatial_setup(p, C.c_int(div), C.c_double(thr), C.c_int(max_count), C.c_int(max_rows), C.c_double(l),
                                                C.c_double(sf), C.c_double(sn))

        entries = [
            lambda: L.xk_trk_photo_spatial_add(p, 1, ip, ip, ip, dp, dp, one),
            lambda: L.xk_trk_photo_spatial_status(p, None, None, None, None, None, C.byref(n1)),
            lambda: L.xk_trk_photo_spatial_rows(p, 0, 0, ip, ip, dp, ip, ub),
            lambda: L.xk_trk_photo_spatial_reset(p),
        ]
        est = lambda: L.xk_trk_photo_spatial_estimate(p, 0, C.byref(o))
        stage = lambda: L.xk_trk_photo_spatial_stage(p, ip, None, dp, dp, dp, fbuf, fbuf)
        assert setup() == XK_EINVAL                                              # before xk_trk_photo_setup
        k.photo_setup(30, 0.0, 0.0, 8)
        for call in entries + [est, stage]:                                      # every entry before the spatial setup
            assert call() == XK_EINVAL
        for kw in (dict(div=1), dict(div=257), dict(div=128), dict(thr=float("nan")), dict(thr=float("inf")), dict(max_count=0),
                   dict(max_rows=0), dict(l=0.0), dict(sf=-1.0), dict(sn=0.0), dict(l=float("nan"))):
            assert setup(**kw) == XK_EINVAL, kw                                  # (div 128 on 128 x 80: one cell column, no row: 0 cells)
        assert setup() == 0
        put_ring(k, sc.RING_PAIRS[:1])
        for call in entries:
            assert call() == 0
        assert est() == XK_EINVAL and stage() == XK_EINVAL                       # no row yet, no estimate yet
        assert L.xk_trk_photo_spatial_estimate(p, 0, None) == XK_EINVAL
        off = np.array([0, 513], np.int32).ctypes.data_as(c_ip)
        assert L.xk_trk_photo_spatial_add(p, 1, off, ip, ip, dp, dp, one) == XK_ECAPACITY      # a group above max_matches
        assert L.xk_trk_photo_spatial_add(p, 0, ip, ip, ip, dp, dp, one) == XK_EINVAL
        assert L.xk_trk_photo_spatial_add(p, 15, ip, ip, ip, dp, dp, one) == XK_EINVAL
        two = np.full(1, 2, np.int32).ctypes.data_as(c_ip)
        assert L.xk_trk_photo_spatial_add(p, 1, ip, ip, ip, dp, dp, two) == XK_EINVAL          # the ring holds two pairs
        assert L.xk_trk_photo_spatial_add(p, 1, ip, ip, ip, dp, dp, ip) == XK_EINVAL           # frame_back 0
        assert L.xk_trk_photo_spatial_add(p, 1, ip, None, ip, dp, dp, one) == 0                # an empty group needs no lists
        assert L.xk_trk_photo_spatial_rows(p, 0, 1, ip, ip, dp, None, None) == XK_EINVAL and L.xk_trk_photo_spatial_rows(p, -1, 0, ip, ip, dp, None, None) == XK_EINVAL
        g, _, calls = sc.points("blocks160")
        k.photo_spatial_setup(8, sc.THR, sc.MAX_COUNT, sc.MAX_ROWS)
        k.photo_spatial_add(*calls[0], (1,))
        rows = k.photo_spatial_rows()
        assert len(rows["b"]) > 0 and setup(div=1) == XK_EINVAL                  # a failed setup ...
        assert k.photo_spatial_rows()["b"].tobytes() == rows["b"].tobytes()      # ... leaves the earlier one, rows and all
        k.photo_reset()                                                          # the ring back to one pair: no frame to look back to
        assert L.xk_trk_photo_spatial_add(p, 1, ip, ip, ip, dp, dp, one) == XK_EINVAL
        # more covered cells than n_max: 64 x 40 cells of 2 pixels, 2400 of them covered by 1200 points in three groups
        put_ring(k, sc.RING_PAIRS[:1])
        k.photo_spatial_setup(2, sc.THR, sc.MAX_COUNT, sc.MAX_ROWS)
        j = np.arange(1200)
        ph = np.stack([(2 * j % 64) * 2, (2 * j // 64) * 2], axis=1).astype(np.int32)
        pcur = ph + np.array([2, 0], np.int32)
        grp = lambda v: [v[:400], v[400:800], v[800:]]
        k.photo_spatial_add(grp(ph), grp(pcur), grp(np.zeros(1200)), grp(np.zeros(1200)), (1, 1, 1))
        assert k.photo_spatial_status()["covered"] == 2400
        with pytest.raises(tracker.XkError) as e:
            k.photo_spatial_estimate()
        assert e.value.status == XK_ECAPACITY and k.photo_spatial_status()["state"] == "accumulating"
        k.photo_setup(30, 0.0, 0.0, 8)                                           # a new photo setup drops the spatial one
        for call in entries + [est, stage]:
            assert call() == XK_EINVAL
        assert setup() == 0
        k.setup(128, 80, (5, 5), 1)                                              # xk_trk_klt_setup drops both
        for call in entries + [est, stage]:
            assert call() == XK_EINVAL
        assert setup() == XK_EINVAL
    finally:
        k.close()
