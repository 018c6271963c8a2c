"""The NumPy restatement of the spatial photometric map (tests/photo_spatial_np.py) and its cases (tests/photo_spatial_cases.py),
without a GPU: the accumulation against a plain Python loop, the least-squares solution against the dense solution in the same
gauge, the GP weights against numpy.linalg.solve, the recovery of a known smooth map up to the gauge, and the figures recorded in
the cases file."""
import numpy as np
import pytest

import photo_spatial_cases as sc
import photo_spatial_np as snp

IDENT = [(1.0, 0.0), (1.0, 0.0)]


def plain_loop(g, ring, calls, max_count, max_rows):
    """The statement once more, with Python ints and floats and nothing else."""
    count, cover, out, dropped = [0] * g["cells"], [0] * g["cells"], [], 0
    for ph, pc, oh, oc, fb in calls:
        a1, b1 = ring[len(ring) - 1 - fb]
        a2, b2 = ring[-1]
        e = (a2 - b2) / (a1 - b1)
        b_hc = (b2 - b1) / (a1 - b1)
        a_hc = e + b_hc
        for j in range(len(ph)):
            ids = []
            for x, y in (ph[j], pc[j]):
                x, y = int(x), int(y)
                inside = 0 <= x < g["w"] and 0 <= y < g["h"] and x // g["div"] < g["cw"] and y // g["div"] < g["ch"]
                ids.append((y // g["div"]) * g["cw"] + x // g["div"] if inside else None)
            sh, sc_ = ids
            if sh is None or sc_ is None or sh == sc_ or count[sh] > max_count:
                continue
            cover[sh] = cover[sc_] = 1
            if len(out) < max_rows:
                out.append((sh, sc_, float(oc[j]) * (a_hc - b_hc) - float(oh[j]) + b_hc))
            else:
                dropped += 1
            count[sc_] += 1
            count[sh] += 1
    return count, cover, out, dropped


def same_as_loop(st, ref):
    count, cover, out, dropped = ref
    sh, sc_, b = snp.rows(st)
    assert list(st["count"]) == count and list(st["coverage"]) == cover and st["dropped"] == dropped
    assert [(int(a), int(c)) for a, c in zip(sh, sc_)] == [(r[0], r[1]) for r in out]
    assert b.tobytes() == np.array([r[2] for r in out], np.float64).tobytes()


@pytest.mark.parametrize("name", list(sc.EST))
def test_accumulation_matches_a_plain_loop(name):
    g, _, calls = sc.points(name)
    ring = [(1.0, 0.0), (1.04, 0.01), (0.97, -0.02)]
    st = snp.new_state(g)
    for i, c in enumerate(calls):
        snp.add(st, g, ring, [c], [1 + i % 2], sc.MAX_COUNT, sc.MAX_ROWS)
    same_as_loop(st, plain_loop(g, ring, [c + (1 + i % 2,) for i, c in enumerate(calls)], sc.MAX_COUNT, sc.MAX_ROWS))
    if name == "remainder":                                                      # points of the remainder column and row exist, and are skipped
        ph = np.concatenate([c[0] for c in calls])
        assert ((ph[:, 0] >= 64) & (ph[:, 0] < 70)).any() and ((ph[:, 1] >= 48) & (ph[:, 1] < 50)).any()
        assert snp.cell(g, 65, 10) == -1 and snp.cell(g, 10, 49) == -1 and snp.cell(g, 63, 47) == 11


def test_cap_same_cell_overflow_and_frame_back():
    g, calls = sc.cap_calls()
    st = snp.new_state(g)
    snp.add(st, g, IDENT, [calls[0]], [1], sc.CAP["max_count"], sc.MAX_ROWS)
    sh = snp.rows(st)[0]
    # cell A takes points 0 ... 40 (the cap is passed inside a chunk), cell B points 87 ... 127 (with the last point of a chunk)
    assert len(sh) == 82 and (sh[:41] == sc.CAP["A"]).all() and (sh[41:] == sc.CAP["B"]).all()
    assert st["count"][sc.CAP["A"]] == 41 and st["count"][sc.CAP["B"]] == 41
    snp.add(st, g, IDENT, [calls[1]], [1], sc.CAP["max_count"], sc.MAX_ROWS)
    same_as_loop(st, plain_loop(g, IDENT, [c + (1,) for c in calls], sc.CAP["max_count"], sc.MAX_ROWS))
    assert not np.isin(snp.rows(st)[0][82:], [sc.CAP["A"], sc.CAP["B"]]).any() and len(st["b"]) > 82
    # the same cell: no row, nothing covered
    g, call = sc.same_cell_call()
    st = snp.new_state(g)
    snp.add(st, g, IDENT, [call], [1], sc.MAX_COUNT, sc.MAX_ROWS)
    assert snp.status(st, g, sc.THR) == dict(rows=0, covered=0, cells=24, dropped=0, ready=False)
    with pytest.raises(ValueError):
        snp.estimate(st, g)
    # overflow: the rows stop at max_rows, counts and coverage go on
    g, _, calls = sc.points("basic")
    full, cut = snp.new_state(g), snp.new_state(g)
    for c in calls:
        snp.add(full, g, IDENT, [c], [1], sc.MAX_COUNT, sc.MAX_ROWS)
        snp.add(cut, g, IDENT, [c], [1], sc.MAX_COUNT, 100)
    assert len(cut["b"]) == 100 and cut["dropped"] == len(full["b"]) - 100 > 0
    assert np.array_equal(cut["count"], full["count"]) and np.array_equal(cut["coverage"], full["coverage"])
    assert snp.rows(cut)[2].tobytes() == snp.rows(full)[2][:100].tobytes()
    # frame_back: each group against its own ring entry
    g, groups, fb = sc.frame_back_groups()
    ring = [(1.0, 0.0)] + list(sc.RING_PAIRS)
    st = snp.new_state(g)
    snp.add(st, g, ring, groups, fb, sc.MAX_COUNT, sc.MAX_ROWS)
    same_as_loop(st, plain_loop(g, ring, [grp + (f,) for grp, f in zip(groups, fb)], sc.MAX_COUNT, sc.MAX_ROWS))
    with pytest.raises(ValueError):
        snp.add(st, g, ring, groups[:1], [4], sc.MAX_COUNT, sc.MAX_ROWS)
    # ready is strict, against the float threshold
    g2 = snp.grid(160, 16, 16)                                                   # 10 cells
    st = snp.new_state(g2)
    st["coverage"][:5] = 1
    assert not snp.status(st, g2, 0.5)["ready"]                                  # 5 / 10 > 0.5 is false: strict
    st["coverage"][:9] = 1
    assert snp.status(st, g2, 0.9)["ready"] and float(np.float32(0.9)) < 0.9     # 9 / 10 > (double)0.9f = 0.899999976...
    assert not snp.status(st, g2, 0.95)["ready"]


@pytest.mark.parametrize("name", list(sc.EST))
def test_solves_against_the_dense_solutions_and_the_recorded_figures(name):
    g, m, st, it, de = sc.restated(name)
    got, rec, bar = sc.measure(name), sc.RECORDED[name], sc.bar(name)
    print(name, got)
    assert it["converged"] and (got["n"], got["rows"]) == (rec["n"], rec["rows"])
    assert abs(got["ls_it"] - rec["ls_it"]) <= 2 and abs(got["gp_it"] - rec["gp_it"]) <= 2
    assert got["cond_l"] <= rec["cond_l"] and got["cond_k"] <= rec["cond_k"]
    for key in ("x", "alpha", "coarse"):
        assert got["err"][key] <= bar[key], (key, got["err"][key], bar[key])
    # the normal equations are those of the dense A, exactly (integers) and to rounding (c)
    sh, sc_, b = snp.rows(st)
    A = snp.design(sh, sc_, it["var_of_cell"], it["n"])
    assert np.array_equal(A.T @ A, it["L"]) and np.allclose(A.T @ b, it["c"], rtol=0, atol=1e-13 * np.abs(b).sum())
    assert np.array_equal(it["var_of_cell"][it["cell_of_var"]], np.arange(it["n"]))
    # the gauge: sum deg_i x_i = 0 on every connected component, for the iteration and the dense solution alike
    comp = components(it["L"])
    for x in (it["x"], de["x"]):
        for cmp in comp:
            assert abs((it["deg"][cmp] * x[cmp]).sum()) <= 1e-12 * (it["deg"][cmp] * np.abs(x[cmp])).sum()
    # recovery of the map the rows were generated from, up to one constant per component
    d = de["x"] - m[it["cell_of_var"]]
    for cmp in comp:
        assert np.ptp(d[cmp]) < 1e-13
    assert len(comp) == (2 if name == "two_components" else 1)
    assert np.array_equal(it["ps"], snp.upsample(g, it["coarse"])) and it["ps"].shape == (g["h"], g["w"])
    if name == "remainder":                                                      # the clamp: the remainder takes the last cell's value
        assert (it["ps"][:, 64:] == it["ps"][:, 63:64]).all() and (it["ps"][48:, :] == it["ps"][47:48, :]).all()
    if name == "cells48":
        assert [c for c in range(48) if it["var_of_cell"][c] < 0] == list(sc.EST[name]["exclude"])


def components(L):
    n, seen, out = len(L), set(), []
    for s in range(n):
        if s in seen:
            continue
        todo, cmp = [s], []
        seen.add(s)
        while todo:
            v = todo.pop()
            cmp.append(v)
            for u in np.flatnonzero(L[v] != 0):
                if int(u) not in seen:
                    seen.add(int(u))
                    todo.append(int(u))
        out.append(np.array(sorted(cmp)))
    return out


def test_a_cap_of_one_iteration_does_not_converge():
    g, _, st, _, _ = sc.restated("basic")
    r = snp.estimate(st, g, cap=1)
    assert not r["converged"] and r["ls"]["iterations"] == 1 and r["alpha"] is None and "ps" not in r
