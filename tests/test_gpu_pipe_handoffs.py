"""The XCD-local hand-offs of the single launch are per FIRST-LEVEL GROUP (csrc/xk_caqr_pipe.hip.h: XP_TQ_CNT [4][8][2], XP_MB_CNT
[8][2]): a tile arrives on the counter of the group that merges its strip and waits for that group's workgroups only; a first-level
group waits for its own tiles only.  It touches no arithmetic, so what can go wrong is an ordering: a group that starts on rows the
other group's count used to cover, a strip read before it is back.  Checked on small systems on the 152-tile, two-group geometry in
which the two groups of an XCD are as unlike each other as the row plan allows -- the accepted rows are dealt TR = ceil(R / 152) to a
tile, tile 19 x + s is slot s of XCD x, slots 0..9 are group A, 10..18 group B:

  few          12 full tracks: a row or two per tile, the last XCDs (or their group B) hold no row at all
  a_plus_one   a track count at which the last XCD that holds rows has group A full and ONE tile of group B
  half         150 tracks, about half of them rejected by the gate

each against the C oracle (tolerances of tests/test_gpu_pipe_split.py), the inlier masks identical, the -DXK_SYNC_STRICT=1 twin
bit for bit (the pattern of tests/test_gpu_soak.py: _strict_twin), ten updates on one handle bit-identical from the second on.
N = 6: 37 columns, two full panels + one of 5; N = 8: 49 columns, the last panel is the residual column alone; N = 11: 67 columns.
One case on the 184-tile geometry and one on BASELINE config 2's shape with fewer tracks (M > 0: split compression on the narrow
geometry; "slam_split" 0: the whole stack on the wide one, two lanes per column) hold NG = 1 and the other tile layout."""
import os

import numpy as np
import pytest

from helpers import rel
from x_multi_agent_amd import synth

pytestmark = pytest.mark.gpu

NT, NTG, TILES = 19, 10, 152           # XkPipeNarrow2: tiles per XCD, of them in group A, tiles of a launch

#        name -> (tracks at N = 6, 8, 11, keyword arguments of synth.make_scenario, seed base)
ROWS = {
    "few": ({6: 12, 8: 12, 11: 12}, dict(outlier_frac=0.0, err_scale=0.3), 5100),
    "a_plus_one": ({6: 16, 8: 49, 11: 54}, dict(outlier_frac=0.0, err_scale=0.3), 5200),
    "half": ({6: 150, 8: 150, 11: 150}, dict(outlier_frac=0.5), 5300),
}
_CACHE = {}


def _case(oracle_c, N, rows):
    """(scenario, oracle result, tiles that hold rows): computed once, shared, never modified."""
    if (N, rows) not in _CACHE:
        ks, kw, seed = ROWS[rows]
        sc = synth.make_scenario(N, ks[N], 0, seed=seed + N, **kw)
        ref = oracle_c.visual_update(sc)
        R = int(((2 * np.diff(sc["trk_off"]) - 3) * ref["inlier"].astype(bool)).sum())      # rows that pass the gates
        TR = max(1, -(-R // TILES))
        _CACHE[(N, rows)] = (sc, ref, -(-R // TR))
    return _CACHE[(N, rows)]


def _strict(xk):
    if not os.path.exists(xk.STRICT_LIB_PATH):
        from x_multi_agent_amd import build
        build.build_strict()
    return xk.STRICT_LIB_PATH


def _updates(eng, sc, count):
    """`count` updates of the same staged inputs on one handle: [(posterior, correction, inlier, inlier_slam)]"""
    out = []
    for _ in range(count):
        eng.stage(sc)
        r = eng.visual_update_staged(sc["sigma_img"])
        out.append((eng.download_P(), r["correction"].copy(), r["inlier"].copy(), r["inlier_slam"].copy()))
        st = eng.caqr_status()
        assert st["schedule"] == 2 and st["giveups"] == 0, st
    return out


def _against_oracle(got, ref, what):
    P, corr, inl, inl_slam = got
    assert np.array_equal(inl, ref["inlier"]) and np.array_equal(inl_slam, ref["inlier_slam"]), what
    assert rel(P, ref["P"]) <= 1e-8 and rel(corr, ref["correction"]) <= 1e-6, (what, rel(P, ref["P"]), rel(corr, ref["correction"]))


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (what, rel(a[0], b[0]))


@pytest.mark.parametrize("rows", sorted(ROWS))
@pytest.mark.parametrize("N", [6, 8, 11])
def test_two_unlike_groups(xk, oracle_c, N, rows):
    sc, ref, filled = _case(oracle_c, N, rows)
    K = len(sc["trk_off"]) - 1
    if rows == "few":
        assert filled <= 7 * NT + NTG, filled                     # the last XCD's group B (at least) holds no row
    if rows == "a_plus_one":
        assert filled % NT == NTG + 1, filled                      # ... group A full, one tile of group B
    if rows == "half":
        assert 0.35 * K <= int(ref["inlier"].sum()) <= 0.65 * K, int(ref["inlier"].sum())
    # the two-group geometry forced, the update inside the launch and behind it
    lab = xk.LabEngine(N, 0, K)
    lab.set_option("pipe_split", 3)
    for kal in (1, 0):
        lab.set_option("pipe_kalman", kal)
        _against_oracle(_updates(lab, sc, 1)[0], ref, (N, rows, kal))
        lab.stage(sc)
        assert lab.bench_staged(sc["sigma_img"], 0, 1)["n_leaf"] == TILES
    lab.close()
    # the release library: the first update of a handle takes 184 tiles, the following ones 152
    eng = xk.Engine(N, 0, K)
    got = _updates(eng, sc, 10)
    eng.stage(sc)
    assert eng.bench_staged(sc["sigma_img"], 0, 1)["n_leaf"] == TILES
    eng.close()
    for g in got:
        _against_oracle(g, ref, (N, rows))
    for i in range(2, 10):
        _same(got[i], got[1], (N, rows, i))
    twin = xk.Engine(N, 0, K, lib_path=_strict(xk))
    tw = _updates(twin, sc, 3)
    twin.close()
    _same(tw[0], got[0], (N, rows, "strict, 184 tiles"))
    _same(tw[2], got[2], (N, rows, "strict, 152 tiles"))


def test_one_group_per_xcd(xk, oracle_c):
    """The 184-tile geometry (NG = 1: group 0's counters are the XCD's) on the shape with the most rejected tracks."""
    sc, ref, _ = _case(oracle_c, 11, "half")
    K = len(sc["trk_off"]) - 1
    lab = xk.LabEngine(11, 0, K)
    lab.set_option("pipe_split", 0)
    got = _updates(lab, sc, 10)
    lab.stage(sc)
    assert lab.bench_staged(sc["sigma_img"], 0, 1)["n_leaf"] == 184
    lab.close()
    for g in got:
        _against_oracle(g, ref, "184 tiles")
    for i in range(1, 10):
        _same(got[i], got[0], i)


@pytest.mark.parametrize("split", [1, 0])
def test_config_2_shape_with_fewer_tracks(xk, oracle_c, split):
    """N = 30, M = 50 as BASELINE config 2, 60 tracks.  split = 1: the tracks' rows in the 181 pose columns + the residual (narrow
    geometries, res_col > 0); 0: the whole stack in 331 columns on the wide geometry -- two lanes per column, one group per XCD."""
    N, _, M = synth.CONFIGS[2]
    K = 60
    if "cfg2" not in _CACHE:
        sc = synth.make_scenario(N, K, M, seed=5400)
        _CACHE["cfg2"] = (sc, oracle_c.visual_update(sc))
    sc, ref = _CACHE["cfg2"]
    out = []
    for path in (None, _strict(xk)):
        eng = xk.Engine(N, M, K, lib_path=path)
        eng.set_option("slam_split", split)
        out.append(_updates(eng, sc, 10 if path is None else 3))
        if path is None:
            eng.stage(sc)
            leaves = eng.bench_staged(sc["sigma_img"], 0, 1)["n_leaf"]
            assert leaves == TILES, leaves                                # narrow-2 (split) / wide (whole stack): 152 tiles either way
        eng.close()
    got, tw = out
    for g in got:
        _against_oracle(g, ref, split)
        assert np.array_equal(g[3], got[0][3])
    for i in range(2, 10):
        _same(got[i], got[1], (split, i))
    _same(tw[0], got[0], (split, "strict, first update"))
    _same(tw[2], got[2], (split, "strict, third update"))
