"""The inputs of the searched device CI round keep the properties the GPU tests rest on (CPU only): which tracks the gates reject,
that the search is short and interior, and how far two CPU routes to M_i = H_i P_i^-1 H_i^T are apart."""
import numpy as np
import pytest

import ci_weights_ref as cw
from ci_round_cases import SHAPE_IDS, SHAPES, fleet_case, searched
from helpers import rel


@pytest.mark.parametrize("world,N,corrupt", SHAPES, ids=SHAPE_IDS)
def test_shapes_of_the_searched_round(world, N, corrupt):
    case = fleet_case(world, N, corrupt)
    a, b = searched(world, N, corrupt)
    assert a["rejected"] == b["rejected"] == (set() if corrupt is None else {corrupt})
    assert a["n_fused"] == case["n_tracks"] - len(a["rejected"]) >= 2
    worst_w = worst_ld = 0.0
    for j, ta in a["tracks"].items():
        tb = b["tracks"][j]
        assert len(ta["w"]) == world and ta["M"].shape == (world, 3 * (world - 1), 3 * (world - 1))
        assert ta["iters"] <= 12 and tb["iters"] <= 12, (j, ta["iters"], tb["iters"])
        assert ta["w"].min() > 1e-3 and tb["w"].min() > 1e-3, (j, ta["w"], tb["w"])
        assert abs(ta["w"].sum() - 1.0) <= 1e-15
        ld = abs(cw.logdet(ta["M"], ta["w"]) - cw.logdet(ta["M"], tb["w"]))
        worst_w, worst_ld = max(worst_w, float(np.abs(ta["w"] - tb["w"]).max())), max(worst_ld, ld)
        assert ld <= 1e-8, (j, ld)
    dP = rel(a["P"], b["P"])
    print(f"world {world}, n = {15 + 6 * N}: rejected {sorted(a['rejected'])}, steps "
          f"{[t['iters'] for t in a['tracks'].values()]}, min w {min(t['w'].min() for t in a['tracks'].values()):.3f}; two CPU routes: "
          f"|dw| {worst_w:.1e}, |d log det| {worst_ld:.1e}, posterior rel {dP:.1e}")
    # the searched posterior is far from the fixed-weight one: a round that ignored the search cannot pass the GPU tests
    from ci_round_cases import yardstick
    fixed = yardstick(case, weights=[[1.0 - (world - 1) * 0.04] + [0.04] * (world - 1)] * case["n_tracks"])
    assert fixed["rejected"] == a["rejected"]
    assert rel(a["P"], fixed["P"]) > 0.1
