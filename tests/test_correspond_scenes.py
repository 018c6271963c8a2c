"""The scenes of tests/correspond_np.py satisfy, by the restatements alone, the conditions that let
tests/test_gpu_find_correspondences.py compare bit for bit -- conditions on inputs, not measurements -- and the
reference's duplicate removal, as restated in oracle/ref_pr.py, is not a clean de-duplication on them."""
import numpy as np
import pytest

import correspond_np as cnp
import essential_np as enp

from oracle import ref_pr


def _pairs(case, exp):
    """What point pair every candidate is: (landmark of the received pixel, landmark of the current pixel)."""
    return [(int(case["land"][q]), int(t)) for q, t in exp["candidates"]]


@pytest.mark.parametrize("name", cnp.RANSAC_SCENES)
def test_ransac_conditions(name):
    case, exp = cnp.scene(name)
    ref, n = exp["ref"], exp["n_candidates"]
    print(name, "candidates", n, "inliers", ref["n_inliers"], "margin", ref["margin"])
    assert exp["status"] == 0 and ref["margin"] >= 1e-6
    pairs = _pairs(case, exp)
    distinct = lambda h: len({pairs[i] for i in enp.sample(case["seed"], h, n)}) == 5
    assert distinct(ref["winner"])
    for h in range(case["n_hyp"]):
        if not distinct(h) and len(ref["counts"][h]):
            assert 2 * int(ref["counts"][h].max()) <= ref["n_inliers"], h
    planted = np.array([int(q) not in case["wrong"] for q, _ in exp["candidates"]])
    assert np.array_equal(ref["mask"].astype(bool), planted)


def test_scene_shapes():
    case, exp = cnp.scene("base")
    assert exp["n_candidates"] == 60 and exp["n_inliers"] == 40 and len(exp["remove_ids"]) == 0 and len(exp["good"]) == 40
    assert sorted(set(exp["classified"][:, 0].tolist())) == [0, 1, 2, 3]          # all four kinds
    case, exp = cnp.scene("boundaries")
    assert exp["n_candidates"] == 270 and exp["n_inliers"] == 266
    wrong_at = [i for i, (q, _) in enumerate(exp["candidates"]) if int(q) in case["wrong"]]
    assert wrong_at == [63, 64, 255, 256]
    inl = [tuple(m) for m, k in zip(exp["candidates"].tolist(), exp["mask"]) if k]
    assert inl[63][1] == inl[64][1] and inl[255][1] == inl[256][1]
    assert exp["remove_ids"].tolist() == [64, 256]
    assert cnp.scene("five")[1]["n_candidates"] == 5 and cnp.scene("five")[1]["status"] == 0
    assert cnp.scene("four")[1]["n_candidates"] == 4 and cnp.scene("four")[1]["status"] == 4
    assert cnp.scene("unrelated")[1]["status"] == 3 and cnp.scene("one_current")[1]["status"] == 3
    assert cnp.scene("no_current")[1]["status"] == 1 and cnp.scene("no_received")[1]["status"] == 2


def test_duplicates_scene_holds_the_patterns_and_is_not_deduplicated():
    case, exp = cnp.scene("duplicates")
    trains = [int(t) for (q, t), k in zip(exp["candidates"], exp["mask"]) if k]
    assert trains[:27] == [0, 1, 1, 0, 20, 21, 2, 3, 4, 3, 2, 22, 23, 5, 5, 5, 24, 25, 6, 7, 8, 9, 9, 8, 7, 26, 27]
    good_t = exp["good"][:, 1].tolist()
    assert len(set(good_t)) < len(good_t)                      # a train index survives twice
    assert len(exp["remove_ids"]) == 9


@pytest.mark.parametrize("name", cnp.RANSAC_SCENES)
def test_the_fast_list_work_equals_the_restatement(name):
    """correspond_np.mask_and_erase, which the scene beyond 4096 rows is held against, gives what ref_pr.good_matches gives."""
    _, exp = cnp.scene(name)
    remove_ids, good = cnp.mask_and_erase([tuple(m) for m in exp["candidates"].tolist()], exp["mask"])
    assert remove_ids == exp["remove_ids"].tolist() and good == [tuple(m) for m in exp["good"].tolist()]
    for trains in ([0, 1, 2, 1, 0], [0, 1, 1, 0], [3, 0, 1, 2, 2, 1, 0], [5, 5, 5, 5], [1, 2, 1, 2, 1]):
        cand = list(enumerate(trains))
        assert cnp.mask_and_erase(cand, np.ones(len(cand), np.uint8)) == (cnp.first_later_twin(cand), _quirk(trains))


def test_the_large_scene_crosses_4096():
    case = cnp.large()
    land = case["land"].tolist()
    assert len(land) == 4260 and len(set(land)) < len(land)
    second = [i for i, l in enumerate(land) if l in land[:i]]
    assert min(second) < 4096 <= max(second)                   # second sightings on both sides of the boundary


def _quirk(trains):
    """good_matches on a 2-NN result whose every query passes the tests with first neighbour trains[q]."""
    n = len(trains)
    idx = np.stack([np.array(trains), np.full(n, 99)], axis=1).astype(np.int32)
    dist = np.stack([np.full(n, 5), np.full(n, 100)], axis=1).astype(np.int32)
    return ref_pr.good_matches(idx, dist, cnp.MIN_D, cnp.RATIO, inlier_mask=np.ones(n, np.uint8))


def test_the_erase_loop_is_not_a_clean_deduplication():
    assert _quirk([0, 1, 2, 1, 0]) == [(0, 0), (1, 1), (3, 1)]
    assert [q for q, _ in _quirk([0, 1, 1, 0])] == [0, 2]
    assert [q for q, _ in _quirk([3, 0, 1, 2, 2, 1, 0])] == [0, 1, 3, 5]
    assert cnp.first_later_twin([(q, t) for q, t in enumerate([0, 1, 2, 1, 0])]) == [4, 3]
