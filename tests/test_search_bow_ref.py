"""The yardstick of vba_search_by_bow (tests/search_bow_ref.py) on the CPU: hand-worked expectations for the micro, tie, threshold
and ratio-flip cases, the float32 product, and a NumPy model of the kernel's fixed-point pass against the sequential loop, with the
node-local bound on its rounds."""
import numpy as np
import pytest

import search_bow_cases as cases
import search_bow_ref as ref_mod
from mc_slam_amd import abi

HAND = ["micro", "states", "ratio_flip_fail", "ratio_flip_pass", "all_taken", "tie_fails", "tie_first_wins", "float32_product", "orientation_drop",
        "one_sided_nodes", "bad_mp2_kf", "bad_mp2_frame", "th_equal_frame", "th_equal_kf", "th_zero_frame", "th_zero_kf", "th_255_frame", "th_255_kf"]


@pytest.mark.parametrize("name", HAND)
def test_hand_worked(name):
    w = cases.ref(name)
    for i, (state, best, d1, d2) in cases.expect(name).items():
        assert (w["state"][i], w["best_idx"][i], w["best_dist"][i], w["best_dist2"][i]) == (state, best, d1, d2), (name, i)
        assert w["match12"][i] == (best if state == 0 else -1)
    assert w["n_matches"] == sum(1 for e in cases.expect(name).values() if e[0] == 0) == int((w["match21"] >= 0).sum())


def test_hand_cases_say_what_they_claim():
    r = cases.ref
    assert set(r("states")["state"]) == {0, 1, 2, 3, 4}
    # the flips: alone (the first query without a map point) the second query decides otherwise
    for name, alone, after in (("ratio_flip_fail", 0, 4), ("ratio_flip_pass", 4, 0)):
        p = cases.cases()[name]
        solo = ref_mod.search_bow_ref(p.copy(good_mp1=np.array([0, 1])))
        assert solo["state"][1] == alone and r(name)["state"][1] == after
    assert r("th_equal_frame")["n_matches"] == 1 and r("th_equal_kf")["n_matches"] == 0
    assert r("th_255_frame")["n_matches"] == 2 and r("th_255_kf")["n_matches"] == 1
    assert r("bad_mp2_kf")["match12"][0] == 1 and r("bad_mp2_frame")["match12"][0] == 0
    d = r("orientation_drop")
    assert list(d["hist"][:4]) == [3, 1, 1, 1] and list(d["ind"]) == [0, 1, 2] and d["state"][5] == 5 and d["match21"][5] == -2 and d["bin"][5] == 3
    assert (d["n_before_filter"], d["n_matches"]) == (6, 5)
    for name in ("empty_keys1", "empty_keys2", "no_shared_node"):
        assert r(name)["n_matches"] == 0 and r(name)["n_q"] == 0 and set(r(name)["state"]) <= {1, 2}
    assert r("no_orientation")["n_matches"] == r("no_orientation")["n_before_filter"] > 20 and not r("no_orientation")["hist"].any()
    assert [r(n)["n_q"] for n in ("queries_256", "queries_257", "queries_513")] == [256, 257, 513]
    assert r("node_70")["max_node_q"] == 70 and r("node_300")["max_node_q"] == 300
    assert cases.cases()["max_keys"].n_keys2 == abi.SEARCH_BOW_MAX_KEYS and r("max_keys")["n_matches"] > 20
    assert r("realistic_frame")["n_matches"] + r("realistic_kf")["n_matches"] >= 500
    assert (r("realistic_kf")["state"] == 5).any() and (r("realistic_frame")["match21"] == -2).any()


def test_the_float32_product():
    """0.6f * 10: the reference's float32 product refuses what a float64 product accepts.  For the ratios the reference uses, 0.75f
    (LoopClosing.cpp:285, Tracking.cpp:2405) and 0.7f (Tracking.cpp:1597), no pair of distances in 0 .. 256 decides differently:
    0.75f * b is exact, and 0.7f lies BELOW 0.7, so a product never rounds down onto an integer it exceeds"""
    assert (6, 10) in cases.float32_flips(0.6)
    assert np.float32(6) < np.float64(np.float32(0.6)) * 10.0 and not (np.float32(6) < np.float32(0.6) * np.float32(10))
    assert cases.ref("float32_product")["state"][0] == 4
    assert cases.float32_flips(0.75) == [] and cases.float32_flips(0.7) == []
    assert cases.float32_flips(0.9) == [] and cases.float32_flips(0.8) != []     # 0.8f lies above 0.8


def _same(a, b, what):
    for k in cases.INTS:
        assert np.array_equal(a[k], b[k]), (what, k)
    assert (a["n_matches"], a["n_before_filter"]) == (b["n_matches"], b["n_before_filter"]), what


@pytest.mark.parametrize("name", [n for n in cases.cases() if n not in ("max_keys",)])
def test_fixed_point_equals_the_sequential_loop(name):
    w = cases.ref(name)
    f = ref_mod.search_bow_fixed_point(cases.cases()[name])
    _same(f, w, name)
    assert 1 <= f["rounds"] <= w["max_node_q"] + 1


def test_the_node_local_bound():
    """the 40-chain needs about 40 rounds in one node and about 5 when it is split over 8 nodes; without the node-local skip the
    result is the same"""
    one, split = ref_mod.search_bow_fixed_point(cases.cases()["chain_40"]), ref_mod.search_bow_fixed_point(cases.cases()["chain_8x5"])
    assert 30 <= one["rounds"] <= cases.CHAIN + 1 and split["rounds"] <= 6
    assert one["n_matches"] == split["n_matches"] == cases.CHAIN
    for name in ("chain_8x5", "crowd_frame", "crowd_kf", "node_70"):
        g = ref_mod.search_bow_fixed_point(cases.cases()[name], node_local=False)
        _same(g, cases.ref(name), name)
    assert max(ref_mod.search_bow_fixed_point(cases.cases()[n])["rounds"] for n in ("crowd_frame", "crowd_kf")) > 2


def test_fixed_point_on_random_tiny_pairs():
    """a few hundred pairs of a handful of keypoints in one to three nodes, descriptors a few bits apart so that most queries
    contend, both modes, thresholds and ratios varied"""
    r = np.random.default_rng(7)
    flips = 0
    for k in range(300):
        mode = int(r.integers(2))
        n1, n2, nn = int(r.integers(1, 9)), int(r.integers(0, 9)), int(r.integers(1, 4))
        s1 = [(int(r.integers(nn)), int(r.integers(0, 24)), int(r.random() < 0.85)) for _ in range(n1)]
        s2 = [(int(r.integers(nn)) + int(r.random() < 0.1) * 7, int(r.integers(0, 24)), int(r.random() < 0.8)) for _ in range(n2)]
        p = cases.pair(mode, s1, s2, th_low=int(r.choice([3, 8, 50])), nn_ratio=float(r.choice([0.6, 0.75, 0.9, 1.0, 1.5])))
        w, f = ref_mod.search_bow_ref(p), ref_mod.search_bow_fixed_point(p)
        _same(f, w, k)
        assert f["rounds"] <= w["max_node_q"] + 1
        flips += f["rounds"] > 2
    assert flips > 30
