"""Conditions on the yardstick of vba_search_for_initialization alone (tests/search_init_ref.py over tests/search_init_cases.py),
checked on the CPU: the float64 yardstick equals the longdouble one in every output, nothing sits on a threshold, the cases exercise
every state, the steals and the dependency on earlier queries, the hand-made cases have the answers their docstrings give, and the
prototype of the kernel's pass equals the sequential loop."""
import numpy as np
import pytest

import search_init_cases as cases_mod
import search_init_ref as ref_mod

NAMES = list(cases_mod.cases())
MARGIN = 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_float64_equals_longdouble_with_margins(name):
    a, b = cases_mod.ref(name), cases_mod.ref(name, "longdouble")
    assert ref_mod.differences(a, b) == []
    assert a["prev_matched"].tobytes() == b["prev_matched"].tobytes()
    assert np.array_equal(a["n_cand"], b["n_cand"])
    print(name, "margin %.3g over %d comparisons, %.3g over %d roundings" % (a["margin"], a["n_fp"], a["margin_r"], a["n_round"]))
    assert a["margin"] >= MARGIN and a["margin_r"] >= MARGIN


def test_coverage():
    states = np.zeros(7, dtype=np.int64)
    matches = steals = moved = 0
    for name in NAMES:
        a, b = cases_mod.ref(name), cases_mod.ref(name, ignore_claims=True)
        states += np.bincount(a["state"], minlength=7)[:7]
        matches += a["n_matches"]
        steals += a["n_stolen"]
        moved += int((a["best_idx"] != b["best_idx"]).sum())
    print("states", states, "matches", matches, "steals", steals, "best_idx moved by earlier queries", moved)
    assert (states > 0).all()
    assert matches >= 500 and steals >= 50 and moved >= 50


def test_micro_by_hand():
    a, e = cases_mod.ref("micro"), cases_mod.micro_expect()
    for k, v in e.items():
        assert np.array_equal(np.asarray(a[k]), np.asarray(v)), (k, a[k], v)
    assert list(a["hist"][:4]) == [3, 1, 1, 1] and a["hist"].sum() == 6
    p = cases_mod.cases()["micro"]
    want = p.prev_matched.copy()
    for i in (0, 6, 7, 8):
        want[i] = p.uv2[a["match12"][i]]
    assert a["prev_matched"].tobytes() == want.tobytes()


def test_hand_made_by_hand():
    r = cases_mod.ref
    a = r("steal")
    assert list(a["state"]) == [5, 0] and (a["n_matches"], a["n_stolen"]) == (1, 1) and list(a["match21"]) == [1, -1] and a["matched_dist"][0] == 3
    a = r("equal_no_steal")
    assert list(a["state"]) == [0, 0, 0, 3] and list(a["best_idx"]) == [0, 1, 2, -1] and list(a["best_dist"]) == [5, 20, 7, 256] and a["n_stolen"] == 0
    a, b = r("ratio_flip"), r("ratio_flip", ignore_claims=True)
    assert list(a["state"]) == [0, 0] and list(a["best_idx"]) == [0, 1] and list(a["best_dist"]) == [2, 11]
    assert b["state"][1] == 4 and (b["best_dist"][1], b["best_dist2"][1]) == (10, 11)
    a = r("int_max_ratio")
    assert list(a["state"]) == [0] and (a["best_dist"][0], a["best_dist2"][0]) == (40, 256) and a["n_matches"] == 1
    a = r("stolen_in_hist")
    assert list(a["hist"][:5]) == [4, 3, 1, 2, 1] and list(a["ind"]) == [0, 1, 3]
    assert list(a["state"]) == [0, 0, 0, 0, 0, 6, 0, 5, 5, 0, 0] and (a["n_before_filter"], a["n_stolen"], a["n_matches"]) == (9, 2, 8)
    assert list(a["match21"]) == [0, 1, 2, 3, 4, 5, 6, 9, 10]          # the filter leaves vnMatches21 alone
    a = r("steal_chain_40")
    assert (a["n_matches"], a["n_stolen"]) == (1, 39) and list(a["state"]) == [5] * 39 + [0] and a["matched_dist"][0] == 6
    a = r("dep_chain_40")
    assert list(a["best_idx"]) == list(range(40)) and list(a["best_dist"]) == [5 * j + 1 for j in range(1, 41)] and a["n_matches"] == 40
    a = r("crowd_64")
    d = [1 + (37 * i + 11) % 50 for i in range(64)]
    accepted = [i for i in range(64) if d[i] < min(d[:i], default=1 << 30)]
    assert [i for i in range(64) if a["state"][i] in (0, 5)] == accepted and a["n_matches"] == 1 and a["n_stolen"] == len(accepted) - 1
    a = r("border")
    assert list(a["state"][:6]) == [2, 2, 2, 2, 0, 0] and a["state"][7] == 0 and list(a["n_cand"][:4]) == [0, 0, 0, 0]
    a = r("upper_levels_only")
    assert list(a["state"]) == [1, 1] and a["n_matches"] == 0
    for name in ("empty_keys1", "empty_keys2"):
        assert r(name)["n_matches"] == 0
    assert set(r("empty_keys2")["state"]) <= {1, 2}


@pytest.mark.parametrize("name", NAMES)
def test_prototype_of_the_pass_equals_the_sequential_loop(name):
    a, c = cases_mod.ref(name), cases_mod.proto(name)
    assert ref_mod.differences(a, c) == []
    assert a["prev_matched"].tobytes() == c["prev_matched"].tobytes()
    nq = cases_mod.n_queries(cases_mod.cases()[name])
    assert 1 <= c["rounds"] <= nq + 1
    if name == "dep_chain_40":
        assert c["rounds"] == 41
    if name == "steal_chain_40":
        assert c["rounds"] == 2
