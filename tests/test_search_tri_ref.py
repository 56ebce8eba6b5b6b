"""The yardstick of vba_search_triangulation (tests/search_tri_ref.py) against itself (CPU only): the three dtypes, the margins of
every floating-point comparison it evaluates, the two forms of the candidate loop, known answers."""
import numpy as np
import pytest

import search_tri_cases as cases
import search_tri_ref as ref_mod

NAMES = list(cases.cases())
MARGIN = 1e-9       # tests/test_gpu_search_tri.py demands equality with nothing excused because of this


@pytest.mark.parametrize("name", NAMES)
def test_float64_equals_longdouble(name):
    assert ref_mod.differences(cases.ref(name), cases.ref(name, "longdouble")) == []
    assert ref_mod.differences(cases.ref(name, toggle=True), cases.ref(name, "longdouble", toggle=True)) == []


def test_every_comparison_has_a_margin():
    """every evaluated floating-point comparison (epipole gate, epipolar gate) lies at least MARGIN relative from its threshold, in
    float64 and in longdouble, with check_orientation either way"""
    worst = min((cases.ref(n, dt, toggle=t)["margin"], n) for n in NAMES for dt in ("float64", "longdouble") for t in (False, True))
    n_fp = sum(cases.ref(n)["n_fp"] for n in NAMES)
    print("comparisons %d  smallest margin %.3e (%s)" % (n_fp, worst[0], worst[1]))
    assert n_fp > 1000 and worst[0] >= MARGIN


def test_print_float32_against_float64():
    """how many decisions move when the gates run in float32, as the reference computes them (recorded in DESIGN.md, not asserted)"""
    moved = keys = 0
    for n in NAMES:
        a, b = cases.ref(n), cases.ref(n, "float32")
        moved += int((a["match12"] != b["match12"]).sum() + ((a["match12"] == b["match12"]) & (a["state"] != b["state"])).sum())
        keys += len(a["state"])
    print("float32 against float64: %d of %d keypoints of keyframe 1 change their match or state" % (moved, keys))


@pytest.mark.parametrize("name", NAMES)
def test_min_form_equals_sequential_form(name):
    assert ref_mod.differences(cases.ref(name), cases.ref(name, form="min")) == []


def test_known_answer_clean_pair():
    """with little noise, no map points and no orientation filter every true pair in a shared node is found and no distractor is matched"""
    from mc_slam_amd import synth
    p = synth.synth_match_pair(77, n_true=120, n_distract1=40, n_distract2=40, n_nodes=15, flip_bits=10, unshared=0.25, mp1=0, mp2=0,
                               angle_noise=0.5, rot_outliers=0, noise=0.1, check_orientation=False)
    r = ref_mod.search_tri_ref(p)
    pair, shared = p.truth["pair"], p.truth["shared"]
    assert shared.sum() > 60 and (~shared).sum() > 10
    want = np.full(p.n_keys1, -1)
    want[pair[shared, 0]] = pair[shared, 1]
    assert np.array_equal(r["match12"], want)
    assert r["n_matches"] == r["n_before_filter"] == shared.sum() and np.array_equal(r["pairs"][:, 0], np.sort(pair[shared, 0]))
    assert set(r["state"][pair[~shared, 0]]) <= {2, 3}


def test_hand_made_answers():
    r = cases.ref("micro")
    for i, (idx2, state, dist) in cases.micro_expect().items():
        assert (r["match12"][i], r["state"][i], r["best_dist"][i]) == (idx2, state, dist), i
    assert len(set(r["pairs"][:, 1])) < len(r["pairs"])                     # two queries share an idx2
    d = cases.ref("den0")
    assert list(d["state"]) == [3, 0, 0] and list(d["match12"]) == [-1, 1, 1]    # den == 0 for query 0; the last of equals for the others
    j = cases.ref("jumps")
    assert sorted(set(i for i, _, _ in j["queries"])) == [4, 5, 10, 11, 14, 15] and j["n_matches"] == 6
    assert cases.ref("no_shared")["n_matches"] == 0 and set(cases.ref("no_shared")["state"]) == {2}
    assert cases.ref("empty1")["match12"].shape == (0,) and set(cases.ref("empty2")["state"]) <= {1, 2}
    b = cases.cases()["big_node"]
    assert max(np.diff(b.node_begin1)) >= 300 and max(np.diff(b.node_begin2)) >= 300 and (np.diff(b.node_begin1) <= 3).sum() > 20
    assert (np.diff(cases.cases()["synth_mid"].node_feat2) < 0).any()


def test_orientation_cases():
    r = cases.ref("ori_round")
    assert list(r["hist"][[0, 1, 4, 5, 12]]) == [0, 6, 0, 4, 1]              # half to even would give 2 in bin 0 and 3 in bin 4
    f = np.float32(1.0) / np.float32(30)
    assert np.float32(cases.half_rot(0) * f) == np.float32(0.5) and np.float32(cases.half_rot(4) * f) == np.float32(4.5)
    assert ref_mod.round_half_away(np.float32(0.5)) == 1 and ref_mod.round_half_away(np.float32(4.5)) == 5 and ref_mod.round_half_away(np.float32(2.4999998)) == 2
    for name, ind, n in (("ori_max2_cut", [3, -1, -1], 21), ("ori_max3_cut", [3, 5, -1], 31), ("ori_edge", [3, 5, 7], 24), ("ori_equal", [2, 4, 6], 15),
                         ("ori_one_bin", [4, -1, -1], 12)):
        r = cases.ref(name)
        assert list(r["ind"]) == ind and r["n_matches"] == n and (r["state"] == 4).sum() == r["n_before_filter"] - n
        off = cases.ref(name, toggle=True)
        assert off["n_matches"] == off["n_before_filter"] == r["n_before_filter"] and not off["hist"].any() and list(off["ind"]) == [-1, -1, -1]
    assert max(cases.ref(n)["hist"][13:].max() for n in NAMES) == 0           # only bins 0 .. 12 can occur
    assert any((cases.cases()[n].angle1[:, None] < cases.cases()[n].angle2[None, :]).any() for n in ("synth_small", "synth_mid"))
