"""The yardstick of vba_search_by_sim3 (tests/search_sim3_ref.py) against itself (CPU only): the three dtypes, the margins of every
floating-point comparison and rounding it evaluates, the two forms of the candidate loop, known answers.  vba_search_by_sim3 returns
no floating-point value (matches, distances, levels, states and counts only), so there is no tolerance to derive: the GPU test
compares every output for equality."""
import numpy as np
import pytest

import search_sim3_cases as cases
import search_sim3_ref as ref_mod

NAMES = list(cases.cases())
MARGIN = 1e-9       # tests/test_gpu_search_sim3.py demands equality with nothing excused because of this (the figure of test_fuse_ref.py)


@pytest.mark.parametrize("name", NAMES)
def test_float64_equals_longdouble(name):
    assert ref_mod.differences(cases.ref(name), cases.ref(name, "longdouble")) == []


@pytest.mark.parametrize("name", NAMES)
def test_min_form_equals_sequential_form(name):
    assert ref_mod.differences(cases.ref(name), cases.ref(name, form="min")) == []


def test_every_comparison_and_rounding_has_a_margin():
    """every evaluated <, > or >= lies at least MARGIN relative from its threshold and every floor or ceil argument at least MARGIN from
    an integer, in float64 and in longdouble"""
    worst = min((cases.ref(n, dt)["margin"], n) for n in NAMES for dt in ("float64", "longdouble"))
    worst_r = min((cases.ref(n, dt)["margin_r"], n) for n in NAMES for dt in ("float64", "longdouble"))
    n_fp, n_round = sum(cases.ref(n)["n_fp"] for n in NAMES), sum(cases.ref(n)["n_round"] for n in NAMES)
    print("comparisons %d  smallest margin %.3e (%s)   roundings %d  smallest margin %.3e (%s)" % ((n_fp,) + worst + (n_round,) + worst_r))
    assert n_fp > 10000 and n_round > 2000 and worst[0] >= MARGIN and worst_r[0] >= MARGIN


def test_states_and_counts():
    """over all cases at least 500 matches are agreed and every state occurs in both directions"""
    for sfx in ("1", "2"):
        count = np.bincount(np.concatenate([cases.ref(n)["state" + sfx] for n in NAMES]), minlength=9)
        print("keypoints of keyframe %s per state 0 .. 8:" % sfx, count.tolist())
        assert (count > 0).all() and len(count) == 9
    found = sum(cases.ref(n)["n_found"] for n in NAMES)
    print("agreed matches over all cases:", found)
    assert found >= 500
    for n in NAMES:                                                           # what the outputs mean to each other
        r = cases.ref(n)
        for sfx in ("1", "2"):
            assert ((r["match" + sfx] >= 0) == (r["state" + sfx] == 0)).all()
            assert (r["best_dist" + sfx][r["state" + sfx] == 0] <= cases.cases()[n].th_high).all()
        m = r["match12"] >= 0
        assert r["n_found"] == m.sum() and (r["match12"][m] == r["match1"][m]).all() and (r["match2"][r["match12"][m]] == np.nonzero(m)[0]).all()


def test_print_float32_against_float64():
    """how many keypoints move when everything runs in float32, as the reference computes it (recorded in DESIGN.md, not asserted)"""
    moved = pts = 0
    for n in NAMES:
        if n == "z_zero":
            continue
        a, b = cases.ref(n), cases.ref(n, "float32")
        for sfx in ("1", "2"):
            moved += int(((a["state" + sfx] != b["state" + sfx]) | (a["match" + sfx] != b["match" + sfx])).sum())
            pts += int((a["state" + sfx] >= 3).sum() + (a["state" + sfx] == 0).sum())
    print("float32 against float64: %d of %d queries change their state or match" % (moved, pts))


@pytest.mark.parametrize("name", [n for n in cases.HAND if n != "border_all"])
def test_hand_made_answers(name):
    expect, first = cases.hand_expect(name)
    for dt in (("float32", "float64", "longdouble") if name == "z_zero" else ("float64",)):      # z_zero is exact in every dtype
        r = cases.ref(name, dt)
        for d, sfx in enumerate(("1", "2")):
            assert len(expect[d]) >= 2
            for k, want in enumerate(expect[d]):
                i = first[d] + k
                assert (r["state" + sfx][i], r["match" + sfx][i], r["best_dist" + sfx][i], r["level" + sfx][i]) == want, (d, k)
            assert (r["state" + sfx][:first[d]] == 1).all()                   # the targets carry no point
    if name == "micro":
        r, p = cases.ref(name), cases.cases()[name]
        assert sorted(r["state1"][r["state1"] != 1]) == [0, 2, 3, 4, 5, 6, 7, 8, 8] == sorted(r["state2"][r["state2"] != 1])
        assert (p.kf1.n_keys, p.kf2.n_keys) == (8 + 9 + 2, 8 + 9 + 3) and r["n_found"] == 0
        assert list(r["level1"][[12, 14]]) == [5, 1] and list(r["level2"][[12, 14]]) == [4, 1]    # state 6 holds the TARGET's n_levels
    if name == "tie_cells":
        for kf in (cases.cases()[name].kf1, cases.cases()[name].kf2):
            f = list(kf.cell_feat)
            assert f.index(5) + 1 == f.index(3) and f.index(7) < f.index(2)   # one cell lists 5 in front of 3; 7 sits in an earlier column


def test_negative_radius_empties_one_axis():
    """every query of one_axis_empty passes the four returns of GetFeaturesInArea; the clamped cell range holds columns and no row in
    keyframe 1 and rows and no column in keyframe 2.  The ranges are taken at the pixels the queries were placed at; the yardstick
    projects to within 1e-9 pixels of them (its own roundings are covered by test_every_comparison_and_rounding_has_a_margin), and
    the floor and ceil arguments here keep 1e-6 from an integer"""
    from fuse_ref import cell_range
    p = cases.cases()["one_axis_empty"]
    for d, (tgt, x_empty) in enumerate(((p.kf2, True), (p.kf1, False))):
        fp = ref_mod._Fp()
        G = cases.GEOM_FLAT[1 - d]
        assert (tgt.grid_cols, tgt.grid_rows) == (G["cols"], G["rows"])
        for i, (u, v) in enumerate(cases.one_axis_empty_uv(G)):
            cells = cell_range(tgt, fp, np.float64, np.float64(u), np.float64(v), np.float64(p.th) * np.float64(tgt.scale[0]))
            print("direction", d, "query", i, "uv", (u, v), "cells x %s .. %s  y %s .. %s" % (cells or (None,) * 4))
            assert cells is not None
            nx0, nx1, ny0, ny1 = cells
            assert (nx1 < nx0 and ny0 <= ny1) if x_empty else (nx0 <= nx1 and ny1 < ny0), (d, i, cells)
        assert fp.n_round == 16 and fp.margin_r >= 1e-6


def test_agreement_cases():
    r, e = cases.ref("agree"), cases.agree_expect()
    for k, want in e.items():
        assert np.asarray(r[k]).tolist() == want, k


def test_border_scale_and_empty_cases():
    a = cases.ref("border_all")                                               # every keypoint of a cell is in the area; the level gate still holds
    assert set(a["state1"]) == {0, 1, 8} == set(a["state2"]) and (a["state1"] == 0).sum() >= 4
    m, h, t = cases.ref("micro"), cases.ref("scale_half"), cases.ref("scale_two")
    n = len(h["state1"])
    for k in ref_mod.INT_KEYS[1:]:                                            # the same answers under s12 = 0.5, 1.25 and 2
        assert np.array_equal(h[k], t[k]) and np.array_equal(h[k], m[k][:len(h[k])]), k
    ps = cases.cases()
    assert not np.allclose(ps["scale_half"].kf1.pos[n - 1], ps["scale_two"].kf1.pos[n - 1])
    for name, n1, n2 in (("queries_1_0", 1, 0), ("queries_255_3", 255, 3), ("queries_256_0", 256, 0), ("queries_257_3", 257, 3), ("queries_513_0", 513, 0),
                         ("queries_3_257", 3, 257), ("empty_kf1", 0, None), ("empty_kf2", None, 0), ("nothing_searchable", 0, 0)):
        r = cases.ref(name)
        for sfx, want in (("1", n1), ("2", n2)):
            if want is not None:
                assert ((r["state" + sfx] != 1) & (r["state" + sfx] != 2)).sum() == want, (name, sfx)
    assert ps["empty_kf1"].kf1.n_keys == 0 and ps["empty_kf2"].kf2.n_keys == 0 and cases.ref("empty_kf1")["match12"].shape == (0,)
    assert (cases.ref("empty_kf1")["state2"] >= 7).sum() > 5 and (cases.ref("empty_kf2")["state1"] >= 7).sum() > 5


def test_generator():
    from mc_slam_amd import synth
    p = cases.cases()["synth_mid"]
    assert (p.kf1.n_keys, p.kf2.n_keys, p.kf1.n_levels, p.kf1.grid_cols, p.kf1.grid_rows) == (1000, 1100, 8, 64, 48) and p.s12 != 1.0
    for kf in (p.kf1, p.kf2):
        for a in (kf.uv, kf.pos, kf.dist_min, kf.dist_max, kf.pred_max, kf.Rcw, kf.tcw, kf.scale):
            assert np.array_equal(a, a.astype(np.float32).astype(np.float64))    # everything went through float32
        assert kf.cell_begin[0] == 0 and kf.cell_begin[-1] == len(kf.cell_feat) <= kf.n_keys and len(set(kf.cell_feat)) == len(kf.cell_feat)
    for a in (p.K, p.R12, p.t12, np.array([p.s12])):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    kind, k1, k2 = p.truth["kind"], p.truth["key1"], p.truth["key2"]
    r = cases.ref("synth_mid")
    kd = lambda name: kind == synth.SIM3_SEARCH_KINDS.index(name)
    m = kd("match")
    assert (r["match12"][k1[m]] == k2[m]).mean() > 0.95 and r["n_found"] >= 0.95 * m.sum()
    assert (np.unpackbits(p.kf1.desc[k1[m]] ^ p.kf2.desc[k2[m]], axis=1).sum(axis=1) == 12).all()
    # the two map copies of a feature disagree in world space, as before a loop is closed
    assert np.linalg.norm(p.kf1.pos[k1[m]] - p.kf2.pos[k2[m]], axis=1).min() > 0.05
    for name, s1, s2 in (("matched", 2, 2), ("no_pt1", 1, 0), ("no_pt2", 0, 1), ("far_desc", 8, 8), ("behind", 3, 3), ("outside", 4, 4), ("distance", 5, 5),
                         ("level_high", 6, 6)):
        assert (r["state1"][k1[kd(name)]] == s1).all() and (r["state2"][k2[kd(name)]] == s2).all() and kd(name).sum() > 5, name
    assert (r["match12"][k1[~m]] == -1).all()
    # distractors in the areas: a found keypoint chose among several candidates
    s = cases.cases()["synth_small"]
    assert (s.kf2.n_levels, s.kf2.grid_cols, s.kf2.bounds[1]) == (6, 50, 600.0) and cases.ref("synth_small")["n_found"] > 20
