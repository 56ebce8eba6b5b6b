"""The yardstick of vba_search_by_projection (tests/search_proj_ref.py, the sequential loop) against itself (CPU only): the three
dtypes, the margins of every floating-point comparison and rounding it evaluates, known answers, how much the queries depend on each
other, and a Python prototype of the kernel's conflict pass against the sequential loop."""
import math

import numpy as np
import pytest

import search_proj_cases as cases
import search_proj_ref as ref_mod
from mc_slam_amd import abi

NAMES = list(cases.cases())
MARGIN = 1e-9       # tests/test_gpu_search_proj.py demands equality with nothing excused because of this


@pytest.mark.parametrize("name", NAMES)
def test_float64_equals_longdouble(name):
    assert ref_mod.differences(cases.ref(name), cases.ref(name, "longdouble")) == []


def test_every_comparison_and_rounding_has_a_margin():
    """every evaluated <, > or >= lies at least MARGIN relative from its threshold and every floor or ceil argument at least MARGIN from
    an integer, in float64 and in longdouble"""
    worst = min((cases.ref(n, dt)["margin"], n) for n in NAMES for dt in ("float64", "longdouble"))
    worst_r = min((cases.ref(n, dt)["margin_r"], n) for n in NAMES for dt in ("float64", "longdouble"))
    n_fp, n_round = sum(cases.ref(n)["n_fp"] for n in NAMES), sum(cases.ref(n)["n_round"] for n in NAMES)
    print("comparisons %d  smallest margin %.3e (%s)   roundings %d  smallest margin %.3e (%s)" % ((n_fp,) + worst + (n_round,) + worst_r))
    assert n_fp > 10000 and n_round > 2000 and worst[0] >= MARGIN and worst_r[0] >= MARGIN


def test_tolerances_come_from_longdouble():
    """the uv and view_cos tolerances of the GPU test are ten times the largest float64-against-longdouble difference, rounded up to
    one digit"""
    for key, measured, tol, unit in (("uv", cases.UV_LONGDOUBLE, cases.UV_TOL, "pixels"), ("view_cos", cases.COS_LONGDOUBLE, cases.COS_TOL, "")):
        worst = max(ref_mod.real_difference(cases.ref(n), cases.ref(n, "longdouble"), key) for n in NAMES)
        print("largest |%s| difference float64 against longdouble: %.3e %s; tolerance %.0e" % (key, worst, unit, tol))
        assert 0 < worst <= measured
        e = 10 ** math.floor(math.log10(10 * measured))
        assert tol == pytest.approx(math.ceil(10 * measured / e) * e, rel=1e-12)


def test_states_and_counts():
    """over all cases every state of either mode occurs and at least 500 queries match"""
    total = 0
    for mode, n_states in ((cases.LAST, 7), (cases.LOCAL, 10)):
        names = [n for n in NAMES if cases.cases()[n].mode == mode]
        count = np.bincount(np.concatenate([cases.ref(n)["state"] for n in names]), minlength=n_states)
        print("mode %d: queries per state 0 .. %d:" % (mode, n_states - 1), count.tolist())
        assert (count > 0).all() and len(count) == n_states
        total += sum(cases.ref(n)["n_matches"] for n in names)
    assert total >= 500


def test_the_queries_depend_on_each_other():
    """at least 50 queries end on a different keypoint than they would with the claims of the call ignored"""
    moved = other = 0
    for n in NAMES:
        a, b = cases.ref(n), cases.ref(n, ignore_claims=True)
        d = a["best_idx"] != b["best_idx"]
        moved += int(d.sum())
        other += int((d & (a["best_idx"] >= 0) & (b["best_idx"] >= 0)).sum())
    print("queries whose best_idx the claims change: %d, of them on another keypoint (not on none): %d" % (moved, other))
    assert other >= 50


def test_print_float32_against_float64():
    """how many queries move when everything runs in float32, as the reference computes it (recorded in DESIGN.md, not asserted)"""
    moved = qs = 0
    for n in NAMES:
        if n.startswith("z_zero") or n == "max_keys":
            continue
        a, b = cases.ref(n), cases.ref(n, "float32")
        moved += int(((a["state"] != b["state"]) | (a["best_idx"] != b["best_idx"])).sum())
        qs += len(a["state"])
    print("float32 against float64: %d of %d queries change their state or best_idx" % (moved, qs))


def _check_uv(r, i, uv):
    if uv is None:
        assert np.isnan(r["uv"][i]).all(), i
    else:
        assert np.abs(r["uv"][i] - uv).max() < 1e-9, i


def test_hand_made_micro_cases():
    r = cases.ref("micro_last")
    expect, totals = cases.micro_expect(cases.LAST)
    for i, (state, idx, dist, b, uv) in expect.items():
        assert (r["state"][i], r["best_idx"][i], r["best_dist"][i], r["bin"][i]) == (state, idx, dist, b), i
        _check_uv(r, i, uv)
    assert sorted(r["state"]) == [0, 0, 0, 0, 1, 2, 3, 4, 5, 6]
    for k, v in totals.items():
        assert np.array_equal(np.asarray(r[k]), np.asarray(v)), k
    assert (r["best_dist2"] == 256).all() and (r["level"] == -128).all() and np.isnan(r["view_cos"]).all()
    r = cases.ref("micro_local")
    expect, totals = cases.micro_expect(cases.LOCAL)
    for i, (state, idx, dist, dist2, level, uv) in expect.items():
        assert (r["state"][i], r["best_idx"][i], r["best_dist"][i], r["best_dist2"][i], r["level"][i]) == (state, idx, dist, dist2, level), i
        _check_uv(r, i, uv)
    assert sorted(r["state"]) == list(range(10)) and (r["bin"] == 255).all() and (r["hist"] == 0).all() and list(r["ind"]) == [-1, -1, -1]
    for k, v in totals.items():
        assert np.array_equal(np.asarray(r[k]), np.asarray(v)), k
    # isInFrustum returned true for exactly the states 0 and 7 .. 9: they hold mTrackViewCos and mnTrackScaleLevel
    seen = np.isin(r["state"], (0, 7, 8, 9))
    assert (r["level"][seen] >= 0).all() and np.allclose(r["view_cos"][seen], 1.0, atol=1e-12) and np.isnan(r["view_cos"][1:5]).all()
    assert r["view_cos"][5] == pytest.approx(-1.0) and r["view_cos"][6] == pytest.approx(1.0)


def test_hand_made_dependency_cases():
    for name, want in cases.hand_expect().items():
        r = cases.ref(name)
        for k, v in want.items():
            assert np.array_equal(np.asarray(r[k]), np.asarray(v)), (name, k, r[k], v)
    c = cases.ref("chain_40")
    assert list(c["best_idx"]) == list(range(cases.CHAIN)) and list(c["best_dist"]) == list(range(1, cases.CHAIN + 1)) and (c["state"] == 0).all()
    assert (cases.ref("chain_40", ignore_claims=True)["best_idx"] == 0).all()
    # the float32 product: the same distances fail the test when the product is formed in float64
    p = cases.cases()["float32_product"]
    assert np.float32(9) > np.float64(np.float32(p.nn_ratio)) * 10 and not (np.float32(9) > np.float32(p.nn_ratio) * np.float32(10))


def test_border_z_zero_and_empty_cases():
    assert list(cases.ref("border_local")["state"]) == [0, 0, 7, 0, 0, 7] and list(cases.ref("border_local")["best_idx"]) == [0, 1, -1, 3, 5, -1]
    assert list(cases.ref("border_last")["state"]) == [0, 0, 4, 0, 0, 4] and list(cases.ref("border_last")["best_idx"]) == [0, 1, -1, 3, 5, -1]
    for n in ("border_all_local", "border_all_last"):
        assert cases.ref(n)["n_matches"] >= 4, n
    assert list(cases.ref("border_returns_local")["state"]) == [7] * 5 and list(cases.ref("border_returns_last")["state"]) == [4] * 5
    for dt in ("float32", "float64", "longdouble"):                           # exact in every dtype
        z = cases.ref("z_zero_local", dt)
        assert list(z["state"]) == [3] * 7 + [0] and not np.isfinite(np.asarray(z["uv"][:7], dtype=float)).any()
        assert np.isnan(float(z["uv"][0][0])) and float(z["uv"][1][0]) == np.inf                 # the NaN is the deviation
        z = cases.ref("z_zero_last", dt)
        assert list(z["state"]) == [3] * 7 + [0] and np.isnan(float(z["uv"][0][0])) and float(z["uv"][3][0]) == -np.inf
    for tag in ("last", "local"):
        e = cases.ref("empty_q_" + tag)
        assert e["state"].shape == (0,) and e["n_matches"] == 0 and (e["key_match"] == -1).all() and len(e["key_match"]) == 50
        k = cases.ref("empty_keys_" + tag)
        assert (k["best_idx"] == -1).all() and k["n_matches"] == 0 and len(k["key_match"]) == 0 and ((k["state"] == (4 if tag == "last" else 7)).sum() > 10)


def test_generator_and_shapes():
    p = cases.cases()["synth_mid_local"]
    assert (p.n_keys, p.n_q, p.n_levels, p.grid_cols, p.grid_rows) == (1000, 600, 8, 64, 48)
    q = cases.cases()["synth_small_last"]
    assert (q.n_keys, q.n_q) == (200, 120) and q.th == 15.0 and p.th == 1.0
    for a in (p.uv, p.q_pos, p.q_normal, p.q_dist_min, p.q_dist_max, p.q_pred_max, p.Rcw, p.tcw, p.Ow, p.K, p.scale, q.uv, q.q_pos):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))        # everything went through float32
    assert p.cell_begin[0] == 0 and p.cell_begin[-1] == len(p.cell_feat) <= p.n_keys and len(set(p.cell_feat)) == len(p.cell_feat)
    assert 0 < p.occupied.sum() < 200 and 0 < (p.q_blocks == 0).sum() < 120 and (q.angle < 360).all() and (q.q_angle < 360).all()
    assert [cases.cases()["queries_%d" % n].n_q for n in (255, 256, 257, 513)] == [255, 256, 257, 513]
    assert cases.cases()["max_keys"].n_keys == abi.SEARCH_PROJ_MAX_KEYS and cases.ref("max_keys")["n_matches"] > 20
    # the orientation filter drops matches, and more than the three kept bins are filled
    r = cases.ref("synth_mid_last")
    assert r["n_before_filter"] > r["n_matches"] > 100 and (r["hist"] > 0).sum() > 3 and (r["key_match"] == -2).sum() > 5
    assert cases.ref("no_orientation")["n_matches"] == cases.ref("synth_small_last")["n_before_filter"]


def conflict_pass(p, want):
    """the kernel's fixed-point iteration in Python, on the candidate lists of the yardstick: rounds of (every open query walks against
    the claim table of the round before; the table is rebuilt with a min) until a round changes no blocking claim.  Returns best_idx,
    state and the number of rounds"""
    T = np.float64
    fp = ref_mod._Fp()
    uvT = p.uv.astype(T)
    cand = {}
    for i in range(p.n_q):
        if want["state"][i] in ((0, 4, 5, 6) if not p.local else (0, 7, 8, 9)):
            u, v = want["uv"][i]
            if p.local:
                lv = int(want["level"][i])
                r = (2.5 if want["view_cos"][i] > 0.998 else 4.0)
                r = (r * p.th if p.th != 1.0 else r) * p.scale[lv]
                lo, hi = lv - 1, lv
            else:
                o = int(p.q_oct[i])
                r, lo, hi = p.th * p.scale[o], o - 1, o + 1
            cand[i] = ref_mod.features_in_area(p, fp, T, uvT, u, v, r, lo, hi)
    base = np.where(p.occupied != 0, -1, 2 ** 31 - 1).astype(np.int64)
    claim, prev = base.copy(), {i: -1 for i in cand}
    best_idx = np.full(p.n_q, -1)
    state = np.asarray(want["state"]).copy()
    for rnd in range(p.n_q + 1):
        changed = False
        for i, c in cand.items():
            if i < rnd:
                continue
            bd = bd2 = 256
            bl = bl2 = bi = -1
            for idx in c:
                if claim[idx] < i:
                    continue
                d = ref_mod.descriptor_distance(p.q_desc[i], p.desc[idx])
                if d < bd:
                    bd2, bd, bl2, bl, bi = bd, d, bl, int(p.oct[idx]), idx
                elif d < bd2:
                    bl2, bd2 = int(p.oct[idx]), d
            if not c:
                st = 7 if p.local else 4
            elif not (bd <= p.th_high and bi >= 0):
                st = 8 if p.local else 5
            elif p.local and bl == bl2 and np.float32(bd) > np.float32(p.nn_ratio) * np.float32(bd2):
                st = 9
            else:
                st = 0
            now = bi if (st == 0 and p.q_blocks[i]) else -1
            changed |= now != prev[i]
            prev[i], best_idx[i], state[i] = now, bi, st
        if not changed:
            return best_idx, state, rnd + 1
        claim = base.copy()
        for i, k in prev.items():
            if k >= 0:
                claim[k] = min(claim[k], i)
    raise AssertionError("the conflict pass did not stop")


@pytest.mark.parametrize("name", ["chain_40", "overwrite", "ratio_blocked", "crowd_last", "crowd_local", "crowd2_last", "crowd2_local", "synth_mid_last"])
def test_conflict_pass_prototype_equals_the_sequential_loop(name):
    p, want = cases.cases()[name], cases.ref(name)
    best_idx, state, rounds = conflict_pass(p, want)
    seq_state = np.where(want["state"] == 6, 0, want["state"]) if not p.local else want["state"]     # state 6 is the filter's, behind the pass
    assert np.array_equal(best_idx, want["best_idx"]) and np.array_equal(state, seq_state)
    print("%s: %d rounds for %d queries" % (name, rounds, p.n_q))
    assert 1 <= rounds <= p.n_q + 1 and (name != "chain_40" or rounds == cases.CHAIN + 1)
