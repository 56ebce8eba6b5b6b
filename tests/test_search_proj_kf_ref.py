"""The yardstick of vba_search_by_projection_kf (tests/search_proj_kf_ref.py, the sequential loop) against itself (CPU only): the three
dtypes, the margins of every floating-point comparison and rounding it evaluates, known answers, how much the queries depend on each
other, and a Python prototype of the kernel's conflict pass against the sequential loop."""
import math

import numpy as np
import pytest

import search_proj_kf_cases as cases
import search_proj_kf_ref as ref_mod
from mc_slam_amd import abi

NAMES = list(cases.cases())
MARGIN = 1e-9       # tests/test_gpu_search_proj_kf.py demands equality with nothing excused because of this


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


def test_tolerance_comes_from_longdouble():
    """the uv tolerance of the GPU test is ten times the largest float64-against-longdouble difference, rounded up to one digit"""
    worst = max(ref_mod.real_difference(cases.ref(n), cases.ref(n, "longdouble"), "uv") for n in NAMES)
    print("largest |uv| difference float64 against longdouble: %.3e pixels; tolerance %.0e" % (worst, cases.UV_TOL))
    assert 0 < worst <= cases.UV_LONGDOUBLE
    e = 10 ** math.floor(math.log10(10 * cases.UV_LONGDOUBLE))
    assert cases.UV_TOL == pytest.approx(math.ceil(10 * cases.UV_LONGDOUBLE / e) * e, rel=1e-12)


def test_states_and_counts():
    """over all cases every state of either mode occurs and at least 500 queries match"""
    total = 0
    for mode, n_states in ((cases.LOOP, 9), (cases.RELOC, 8)):
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
    r = cases.ref("micro_loop")
    expect, totals = cases.micro_expect(cases.LOOP)
    for i, (state, idx, dist, level, uv) in expect.items():
        assert (r["state"][i], r["best_idx"][i], r["best_dist"][i], r["level"][i]) == (state, idx, dist, level), i
        _check_uv(r, i, uv)
    assert sorted(r["state"]) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 8] and (r["bin"] == 255).all()
    for k, v in totals.items():
        assert np.array_equal(np.asarray(r[k]), np.asarray(v)), k
    r = cases.ref("micro_reloc")
    expect, totals = cases.micro_expect(cases.RELOC)
    for i, (state, idx, dist, level, b, uv) in expect.items():
        assert (r["state"][i], r["best_idx"][i], r["best_dist"][i], r["level"][i], r["bin"][i]) == (state, idx, dist, level, b), i
        _check_uv(r, i, uv)
    assert sorted(r["state"]) == [0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7]
    for k, v in totals.items():
        assert np.array_equal(np.asarray(r[k]), np.asarray(v)), k


def test_hand_made_dependency_cases():
    for name, want in cases.hand_expect().items():
        r = cases.ref(name)
        for k, v in want.items():
            assert np.array_equal(np.asarray(r[k]), np.asarray(v)), (name, k, r[k], v)
    for name in ("chain_40", "chain_40_reloc"):
        c = cases.ref(name)
        assert list(c["best_idx"]) == list(range(cases.CHAIN)) and list(c["best_dist"]) == list(range(1, cases.CHAIN + 1)) and (c["state"] == 0).all()
        assert (cases.ref(name, ignore_claims=True)["best_idx"] == 0).all()
    # the point of behind_reloc lies behind the camera and projects inside the bounds
    p = cases.cases()["behind_reloc"]
    assert p.q_pos[0, 2] == -4.0 and np.abs(cases.ref("behind_reloc")["uv"][0] - (20.5, 20.5)).max() < 1e-9


def test_border_z_zero_and_empty_cases():
    assert list(cases.ref("border_loop")["state"]) == [0, 0, 7, 0, 0, 7] and list(cases.ref("border_loop")["best_idx"]) == [0, 1, -1, 3, 5, -1]
    assert list(cases.ref("border_reloc")["state"]) == [0, 0, 5, 0, 0, 5] and list(cases.ref("border_reloc")["best_idx"]) == [0, 1, -1, 3, 5, -1]
    for n in ("border_all_loop", "border_all_reloc"):
        assert cases.ref(n)["n_matches"] >= 4, n
    assert list(cases.ref("border_returns_loop")["state"]) == [7] * 5 and list(cases.ref("border_returns_reloc")["state"]) == [5] * 5
    for dt in ("float32", "float64", "longdouble"):                           # exact in every dtype
        z = cases.ref("z_zero_loop", dt)
        assert list(z["state"]) == [3] * 7 + [0] and not np.isfinite(np.asarray(z["uv"][:7], dtype=float)).any()
        assert np.isnan(float(z["uv"][0][0])) and float(z["uv"][1][0]) == np.inf
        z = cases.ref("z_zero_reloc", dt)
        assert list(z["state"]) == [2] * 7 + [0] and np.isnan(float(z["uv"][0][0])) and float(z["uv"][3][0]) == -np.inf   # the NaN is the deviation
    for tag, empty in (("loop", 7), ("reloc", 5)):
        e = cases.ref("empty_q_" + tag)
        assert e["state"].shape == (0,) and e["n_matches"] == 0 and (e["key_match"] == -1).all() and len(e["key_match"]) == 50
        k = cases.ref("empty_keys_" + tag)
        assert (k["best_idx"] == -1).all() and k["n_matches"] == 0 and len(k["key_match"]) == 0 and ((k["state"] == empty).sum() > 10)


def test_generator_and_shapes():
    p = cases.cases()["synth_mid_loop"]
    assert (p.n_keys, p.n_q, p.n_levels, p.grid_cols, p.grid_rows) == (1000, 600, 8, 64, 48) and (p.th, p.th_dist) == (10.0, 50)
    q = cases.cases()["synth_small_reloc"]
    assert (q.n_keys, q.n_q) == (200, 120) and (q.th, q.th_dist) == (10.0, 100)
    for a in (p.uv, p.q_pos, p.q_normal, p.q_dist_min, p.q_dist_max, p.q_pred_max, p.Rcw, p.tcw, p.Ow, p.K, p.scale, q.uv, q.q_pos):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))        # everything went through float32
    assert p.cell_begin[0] == 0 and p.cell_begin[-1] == len(p.cell_feat) <= p.n_keys and len(set(p.cell_feat)) == len(p.cell_feat)
    assert 0 < p.occupied.sum() < 200 and (q.angle < 360).all() and (q.q_angle < 360).all()
    assert [cases.cases()["queries_%d" % n].n_q for n in (255, 256, 257, 513)] == [255, 256, 257, 513]
    assert cases.cases()["max_keys"].n_keys == abi.SEARCH_PROJ_KF_MAX_KEYS and cases.ref("max_keys")["n_matches"] > 20
    cr = cases.cases()["crowd_loop"]
    assert (cr.n_keys, cr.n_q) == (120, 400)
    # points behind the camera match in reloc mode
    m = cases.cases()["synth_mid_reloc"]
    r = cases.ref("synth_mid_reloc")
    behind = m.truth["behind"]
    zc = (m.q_pos @ m.Rcw.T + m.tcw)[:, 2]
    assert behind.sum() > 10 and (zc[behind] < 0).all() and (np.isin(r["state"][behind], (0, 7))).sum() > 5
    # the orientation filter drops matches, and more than the three kept bins are filled
    assert r["n_before_filter"] > r["n_matches"] > 100 and (r["hist"] > 0).sum() > 3 and (r["key_match"] == -2).sum() > 5
    assert cases.ref("no_orientation")["n_matches"] == cases.ref("synth_small_reloc")["n_before_filter"]


@pytest.mark.parametrize("name", ["chain_40", "chain_40_reloc", "crowd_loop", "crowd_reloc", "synth_mid_loop", "synth_mid_reloc", "all_taken_loop", "levels_reloc"])
def test_conflict_pass_prototype_equals_the_sequential_loop(name):
    p, want = cases.cases()[name], cases.ref(name)
    got = ref_mod.conflict_pass(p)
    assert ref_mod.differences(got, want) == []
    print("%s: %d rounds for %d queries" % (name, got["rounds"], p.n_q))
    assert 1 <= got["rounds"] <= p.n_q + 1 and (not name.startswith("chain_40") or got["rounds"] == cases.CHAIN + 1)
