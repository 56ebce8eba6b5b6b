"""The yardstick of vba_fuse (tests/fuse_ref.py) against itself (CPU only): the three dtypes, the margins of every floating-point
comparison and rounding it evaluates, the two forms of the candidate loop, known answers."""
import math

import numpy as np
import pytest

import fuse_cases as cases
import fuse_ref as ref_mod

NAMES = list(cases.cases())
MARGIN = 1e-9       # tests/test_gpu_fuse.py demands equality with nothing excused because of this


@pytest.mark.parametrize("name", NAMES)
def test_float64_equals_longdouble(name):
    assert ref_mod.differences(cases.ref(name), cases.ref(name, "longdouble")) == []


@pytest.mark.parametrize("name", NAMES)
def test_min_form_equals_sequential_form(name):
    a, b = cases.ref(name), cases.ref(name, form="min")
    assert ref_mod.differences(a, b) == [] and ref_mod.uv_difference(a, b) == 0.0


def test_every_comparison_and_rounding_has_a_margin():
    """every evaluated <, > or >= lies at least MARGIN relative from its threshold and every floor or ceil argument at least MARGIN from
    an integer, in float64 and in longdouble"""
    worst = min((cases.ref(n, dt)["margin"], n) for n in NAMES for dt in ("float64", "longdouble"))
    worst_r = min((cases.ref(n, dt)["margin_r"], n) for n in NAMES for dt in ("float64", "longdouble"))
    n_fp, n_round = sum(cases.ref(n)["n_fp"] for n in NAMES), sum(cases.ref(n)["n_round"] for n in NAMES)
    print("comparisons %d  smallest margin %.3e (%s)   roundings %d  smallest margin %.3e (%s)" % ((n_fp,) + worst + (n_round,) + worst_r))
    assert n_fp > 10000 and n_round > 2000 and worst[0] >= MARGIN and worst_r[0] >= MARGIN


def test_uv_tolerance_comes_from_longdouble():
    """the uv tolerance of the GPU test is ten times the largest float64-against-longdouble difference, rounded up to one digit"""
    worst = max(ref_mod.uv_difference(cases.ref(n), cases.ref(n, "longdouble")) for n in NAMES)
    print("largest |uv| difference float64 against longdouble: %.3e pixels; tolerance %.0e" % (worst, cases.UV_TOL))
    assert 0 < worst <= cases.UV_LONGDOUBLE
    e = 10 ** math.floor(math.log10(10 * cases.UV_LONGDOUBLE))
    assert cases.UV_TOL == pytest.approx(math.ceil(10 * cases.UV_LONGDOUBLE / e) * e, rel=1e-12)


def test_states_and_counts():
    """over all cases at least 500 points are found and every state occurs"""
    st = np.concatenate([cases.ref(n)["state"] for n in NAMES])
    count = np.bincount(st, minlength=9)
    print("points per state 0 .. 8:", count.tolist())
    assert count[0] >= 500 and (count > 0).all() and len(count) == 9
    assert sum(cases.ref(n)["n_found"] for n in NAMES) == count[0]


def test_print_float32_against_float64():
    """how many points move when everything runs in float32, as the reference computes it (recorded in DESIGN.md, not asserted)"""
    moved = pts = 0
    for n in NAMES:
        if n == "z_zero":
            continue
        a, b = cases.ref(n), cases.ref(n, "float32")
        moved += int(((a["state"] != b["state"]) | (a["best_idx"] != b["best_idx"])).sum())
        pts += len(a["state"])
    print("float32 against float64: %d of %d points change their state or best_idx" % (moved, pts))


def test_hand_made_answers():
    r = cases.ref("micro")
    for i, (state, idx, dist, level, uv) in cases.micro_expect().items():
        assert (r["state"][i], r["best_idx"][i], r["best_dist"][i], r["level"][i]) == (state, idx, dist, level), i
        if uv is None:
            assert np.isnan(r["uv"][i]).all(), i
        else:
            assert np.abs(r["uv"][i] - uv).max() < 1e-9, i
    assert sorted(r["state"]) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 8] and r["n_found"] == 1
    t = cases.ref("tie_cells")
    assert list(t["state"]) == [0, 0] and list(t["best_idx"]) == [7, 5] and list(t["best_dist"]) == [8, 6]
    p = cases.cases()["tie_cells"]
    f = list(p.cell_feat)
    assert f.index(5) + 1 == f.index(3) and f.index(7) < f.index(2)           # one cell lists 5 in front of 3; 7 sits in an earlier column
    for dt in ("float32", "float64", "longdouble"):                           # exact in every dtype
        z = cases.ref("z_zero", dt)
        assert list(z["state"]) == [3] * 7 + [0] and not np.isfinite(np.asarray(z["uv"][:7], dtype=float)).any()
        assert np.isnan(float(z["uv"][0][0])) and float(z["uv"][1][0]) == np.inf and np.isnan(float(z["uv"][1][1])) and float(z["uv"][3][0]) == -np.inf
        assert float(z["uv"][5][0]) == -np.inf and float(z["uv"][5][1]) == -np.inf   # z = -0.0 + tcw[2] is +0.0
    e = cases.ref("level_edges")
    assert list(e["state"]) == [6, 0, 0, 6, 0, 8, 0, 0, 8] and list(e["level"]) == [-1, 0, 3, 4, 2, 0, 1, 2, 3]
    assert list(e["best_idx"]) == [-1, 0, 1, -1, 4, -1, 7, 7, -1] and list(e["best_dist"][[2, 4, 6]]) == [7, 10, 3]


def test_border_cases():
    b = cases.ref("border")
    assert list(b["state"]) == [0, 0, 7, 0, 0, 7] and list(b["best_idx"]) == [0, 1, -1, 3, 5, -1]
    a = cases.ref("border_all")                                               # every keypoint of a cell is in the area; the level gate still holds
    assert set(a["state"]) == {0, 8} and a["n_found"] >= 4
    assert list(cases.ref("border_returns")["state"]) == [7, 7, 7, 7, 7]


@pytest.mark.parametrize("name, x_empty", [("rows_empty", False), ("cols_empty", True)])
def test_negative_radius_empties_one_axis(name, x_empty):
    """every point of the case passes the gates and the four returns of GetFeaturesInArea; its clamped cell range holds columns and
    no row (rows_empty) or rows and no column (cols_empty); the yardstick leaves with state 7"""
    p, r = cases.cases()[name], cases.ref(name)
    assert list(r["state"]) == [7] * p.n_pt and list(r["level"]) == [0] * p.n_pt and p.n_pt >= 4
    fp = ref_mod._Fp()
    for i in range(p.n_pt):
        cells = ref_mod.cell_range(p, fp, np.float64, r["uv"][i, 0], r["uv"][i, 1], np.float64(p.th) * np.float64(p.scale[0]))
        print(name, "point", i, "uv", r["uv"][i], "cells x %s .. %s  y %s .. %s" % (cells or (None,) * 4))
        assert cells is not None
        nx0, nx1, ny0, ny1 = cells
        assert (nx1 < nx0 and ny0 <= ny1) if x_empty else (nx0 <= nx1 and ny1 < ny0), (i, cells)
    assert fp.n_round == 4 * p.n_pt and fp.margin_r >= MARGIN


def test_reproj_and_empty_cases():
    on, off = cases.ref("reproj_on"), cases.ref("reproj_off")
    moved = (on["state"] != off["state"]) | (on["best_idx"] != off["best_idx"])
    assert moved.sum() >= 5 and off["n_found"] > on["n_found"]
    assert np.array_equal(on["level"], off["level"]) and set(on["state"][moved]) == {8}
    assert cases.ref("empty_pt")["state"].shape == (0,) and cases.ref("empty_pt")["n_found"] == 0
    k = cases.ref("empty_keys")
    assert set(k["state"]) <= {1, 2, 3, 4, 5, 6, 7} and (k["state"] == 7).sum() > 10 and (k["best_idx"] == -1).all()
    s = cases.ref("all_skipped")
    assert set(s["state"]) == {1} and np.isnan(s["uv"]).all() and (s["level"] == -128).all() and (s["best_dist"] == 256).all()


def test_generator():
    from mc_slam_amd import synth
    p = cases.cases()["synth_mid"]
    assert (p.n_keys, p.n_pt, p.n_levels, p.grid_cols, p.grid_rows) == (1000, 600, 8, 64, 48)
    for a in (p.uv, p.pos, p.normal, p.dist_min, p.dist_max, p.pred_max, p.Rcw, p.tcw, p.Ow, p.K, p.scale, p.inv_level_sigma2):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))        # everything went through float32
    assert p.cell_begin[0] == 0 and p.cell_begin[-1] == len(p.cell_feat) <= p.n_keys and len(set(p.cell_feat)) == len(p.cell_feat)
    kind, key = p.truth["kind"], p.truth["key"]
    r = cases.ref("synth_mid")
    m = kind == synth.FUSE_KINDS.index("match")
    assert (r["best_idx"][m & (r["state"] == 0)] == key[m & (r["state"] == 0)]).mean() > 0.98 and (r["state"][m] == 0).mean() > 0.8
    d = np.unpackbits(p.pt_desc[m] ^ p.desc[key[m]], axis=1).sum(axis=1)
    assert (d == 12).all()
    for name, st in (("skip", 1), ("behind", 2), ("outside", 3), ("distance", 4), ("angle", 5), ("level_high", 6)):
        assert (r["state"][kind == synth.FUSE_KINDS.index(name)] == st).all(), name
    assert len(set(cases.cases()["tiles_513"].truth["key"])) < 450              # a keypoint matched by two points of one call
