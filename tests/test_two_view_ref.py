"""The yardstick of vba_two_view_init (tests/two_view_ref.py) against itself, on the CPU: that every case of tests/two_view_cases.py
ends the way it is there for, that every comparison the yardstick evaluates keeps a margin (so that the GPU comparison excuses
nothing), how far float64 is from longdouble (the GPU tolerances are ten times these figures) and float32 from float64 (the
documented FP64-vs-CV_32F difference), that the sign convention of the SVDs does not reach the answer, and a known answer."""
import numpy as np
import pytest

import two_view_cases as cases
import two_view_ref as ref
from mc_slam_amd import synth

MIN_GAP = 1e-6        # relative gap between the two smallest singular values of every 9-column A
MIN_MARGIN = 1e-9     # distance of every evaluated comparison from its threshold


def unit(M):
    """a matrix up to scale and sign: Frobenius norm 1, the largest-magnitude entry positive"""
    M = np.asarray(M, dtype=np.longdouble)
    n = np.sqrt((M * M).sum())
    if n == 0:
        return M
    M = M / n
    return M * np.sign(M.ravel()[np.argmax(np.abs(M))])


def differences(a, b):
    """name -> the largest difference between two answers of the yardstick (or of the library) in the quantities the GPU test
    compares within a tolerance; scores relative, matrices up to scale and sign, points relative to their distance from the origin"""
    L = lambda x: np.asarray(x, dtype=np.longdouble)
    d = {}
    rel = lambda x, y: float(np.max(np.abs(L(x) - L(y)) / np.maximum(np.abs(L(y)), 1), initial=0))
    d["hyp_score"] = max(rel(a["hyp_score_h"], b["hyp_score_h"]), rel(a["hyp_score_f"], b["hyp_score_f"]))
    d["score"] = max(rel(a["score_h"], b["score_h"]), rel(a["score_f"], b["score_f"]))
    d["rh"] = 0.0 if np.isnan(float(b["rh"])) else float(abs(L(a["rh"]) - L(b["rh"])))
    d["HF"] = float(max(np.abs(unit(a["H21"]) - unit(b["H21"])).max(), np.abs(unit(a["F21"]) - unit(b["F21"])).max()))
    d["parallax"] = float(np.abs(L(a["rt_parallax"]) - L(b["rt_parallax"])).max())
    if b["ok"] and a["ok"]:
        d["pose"] = float(max(np.abs(L(a["R21"]) - L(b["R21"])).max(), np.abs(L(a["t21"]) - L(b["t21"])).max()))   # [R21 | t21], one quantity
        nz = np.linalg.norm(np.asarray(b["x3d"], dtype=np.float64), axis=1) > 0
        if nz.any():
            d["x3d"] = float((np.linalg.norm((L(a["x3d"]) - L(b["x3d"]))[nz].astype(np.float64), axis=1) / np.linalg.norm(np.asarray(b["x3d"], dtype=np.float64)[nz], axis=1)).max())
    return d


def decisions(r):
    return (r["ok"], r["model"], r["reason"], r["best_hyp_h"], r["best_hyp_f"], r["n_inliers_h"], r["n_inliers_f"], r["n_rt"], r["best_rt"],
            tuple(int(g) for g in r["rt_good"]), r["inlier_h"].tobytes(), r["inlier_f"].tobytes(), None if r["triangulated"] is None else r["triangulated"].tobytes())


@pytest.mark.parametrize("name", cases.IDS)
def test_case_ends_as_intended_with_margins(name):
    r = cases.reference(name)
    p = cases.make(name)
    assert (r["ok"], r["model"], r["reason"]) == cases.NAMES[name][3]
    assert p.n_keys1 > p.n_matches and p.n_keys2 > p.n_matches
    for g in (r["gap_h"], r["gap_f"]):
        assert g.size == p.n_hyp and (g.size == 0 or g.min() >= MIN_GAP), g.min()
    small = {k: v for k, v in r["margins"].items() if not v >= MIN_MARGIN}
    assert not small, small


def test_the_cases_cover_what_they_are_for():
    R = {n: cases.reference(n) for n in cases.IDS}
    assert {r["reason"] for r in R.values()} == {0, 1, 2, 3, 4, 5}
    assert {(r["model"], r["ok"]) for r in R.values()} >= {(1, 1), (2, 1)}
    assert {cases.make(n).n_matches for n in cases.IDS} >= {8, 9, 63, 64, 65, 255, 256, 257, 300}
    assert {cases.make(n).n_hyp for n in cases.IDS} >= {0, 1, 15, 16, 17, 200}
    good = [int(g) for r in R.values() for g in r["rt_good"][:r["n_rt"]] if g > 0]
    assert min(good) < 51 < max(good)                                      # both arms of min(50, size - 1)
    win = [r["rt"][r["best_rt"]] for r in R.values() if r["ok"]]
    assert any(0 < w["n_good"] < 51 for w in win) and any(w["n_good"] > 51 for w in win)
    assert sum(int((w["state"] == 1).sum()) for w in win) >= 50            # counted in nGood, cos >= 0.99998: not flagged
    r = R["wrong30-300x200"]
    wrong = cases.make("wrong30-300x200").truth["wrong"]
    assert 0.2 < wrong.mean() < 0.4 and r["ok"] == 1 and not r["inlier_f"][wrong].all()


def test_print_float64_against_longdouble():
    """the figures the GPU tolerances are derived from (tests/test_gpu_two_view.py)"""
    worst = {}
    for n in cases.IDS:
        a, b = cases.reference(n), cases.reference(n, "longdouble")
        assert decisions(a) == decisions(b), n
        for k, v in differences(a, b).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("float64 against longdouble, largest over all cases:", {k: "%.3e" % v for k, v in worst.items()})
    assert set(worst) == {"hyp_score", "score", "rh", "HF", "parallax", "pose", "x3d"}


def test_print_float32_against_float64():
    """what CV_32F arithmetic changes: which decisions move, and by how much the figures do"""
    moved, worst = [], {}
    for n in cases.IDS:
        a, b = cases.reference(n, "float32"), cases.reference(n)
        if (a["ok"], a["model"], a["reason"]) != (b["ok"], b["model"], b["reason"]):
            moved.append((n, (a["ok"], a["model"], a["reason"]), (b["ok"], b["model"], b["reason"])))
        for k, v in differences(a, b).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("float32 against float64: (ok, model, reason) moved in", moved, "largest differences", {k: "%.3e" % v for k, v in worst.items()})


@pytest.mark.parametrize("name", cases.IDS)
def test_the_sign_convention_does_not_reach_the_answer(name):
    a, b = cases.reference(name), cases.reference(name, "float64", True)
    assert (a["ok"], a["reason"], a["model"]) == (b["ok"], b["reason"], b["model"])
    assert sorted(a["rt_good"].tolist()) == sorted(b["rt_good"].tolist())
    if a["ok"]:
        assert np.array_equal(a["triangulated"], b["triangulated"])
        d = differences(b, a)
        assert d["pose"] <= 1e-12 and d.get("x3d", 0.0) <= 1e-10, d
        if a["n_rt"] == 4:
            assert not np.array_equal(a["rt_good"], b["rt_good"]) or a["best_rt"] == b["best_rt"]


def test_the_flipped_convention_permutes_the_hypotheses():
    """somewhere among the cases the flip does move the winner to another index: the invariance above is not vacuous"""
    assert any(cases.reference(n)["ok"] and cases.reference(n)["best_rt"] != cases.reference(n, "float64", True)["best_rt"] for n in cases.IDS)


@pytest.mark.parametrize("kind,model,seed", [("general", 2, 11), ("plane", 1, 13)])
def test_known_answer_on_noise_free_pairs(kind, model, seed):
    p = synth.make_two_view(seed, 120, 16, kind, baseline=1.0, noise=0.0, float32=False)
    a, b = ref.two_view(p), ref.two_view(p, np.longdouble)
    assert a["ok"] == b["ok"] == 1 and a["model"] == b["model"] == model
    R, t = p.truth["R21"], p.truth["t21"]
    err = lambda r: max(float(np.abs(r["R21"] - R).max()), float(np.abs(r["t21"] - t).max()))
    agree = max(float(np.abs(a["R21"] - b["R21"]).max()), float(np.abs(a["t21"] - b["t21"]).max()))
    print(kind, "error against the generating motion: float64 %.2e longdouble %.2e, float64 against longdouble %.2e" % (err(a), err(b), agree))
    assert err(b) <= 1e-11
    assert err(a) <= 10 * agree + err(b)
