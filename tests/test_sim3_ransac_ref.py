"""CPU checks of the vba_sim3_ransac yardstick (tests/sim3_ransac_ref.py) and of the conditions the GPU comparison rests on, for
every case of tests/sim3_ransac_cases.py and EVERY hypothesis of it (no hypothesis is excused: the share left out is zero)."""
import numpy as np
import pytest

import sim3_ransac_cases as cases
import sim3_ransac_ref as ref

GAP_MIN = 1e-4      # (lambda1 - lambda2) / |lambda1|: the dominant eigenvector is determined to ~ eps / gap
MARGIN_MIN = 1e-6   # |err / gate - 1| of the closest pair: 1e-6 is ~ 1e9 ulp, no rounding difference between two FP64 routes flips a flag


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_conditions_hold_for_every_hypothesis(case):
    r = cases.reference(case)
    assert r["gap"].shape == (case[5],)
    print("case", case, "smallest gap %.2e" % r["gap"].min(), "smallest margin %.2e" % r["margin"].min())
    assert (r["gap"] >= GAP_MIN).all(), (np.argmin(r["gap"]), r["gap"].min())
    assert (r["margin"] >= MARGIN_MIN).all(), (np.argmin(r["margin"]), r["margin"].min())


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_float64_and_longdouble_flags_identical(case):
    r, rl = cases.reference(case), cases.reference(case, "longdouble")
    assert (r["flags"] == rl["flags"]).all()
    assert (r["hyp_inliers"] == rl["hyp_inliers"]).all()
    for k in ("hit", "its_done", "best_hyp", "best_inliers", "n_inliers"):
        assert r[k] == rl[k], k


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_jacobi_against_eigh(case):
    """the dominant eigenpair of Horn's N against np.linalg.eigh to 1e-13: the eigenvalue relative to |lambda1|, the eigenvector
    scaled by the gap (an eigenvector is determined to eps / gap, so that product is what 1e-13 can be asked of), and the
    residual |N v - lambda v| / |lambda1|"""
    h = cases.reference(case)["hyp"]
    N, lam, V = h["N"], h["lam"], h["V"]
    w, U = np.linalg.eigh(N)
    k = np.argmax(lam, axis=1)
    idx = np.arange(len(N))
    l1, v1 = lam[idx, k], V[idx, :, k]
    u1 = U[:, :, 3]
    sgn = np.sign(np.einsum("hi,hi->h", v1, u1))
    gap = (w[:, 3] - w[:, 2]) / np.abs(w[:, 3])
    assert (np.abs(l1 - w[:, 3]) <= 1e-13 * np.abs(w[:, 3])).all()
    assert (np.abs(v1 - sgn[:, None] * u1).max(axis=1) * gap <= 1e-13).all()
    res = np.abs(np.einsum("hab,hb->ha", N, v1) - l1[:, None] * v1).max(axis=1)
    assert (res <= 1e-13 * np.abs(l1)).all()
    # all four eigenvalues, sorted
    assert (np.abs(np.sort(lam, axis=1) - w) <= 1e-13 * np.abs(w[:, 3:4])).all()


def test_the_cases_cover_what_they_are_there_for():
    kinds = set()
    for case in cases.CASES:
        r = cases.reference(case)
        n_hyp, min_in = case[5], case[6]
        if r["hit"] == 0:
            kinds.add("hit at 0")
        if r["hit"] >= 40:
            kinds.add("late hit")
        if r["hit"] < 0:
            kinds.add("no hit")
            if r["hyp_inliers"].max() == min_in:
                kinds.add("max c == min_inliers")
            if n_hyp > 256:
                kinds.add("no hit past lane 256")
    assert kinds == {"hit at 0", "late hit", "no hit", "max c == min_inliers", "no hit past lane 256"}, kinds
    assert {c[1] for c in cases.CASES} == {3, 25, 63, 64, 65, 120, 400}
    assert {c[5] for c in cases.CASES} == {1, 5, 64, 257, 300}
    assert {c[2] for c in cases.CASES} == {0, 1}


def test_scan_rules():
    # a tie replaces the best (>=), and the scan goes on when the count is no hit
    assert ref.scan([5, 7, 7, 3], 20, 0) == (-1, 4, 2, 7)
    # c == min_inliers is no hit (strict >); one more is
    assert ref.scan([20, 20], 20, 0) == (-1, 2, 1, 20)
    assert ref.scan([20, 21, 30], 20, 0) == (1, 2, 1, 21)
    # the incoming best blocks smaller counts, hit-sized ones included; equal ones pass
    assert ref.scan([25, 29], 20, 30) == (-1, 2, -1, 30)
    assert ref.scan([25, 30, 31], 20, 30) == (1, 2, 1, 30)
    # zero counts of a fresh solver are accepted (0 >= 0): best_hyp moves, nothing else
    assert ref.scan([0, 0], 20, 0) == (-1, 2, 1, 0)
    assert ref.scan([], 20, 4) == (-1, 0, -1, 4)


def test_degenerate_triples_in_the_yardstick():
    p = cases.make(cases.CASES[6])
    c, _, _, _ = ref.counts(p.copy(fix_scale=0), [[5, 5, 5]])
    assert c[0] == 0                      # 0/0 in the scale: NaN fails every `<`
    c, _, _, _ = ref.counts(p, [[5, 5, 9], [5, 9, 5]])
    assert ((c >= 0) & (c <= p.n_pairs)).all()


def test_print_float64_against_longdouble():
    """the figures the tolerances of tests/test_gpu_sim3_ransac.py derive from (printed, -s shows them): the largest difference of
    (t, q, s) between the float64 and the longdouble yardstick over all hypotheses of all cases"""
    dt = dq = ds = 0.0
    for case in cases.CASES:
        h, hl = cases.reference(case)["hyp"], cases.reference(case, "longdouble")["hyp"]
        dt = max(dt, float(np.abs(h["t"] - hl["t"]).max()))
        dq = max(dq, float(np.abs(h["q"] - hl["q"]).max()))
        ds = max(ds, float(np.abs(h["s"] - hl["s"]).max()))
    print("float64 against longdouble over all hypotheses of all cases: |dt| %.3e  |dq| %.3e  |ds| %.3e" % (dt, dq, ds))
    assert np.isfinite([dt, dq, ds]).all()


def test_print_float32_deviation():
    """how many counts and which hits change when the yardstick computes as the reference does, in float32 (printed for DESIGN.md
    section 8, row f-7; not asserted: it is the size of a recorded deviation, not a requirement)"""
    n_c = n_tot = 0
    hits = []
    worst = 0
    for case in cases.CASES:
        r, r32 = cases.reference(case), cases.reference(case, "float32")
        d = r["hyp_inliers"].astype(int) - r32["hyp_inliers"].astype(int)
        n_c += int((d != 0).sum())
        n_tot += len(d)
        worst = max(worst, int(np.abs(d).max()))
        if r["hit"] != r32["hit"]:
            hits.append((case, r["hit"], r32["hit"]))
    print("float32 against float64: %d of %d counts differ (largest difference %d); hits that change: %s" % (n_c, n_tot, worst, hits))
