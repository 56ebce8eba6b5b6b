"""CPU checks of tests/sim3_ref.py, the NumPy restatement of Optimizer::OptimizeSim3 that the GPU tests use as their yardstick:
it has to be trustworthy before the GPU is compared with it."""
import os

import numpy as np
import pytest

import sim3_cases
import sim3_ref
from mc_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sim3_pairs.npz")


def _state(p):
    return p.S12[3:7].copy(), p.S12[:3].copy(), float(p.S12[7])


@pytest.mark.parametrize("fix", [False, True])
def test_analytic_jacobians_against_central_differences(fix):
    """step 1e-6: truncation O(h^2) and rounding eps / h are both below 1e-6 of the largest entry (the reference's own 1e-9 step
    is too noisy to test against)"""
    p = synth.make_sim3_pair(1, 40, fix_scale=fix)
    S = _state(p)
    _, _, y, z = sim3_ref.errors(S, p)
    Ja = sim3_ref.jac_analytic(S, p, y, z, fix)
    Jn = sim3_ref.jac_numeric(S, p, fix, step=1e-6)
    for a, n, name in ((Ja[0], Jn[0], "J12"), (Ja[1], Jn[1], "J21")):
        rel = np.abs(a - n).max() / np.abs(a).max()
        print(name, "max |analytic - numeric| / max |J| = %.2e (max |J| %.1f)" % (rel, np.abs(a).max()))
        assert rel <= 1e-6
    if fix:
        assert not Ja[0][:, :, 6].any() and not Ja[1][:, :, 6].any()


def _compose_identity(u):
    a, b = sim3_ref.sim3_exp(u), sim3_ref.sim3_exp(-np.asarray(u))
    q, t, s = sim3_ref.sim3_mul(a, b)
    return max(np.abs(sim3_ref.q2R(q) - np.eye(3)).max(), np.abs(t).max(), abs(s - 1.0))


def test_exp_takes_all_four_branches_and_inverts():
    """exp(d) exp(-d) = identity to 1e-12 in every branch.  The closed forms of sim3.h:92-118 are first-order inside |sigma| < 1e-5
    (C = 1 for (e^sigma - 1) / sigma, A and B without their sigma terms), so W(d) upsilon carries an error of about
    |sigma| |upsilon| / 2 there: the updates of those two branches have |sigma| |upsilon| <= 1e-13, as the steps of a converged LM
    have; the two |sigma| >= 1e-5 branches take a translation of ordinary size.  In the theta < 1e-5, |sigma| >= 1e-5 branch the reference's
    B = (sigma^2 / 2 - sigma + 1) e^sigma / sigma^3 lacks the -1 of the exact limit and is O(1 / sigma^3), so its term B W^2 upsilon is
    about theta^2 |upsilon| / sigma^3 (restated as it stands): that case takes theta = 1e-8, which keeps the term at 1e-14."""
    seen = set()
    for om, ups, sg in ((1e-7, 1e-6, 1e-7), (0.2, 1e-6, 1e-7), (1e-8, 1.0, 0.1), (0.2, 1.0, 0.1)):
        u = np.array([om, -0.5 * om, 0.3 * om, 0.1 * ups, -0.2 * ups, 0.05 * ups, sg])
        info = {}
        sim3_ref.sim3_exp(u, info)
        seen.add(info["branch"])
        print("branch", info["branch"], "|exp(d) exp(-d) - 1| = %.2e" % _compose_identity(u))
        assert _compose_identity(u) <= 1e-12, (om, sg, _compose_identity(u))
    assert seen == {0, 1, 2, 3}


def test_exp_is_continuous_across_both_eps_switches():
    """the closed forms on either side of theta = 1e-5 and of |sigma| = 1e-5 meet up to the terms the small branch drops:
    theta switch, |sigma| < eps -- R = I + W + W^2 against Rodrigues (W^2 / 2) and A, B = 1/2, 1/6: O(theta^2) = 1e-10;
    theta switch, |sigma| >= eps -- the small-theta B = (sigma^2 / 2 - sigma + 1) e^sigma / sigma^3 (O(1 / sigma^3): it lacks the -1 of the
    exact limit, restated as it stands) against the regular B = O(1): a jump of B eps^2 |upsilon| in t;
    sigma switch -- C = 1 against (e^sigma - 1) / sigma = 1 + sigma / 2: a jump of eps / 2 |upsilon| in t, nothing in R and s; for
    theta < eps the same B (1e15 at sigma = eps) adds theta^2 |upsilon| / eps^3, so that case takes theta = 1e-12."""
    d = np.array([0.6, 0.0, 0.8])                      # unit direction: theta = |omega| exactly controllable
    up = np.array([0.3, -0.2, 0.1])
    h = 1e-10
    for sg in (0.0, 0.05):                              # theta switch, in both sigma branches
        lo = sim3_ref.sim3_exp(np.concatenate([d * (1e-5 - h), up, [sg]]))
        hi = sim3_ref.sim3_exp(np.concatenate([d * (1e-5 + h), up, [sg]]))
        b_small = (0.5 * sg * sg - sg + 1) * np.exp(sg) / sg ** 3 if sg else 0.0
        bound = (b_small + 1.0) * 1e-10 * np.sqrt(up @ up) + 1e-9
        print("theta switch at sigma %g: |dt| %.2e (bound %.2e)" % (sg, np.abs(lo[1] - hi[1]).max(), bound))
        assert np.abs(lo[0] - hi[0]).max() <= 1e-9 and np.abs(lo[1] - hi[1]).max() <= bound and lo[2] == hi[2]
    jump = 0.5 * 1e-5 * np.sqrt(up @ up) * 1.01 + 1e-9
    for th in (1e-12, 0.3):                             # sigma switch, in both theta branches
        lo = sim3_ref.sim3_exp(np.concatenate([d * th, up, [1e-5 - h]]))
        hi = sim3_ref.sim3_exp(np.concatenate([d * th, up, [1e-5 + h]]))
        print("sigma switch at theta %g: |dt| %.2e (bound %.2e)" % (th, np.abs(lo[1] - hi[1]).max(), jump))
        assert np.abs(lo[0] - hi[0]).max() <= 1e-15 and np.abs(lo[1] - hi[1]).max() <= jump and abs(lo[2] - hi[2]) <= 1e-9


def _dist(S, T):
    dq = min(np.abs(S[3:7] - T[3:7]).max(), np.abs(S[3:7] + T[3:7]).max())
    return np.abs(S[:3] - T[:3]).max(), dq, abs(S[7] - T[7]) / T[7]


def test_noise_free_problem_recovers_the_truth():
    p = synth.make_sim3_pair(3, 80, outlier_frac=0.0, noise=False)
    r = sim3_ref.optimize(p)
    assert r.n_inliers == 80 and not r.outlier.any()
    dt, dq, ds = _dist(r.S12, p.truth["S12"])
    print("noise-free: |dt| %.2e |dq| %.2e |ds|/s %.2e" % (dt, dq, ds))
    assert max(dt, dq, ds) <= 1e-6


def test_fix_scale_returns_the_scale_bit_identical():
    p = synth.make_sim3_pair(4, 120, fix_scale=True)
    r = sim3_ref.optimize(p)
    assert r.n_inliers > 0
    assert r.S12[7].tobytes() == p.S12[7].tobytes()
    assert not np.array_equal(r.S12[:7], p.S12[:7])


def test_fewer_than_ten_good_pairs_returns_zero_and_keeps_S12():
    p = synth.make_sim3_pair(5, 16, outlier_frac=0.0)
    p.uv1[:9] += 60.0                                   # 9 gross outliers: at most 7 pairs can survive the first test
    r = sim3_ref.optimize(p)
    assert r.n_inliers == 0 and r.its_done[1] == 0
    assert r.S12.tobytes() == p.S12.tobytes()
    assert r.n_bad_stage1 >= 7 and r.outlier.sum() == r.n_bad_stage1 and r.outlier[:9].all()


def test_stage2_budget_follows_nbad():
    """stage 2 is given 10 iterations when the first test removed a pair and 5 when it did not (src/Optimizer.cpp:4748-4752).  At
    those budgets LM stops on its own after 2-4 iterations, so the count cannot show which one was granted: the restatement reports
    the budget it handed to the second optimize(), and a second run with budgets that the problems do use up (2 and 1: one LM
    iteration cannot meet the three-small-steps stop) shows the same choice in its_done."""
    clean = synth.make_sim3_pair(11, 25, outlier_frac=0.0)
    dirty = synth.make_sim3_pair(12, 120, outlier_frac=0.1)
    for p, want in ((clean, 5), (dirty, 10)):
        r = sim3_ref.optimize(p)
        assert (r.n_bad_stage1 == 0) == (want == 5)
        assert r.stage2_budget == want and 1 <= r.its_done[1] <= want
        q = p.copy(its_stage2_bad=2, its_stage2_clean=1)
        r = sim3_ref.optimize(q)
        assert r.its_done[1] == (1 if want == 5 else 2), (want, r.its_done)


def test_argument_checks():
    p = synth.make_sim3_pair(6, 20)
    for field, val in (("S12", np.r_[p.S12[:7], 0.0]), ("S12", np.r_[p.S12[:3], 0, 0, 0, 0, 1.0]), ("S12", np.r_[np.nan, p.S12[1:]]),
                       ("its_stage1", 0), ("w1", p.w1[:-1])):
        q = p.copy()
        setattr(q, field, val)
        with pytest.raises(ValueError):
            sim3_ref.optimize(q)
    with pytest.raises(ValueError):
        sim3_ref.optimize(p, jac="automatic")
    e = synth.make_sim3_pair(6, 0)
    r = sim3_ref.optimize(e)
    assert r.n_inliers == 0 and r.S12.tobytes() == e.S12.tobytes()


def _golden():
    return np.load(GOLDEN)


def test_golden_match():
    """the fixture (tests/golden/make_golden_sim3.py) pins the restatement against drift"""
    z = _golden()
    for k in range(int(z["n_problems"])):
        p = sim3_cases.make(tuple(z["case_%d" % k].tolist()[:2]) + (bool(z["case_%d" % k][2]), float(z["frac_%d" % k]), bool(z["case_%d" % k][3])),
                            sim3_cases.FULL)
        for name in ("S12", "p1c", "p2c", "uv1", "uv2", "w1", "w2", "K1", "K2"):
            assert np.array_equal(getattr(p, name), z["%s_%d" % (name, k)]), (k, name)    # the generator has not drifted either
        r = sim3_ref.optimize(p)
        assert r.n_inliers == int(z["n_inliers_%d" % k]) and r.n_bad_stage1 == int(z["n_bad_%d" % k])
        assert np.array_equal(r.outlier, z["outlier_%d" % k])
        np.testing.assert_allclose(r.S12, z["S12_out_%d" % k], rtol=0, atol=1e-9)
        np.testing.assert_allclose(r.chi2_stage, z["chi2_stage_%d" % k], rtol=1e-9)


def test_numeric_against_analytic_on_the_golden_problems():
    """what the reference does (central differences, step 1e-9) against what the kernel does: same flags, estimates within 1e-6"""
    z = _golden()
    for k in range(int(z["n_problems"])):
        c = z["case_%d" % k]
        p = sim3_cases.make((int(c[0]), int(c[1]), bool(c[2]), float(z["frac_%d" % k]), bool(c[3])), sim3_cases.FULL)
        a, n = sim3_ref.optimize(p), sim3_ref.optimize(p, jac="numeric")
        dt, dq, ds = _dist(n.S12, a.S12)
        print("golden %d: numeric vs analytic |dt| %.2e |dq| %.2e |ds|/s %.2e its %s vs %s" % (k, dt, dq, ds, n.its_done, a.its_done))
        assert np.array_equal(a.outlier, n.outlier) and a.n_inliers == n.n_inliers and a.n_bad_stage1 == n.n_bad_stage1
        assert max(dt, dq, ds) <= 1e-6


@pytest.mark.parametrize("case", sim3_cases.SCHEDULE, ids=sim3_cases.case_id)
def test_schedule_cases_are_decidable_at_the_short_budgets(case):
    """condition of the GPU schedule-parity test: every LM trial of both stages changes the cost by more than 1e-10 relative, and
    no chi2 that either outlier test reads lies within 1e-6 of the gate"""
    p = sim3_cases.make(case, sim3_cases.SHORT)
    r = sim3_ref.optimize(p, trace=True)
    assert r.n_inliers > 0 and len(r.trace[0]) >= 3 and len(r.trace[1]) >= 1
    for st in (0, 1):
        rel = min(abs(c0 - c1) / abs(c0) for c0, c1, _ in r.trace[st])
        print(sim3_cases.case_id(case), "stage", st, "smallest relative cost change of a trial %.2e" % rel)
        assert sim3_ref.decidable(r.trace[st], 1e-10)
    assert sim3_ref.gate_margin(r, p.th2) > 1e-6


@pytest.mark.parametrize("case", sim3_cases.RESULT, ids=sim3_cases.case_id)
def test_result_cases_keep_clear_of_the_gate_at_the_reference_budgets(case):
    p = sim3_cases.make(case, sim3_cases.FULL)
    r = sim3_ref.optimize(p, trace=True)
    print(sim3_cases.case_id(case), "gate margin %.2e" % sim3_ref.gate_margin(r, p.th2), "n_bad_stage1", r.n_bad_stage1,
          "decidable", [sim3_ref.decidable(t) for t in r.trace])
    assert sim3_ref.gate_margin(r, p.th2) > 1e-6


def test_result_cases_cover_both_stage2_budgets():
    nb = [sim3_ref.optimize(sim3_cases.make(c, sim3_cases.FULL)).n_bad_stage1 for c in sim3_cases.RESULT]
    assert any(b == 0 for b in nb) and any(b > 0 for b in nb)
