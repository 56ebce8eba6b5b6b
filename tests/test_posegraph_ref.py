"""The yardstick of the pose-graph tests (tests/posegraph_ref.py) on the CPU: its Sim3 arithmetic, known answers, the measured
float64-against-longdouble sensitivity that the GPU tolerances of tests/posegraph_cases.py are derived from, the decidability of
the schedule-parity cases, and the ten-trial stop."""
import functools

import numpy as np
import pytest

import posegraph_cases as pc
import posegraph_ref as ref
from mc_slam_amd import synth


@functools.lru_cache(maxsize=None)
def _run(name, its, long):
    return ref.optimize(pc.case(name, its=its), dtype=np.longdouble if long else np.float64)


def _qdiff(a, b):
    return np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1)).max()


# ---- arithmetic ----
def _tangents():
    """updates in all four branches of sim3.h (|sigma| < 1e-5 or not, theta < 1e-5 or not) and on both sides of both thresholds"""
    r = np.random.default_rng(5)
    rows, want = [], []
    for sg, bs in ((0.0, 1), (3e-6, 1), (0.9999e-5, 1), (1.0001e-5, 0), (0.2, 0), (-0.3, 0)):
        for th, bt in ((0.0, 1), (4e-6, 1), (0.9999e-5, 1), (1.0001e-5, 0), (0.4, 0), (2.5, 0)):
            ax = r.normal(size=3)
            rows.append(np.concatenate([th * ax / np.linalg.norm(ax), r.normal(size=3), [sg]]))
            want.append((0 if bt else 1) if bs else (2 if bt else 3))
    return np.array(rows), np.array(want)


def test_exp_takes_the_branch_of_its_thresholds_and_log_inverts_it():
    u, want = _tangents()
    info = {}
    S = ref.sim3_exp(u, info)
    assert np.array_equal(info["branch"], want) and set(want) == {0, 1, 2, 3}
    back = ref.sim3_log(S)
    # omega and sigma come back in every branch.  upsilon comes back wherever the reference's own formulas are consistent: the B
    # of its branch "sigma not small, angle small" lacks the "- 1" of the series (sim3.h:116, :199: B ~ 1 / sigma^3), and log takes
    # that branch up to theta = 4.47e-3 (d > 1 - 1e-5) while exp leaves it at theta = 1e-5, so there the two disagree
    assert np.abs(back[:, [0, 1, 2, 6]] - u[:, [0, 1, 2, 6]]).max() <= 1e-9
    theta = np.linalg.norm(u[:, :3], axis=1)
    ok = ~((np.abs(u[:, 6]) >= 1e-5) & (theta < 4.4e-3))
    assert ok.sum() >= 24 and np.abs(back[ok][:, 3:6] - u[ok][:, 3:6]).max() <= 1e-9
    # both small-angle thresholds of log (d > 1 - 1e-5, i.e. theta < 4.47e-3) with sigma = 0
    th = np.array([4.4e-3, 4.5e-3, 1e-3, 1e-2])
    v = np.zeros((4, 7)); v[:, 1] = th; v[:, 3:6] = [0.3, -0.2, 0.5]
    info2 = {}
    back2 = ref.sim3_log(ref.sim3_exp(v), info2)
    assert list(info2["branch"]) == [0, 1, 0, 1]
    assert np.abs(back2 - v).max() <= 1e-7            # the small-angle branch is a truncation: omega to theta^3 / 6, A and B to theta^2


def test_product_with_the_inverse_is_the_identity():
    u, _ = _tangents()
    S = ref.sim3_exp(u)
    for P in (ref.sim3_mul(S, ref.sim3_inv(S)), ref.sim3_mul(ref.sim3_inv(S), S)):
        assert np.abs(P[0] - [0, 0, 0, 1]).max() <= 1e-15 and np.abs(P[2] - 1).max() <= 1e-15
        assert (np.abs(P[1]).max(axis=1) <= 1e-15 * np.maximum(1.0, np.abs(S[1]).max(axis=1))).all()     # relative to |t|
    p = np.random.default_rng(1).normal(size=(len(u), 3))
    back = ref.sim3_map(ref.sim3_inv(S), ref.sim3_map(S, p))
    assert (np.abs(back - p).max(axis=1) <= 1e-14 * np.maximum(1.0, np.abs(S[1]).max(axis=1))).all()


def test_central_differences_agree_with_a_longdouble_difference_quotient():
    p = pc.case("ARROW")
    ei, ej = p.edge_i.astype(int), p.edge_j.astype(int)
    J = ref.jacobians(ref.unpack(p.S), ref.unpack(p.edge_S), ei, ej, False)
    Jl = ref.jacobians(ref.unpack(p.S, np.longdouble), ref.unpack(p.edge_S, np.longdouble), ei, ej, False)
    Jw = ref.jacobians(ref.unpack(p.S, np.longdouble), ref.unpack(p.edge_S, np.longdouble), ei, ej, False, delta=1e-6)
    scale = max(np.abs(Jl[0]).max(), np.abs(Jl[1]).max())
    for k in (0, 1):
        # float64: rounding of the error (1e-16 of values up to ~5) over 2e-9; longdouble with two step sizes: truncation only
        assert np.abs(J[k] - Jl[k]).max() <= 1e-5 * scale
        assert np.abs(Jl[k] - Jw[k]).max() <= 1e-6 * scale
    fx = ref.jacobians(ref.unpack(p.S), ref.unpack(p.edge_S), ei, ej, True)
    assert not fx[0][:, :, 6].any() and not fx[1][:, :, 6].any()       # fix_scale: the scale column is exactly zero
    assert fx[0][:, :, :6].any()


# ---- known answers ----
def test_a_noise_free_graph_stays_put():
    p = synth.make_posegraph(3, 20, span=2, loops=[(19, 0), (18, 1)], noise=False, fix_scale=True)
    assert np.abs(p.S - p.truth["S"]).max() <= 1e-14          # (the odometry is composed from the true relative motions)
    r = ref.optimize(p)
    assert r.chi2_initial <= 1e-25 and r.chi2_final <= 1e-25
    assert np.abs(r.S[:, :3] - p.S[:, :3]).max() <= 1e-12 and _qdiff(r.S[:, 3:7], p.S[:, 3:7]) <= 1e-12


def test_a_drifted_graph_is_pulled_towards_the_truth_by_exact_loop_edges():
    """every non-loop edge is measured from the drifted poses, so the optimum is a compromise, not the truth: the loop-closed
    estimate has to be several times closer to the truth than the input (the gauge is that of the fixed vertex 0, which starts at
    the truth).  With a single exact edge the truth itself comes back."""
    p = synth.make_posegraph(4, 40, span=2, loops=[(39 - k, k) for k in range(4)], fix_scale=True, trans_drift=5e-2, n_corrected=0)
    r = ref.optimize(p)
    e_in = np.abs(p.S[:, :3] - p.truth["S"][:, :3]).max()
    e_out = np.abs(r.S[:, :3] - p.truth["S"][:, :3]).max()
    assert r.chi2_final < 0.1 * r.chi2_initial and e_out < 0.5 * e_in, (e_in, e_out)
    two = synth.make_posegraph(6, 2, span=0, loops=[(1, 0)], fix_scale=True)
    two.S[1, :3] += [0.3, -0.2, 0.1]
    r = ref.optimize(two)
    assert np.abs(r.S[:, :3] - two.truth["S"][:, :3]).max() <= 1e-7 and _qdiff(r.S[:, 3:7], two.truth["S"][:, 3:7]) <= 1e-8


# ---- the tolerances of the GPU tests ----
def test_gpu_tolerances_are_ten_times_the_measured_sensitivity():
    d_t = d_q = d_s = d_chi = 0.0
    for name, its in [(n, 20) for n in pc.CASES] + [(n, 3) for n in pc.SCHEDULE]:
        a, b = _run(name, its, False), _run(name, its, True)
        d_t = max(d_t, np.abs(a.S[:, :3] - b.S[:, :3]).max())
        d_q = max(d_q, _qdiff(a.S[:, 3:7], b.S[:, 3:7]))
        d_s = max(d_s, np.abs(a.S[:, 7] / b.S[:, 7] - 1).max())
        d_chi = max(d_chi, abs(a.chi2_final / b.chi2_final - 1))
    print("d_t %.3e d_q %.3e d_s %.3e d_chi %.3e" % (d_t, d_q, d_s, d_chi))
    for d, tol, what in ((d_t, pc.TOL_T, "TOL_T"), (d_q, pc.TOL_Q, "TOL_Q"), (d_s, pc.TOL_S, "TOL_S"), (d_chi, pc.TOL_CHI, "TOL_CHI")):
        assert 10 * d <= tol <= 100 * d, (what, d, tol)


@pytest.mark.parametrize("name", pc.SCHEDULE)
def test_schedule_cases_are_decided_on_real_cost_changes(name):
    r = _run(name, 3, False)
    assert len(r.trace) == r.lm_trials and ref.decidable(r.trace)
    rl = _run(name, 3, True)
    assert (r.its_done, r.lm_trials, r.stop) == (rl.its_done, rl.lm_trials, rl.stop)
    assert [t[2] for t in r.trace] == [t[2] for t in rl.trace]


def test_a_rejected_first_step_is_retried_ten_times():
    """a loop measurement wrong by 2.5 rad: the first step and all nine retries raise the cost, so LM gives up after ten trials
    and every estimate is popped back"""
    for long in (False, True):
        r = _run("REJECT", 20, long)
        assert (r.its_done, r.lm_trials, r.stop) == (1, 10, 1)
        assert not any(t[2] for t in r.trace) and ref.decidable(r.trace)
        assert all(t[1] > 1.05 * t[0] for t in r.trace)                 # rejected on a cost that rose by more than 5 %
        assert np.array_equal(r.S, pc.case("REJECT").S)
        assert r.lambda_final == 1e-16 * 2.0 ** sum(range(1, 11))       # nu doubles at every rejection: 2, 4, 8, ...


def test_yardstick_runs_in_seconds():
    import time
    t = time.time()
    ref.optimize(pc.case("BIG"))
    assert time.time() - t < 20
