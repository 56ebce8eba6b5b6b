"""vba_sim3_optimize (k_sim3_opt) against tests/sim3_ref.py with analytic Jacobians, on a real MI355X.

The seeds come from tests/sim3_cases.py; tests/test_sim3_ref.py asserts on the CPU, for every seed and budget used here, that the
reference decides every LM trial of the schedule-parity runs on a cost change above 1e-10 relative and that no chi2 either outlier
test reads lies within 1e-6 of the gate.  Flags are compared for every pair of every problem: none is excused."""
import numpy as np
import pytest

import sim3_cases
import sim3_ref
from mc_slam_amd import backend, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0, hooks=True)
    yield b
    b.close()


def _estimate_close(got, want, tag):
    dt = np.abs(got[:3] - want[:3]).max()
    dq = min(np.abs(got[3:7] - want[3:7]).max(), np.abs(got[3:7] + want[3:7]).max())
    ds = abs(got[7] - want[7]) / want[7]
    print(tag, "|dt| %.2e |dq| %.2e |ds|/s %.2e" % (dt, dq, ds))
    assert dt <= 1e-6 and dq <= 1e-7 and ds <= 1e-7, (tag, dt, dq, ds)


def _common(g, r, tag):
    assert g.status == r.status == 0
    assert g.n_bad_stage1 == r.n_bad_stage1, tag
    assert np.array_equal(g.outlier, r.outlier), (tag, np.nonzero(g.outlier != r.outlier)[0])
    assert g.n_inliers == r.n_inliers, tag
    print(tag, "chi2_stage gpu", g.chi2_stage, "ref", r.chi2_stage, "its gpu", g.its_done, "ref", r.its_done)
    np.testing.assert_allclose(g.chi2_stage, r.chi2_stage, rtol=1e-7, atol=0)
    _estimate_close(g.S12, r.S12, tag)
    np.testing.assert_allclose(g.chi2_12, r.chi2_12, rtol=1e-6)
    np.testing.assert_allclose(g.chi2_21, r.chi2_21, rtol=1e-6)


@pytest.mark.parametrize("case", sim3_cases.SCHEDULE, ids=sim3_cases.case_id)
def test_schedule_parity_at_short_budgets(ba, case):
    """budgets (3, 2, 2): the problems do not converge, so the estimate returned depends on every lambda, rho and nu"""
    p = sim3_cases.make(case, sim3_cases.SHORT)
    r = sim3_ref.optimize(p, trace=True)
    assert sim3_ref.decidable(r.trace[0]) and sim3_ref.decidable(r.trace[1])
    g = ba.sim3_optimize([p])[0]
    assert tuple(g.its_done) == tuple(r.its_done), (g.its_done, r.its_done)
    _common(g, r, sim3_cases.case_id(case))


@pytest.mark.parametrize("case", sim3_cases.RESULT, ids=sim3_cases.case_id)
def test_result_parity_at_the_reference_budgets(ba, case):
    """budgets (5, 10, 5): the problems converge, and LM then decides on rounding, so an iteration count is compared only for a
    stage whose every reference trial moved the cost by more than 1e-10 relative"""
    p = sim3_cases.make(case, sim3_cases.FULL)
    r = sim3_ref.optimize(p, trace=True)
    g = ba.sim3_optimize([p])[0]
    budget = (p.its_stage1, p.its_stage2_bad if r.n_bad_stage1 > 0 else p.its_stage2_clean)
    for k in (0, 1):
        if sim3_ref.decidable(r.trace[k]):
            assert g.its_done[k] == r.its_done[k], (k, g.its_done, r.its_done)
        else:
            assert 1 <= g.its_done[k] <= budget[k], (k, g.its_done, budget)
    _common(g, r, sim3_cases.case_id(case))


def test_result_cases_cover_both_stage2_budgets(ba):
    ps = [sim3_cases.make(c, sim3_cases.FULL) for c in sim3_cases.RESULT]
    nb = [g.n_bad_stage1 for g in ba.sim3_optimize(ps)]
    assert any(b == 0 for b in nb) and any(b > 0 for b in nb)


def _bits(r):
    return (r.n_inliers, r.status, r.n_bad_stage1, tuple(r.its_done), r.chi2_stage.tobytes(), r.outlier.tobytes(), r.chi2_12.tobytes(),
            r.chi2_21.tobytes(), r.S12.tobytes())


def _ragged():
    few = synth.make_sim3_pair(31, 16, outlier_frac=0.0)
    few.uv1[:9] += 60.0                                  # leaves fewer than 10 good pairs: returns 0
    return [synth.make_sim3_pair(32, 120), synth.make_sim3_pair(33, 0), few, synth.make_sim3_pair(34, 90, fix_scale=True),
            synth.make_sim3_pair(35, 2000, outlier_frac=0.2), synth.make_sim3_pair(36, 25, outlier_frac=0.0),
            synth.make_sim3_pair(37, 65, same_K=True), synth.make_sim3_pair(38, 400, outlier_frac=0.3)]


def test_ragged_batch_equals_single_calls_bit_for_bit(ba):
    ps = _ragged()
    batch = ba.sim3_optimize(ps)
    again = ba.sim3_optimize(ps)
    single = [ba.sim3_optimize([p])[0] for p in ps]
    for k, (b, a, s) in enumerate(zip(batch, again, single)):
        assert _bits(b) == _bits(s), k
        assert _bits(b) == _bits(a), k
    assert batch[1].n_inliers == 0 and batch[1].S12.tobytes() == ps[1].S12.tobytes()
    assert batch[2].n_inliers == 0 and batch[2].S12.tobytes() == ps[2].S12.tobytes() and batch[2].outlier[:9].all()
    assert batch[2].its_done[1] == 0 and batch[2].outlier.sum() == batch[2].n_bad_stage1
    assert batch[4].n_inliers > 1000
    # and against the yardstick, the 2 000-pair problem included
    for k, p in enumerate(ps):
        r = sim3_ref.optimize(p)
        assert np.array_equal(batch[k].outlier, r.outlier) and batch[k].n_inliers == r.n_inliers, k
        _estimate_close(batch[k].S12, r.S12, "ragged %d" % k)


def test_small_call_after_a_large_one_equals_a_fresh_handle(ba):
    """arena reuse: 64 candidates of 200 pairs, then 1 candidate of 7 pairs on the same handle -- bit for bit what a fresh handle
    returns for the small call (nothing the large call left in the arena or the staging is read)"""
    ba.sim3_optimize([synth.make_sim3_pair(200 + k, 200) for k in range(64)])
    p = synth.make_sim3_pair(39, 7, outlier_frac=0.0).copy(min_inliers=3)                # seven pairs are enough: both stages run
    got = ba.sim3_optimize([p])[0]
    fresh = backend.LocalBA(0, hooks=True)
    try:
        want = fresh.sim3_optimize([p])[0]
    finally:
        fresh.close()
    assert got.n_inliers > 0 and got.its_done[1] > 0 and _bits(got) == _bits(want)


def test_batched_call_is_one_kernel_launch(ba):
    ba.sim3_optimize(_ragged())
    assert ba.get_profile()["kernel_launches"] == 1


def test_noise_free_problem_recovers_the_truth(ba):
    p = synth.make_sim3_pair(3, 80, outlier_frac=0.0, noise=False)
    g = ba.sim3_optimize([p])[0]
    assert g.n_inliers == 80 and not g.outlier.any()
    _estimate_close(g.S12, p.truth["S12"], "noise-free vs truth")


def test_fix_scale_leaves_the_scale_bit_identical(ba):
    p = synth.make_sim3_pair(4, 120, fix_scale=True)
    g = ba.sim3_optimize([p])[0]
    assert g.n_inliers > 0 and g.S12[7].tobytes() == p.S12[7].tobytes()
    assert not np.array_equal(g.S12[:7], p.S12[:7])


def test_bad_arguments_fail_with_a_message(ba):
    p = synth.make_sim3_pair(6, 20)
    for field, val, msg in (("S12", np.r_[p.S12[:7], 0.0], "scale of S12 is not positive"),
                            ("S12", np.r_[p.S12[:3], 0, 0, 0, 0, 1.0], "zero quaternion"),
                            ("S12", np.r_[np.nan, p.S12[1:]], "S12 is not finite"),
                            ("its_stage1", 0, "budgets must be at least 1")):
        q = p.copy()
        setattr(q, field, val)
        with pytest.raises(RuntimeError, match=msg):
            ba.sim3_optimize([p, q])
    packed = ba.sim3_pack([p])
    packed[1][0].n_pairs = -1
    with pytest.raises(RuntimeError, match="negative n_pairs"):
        ba.sim3_call(packed)
    packed = ba.sim3_pack([p])
    packed[1][0].uv2 = None
    with pytest.raises(RuntimeError, match="NULL array"):
        ba.sim3_call(packed)
    assert ba.sim3_optimize([p])[0].n_inliers > 0


def test_refused_while_an_asynchronous_ticket_is_pending(ba):
    p = synth.make_sim3_pair(7, 60)
    want = ba.sim3_optimize([p])[0]
    w = synth.config_c3(seed=7, n_kf=10, n_pt=400, n_obs=2000)
    assert ba.lib.vba_debug_async_hold(ba.h, 1) == 0
    try:
        t = ba.submit([w])
        with pytest.raises(RuntimeError, match="asynchronous batches pending: wait for them first"):
            ba.sim3_optimize([p])
    finally:
        assert ba.lib.vba_debug_async_hold(ba.h, 0) == 0
    ba.wait(t)
    assert _bits(ba.sim3_optimize([p])[0]) == _bits(want)


def test_a_sim3_call_disturbs_no_solver_state(ba):
    """vba_solve of the smoke window on the same handle: bit-identical before and after a Sim3 call"""
    w = synth.config_c3(seed=7, n_kf=10, n_pt=400, n_obs=2000)
    q0, r0 = ba.solve(w)
    ba.sim3_optimize(_ragged())
    q1, r1 = ba.solve(w)
    for k in ("kf_pose", "kf_vel", "kf_bias", "pt"):
        assert np.array_equal(getattr(q0, k), getattr(q1, k)), k
    assert r0.its_done == r1.its_done and r0.chi2_vis == r1.chi2_vis and np.array_equal(r0.obs_outlier, r1.obs_outlier)
    assert np.array_equal(r0.chi2_trace, r1.chi2_trace)
