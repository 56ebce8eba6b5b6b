"""vba_posegraph_optimize (k_posegraph_opt, k_posegraph_points) against tests/posegraph_ref.py, on a real MI355X.

The graphs and the tolerances come from tests/posegraph_cases.py; tests/test_posegraph_ref.py derives the tolerances on the CPU
(float64 against longdouble yardstick) and asserts that every LM trial of the schedule-parity runs is decided on a cost change
above 1e-10 relative.  Every yardstick run is computed once per session and shared."""
import functools

import numpy as np
import pytest

import posegraph_cases as pc
import posegraph_ref as ref
from mc_slam_amd import backend, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0, hooks=True)
    yield b
    b.close()


@functools.lru_cache(maxsize=None)
def _ref(name, its):
    return ref.optimize(pc.case(name, its=its))


def _close(g, r, tag):
    """estimates and chi2 within the tolerances of posegraph_cases"""
    dt = np.abs(g.S[:, :3] - r.S[:, :3]).max()
    dq = np.minimum(np.abs(g.S[:, 3:7] - r.S[:, 3:7]).max(axis=1), np.abs(g.S[:, 3:7] + r.S[:, 3:7]).max(axis=1)).max()
    ds = np.abs(g.S[:, 7] / r.S[:, 7] - 1).max()
    dc = abs(g.chi2_final - r.chi2_final) / r.chi2_final
    d0 = abs(g.chi2_initial - r.chi2_initial) / r.chi2_initial
    print(tag, "|dt| %.2e |dq| %.2e |ds|/s %.2e |dchi|/chi %.2e (initial %.2e)  gpu (its, trials, stop) %s ref %s" % (
        dt, dq, ds, dc, d0, (g.its_done, g.lm_trials, g.stop), (r.its_done, r.lm_trials, r.stop)))
    assert g.status == 0
    assert dt <= pc.TOL_T and dq <= pc.TOL_Q and ds <= pc.TOL_S and dc <= pc.TOL_CHI and d0 <= pc.TOL_CHI, (tag, dt, dq, ds, dc, d0)


def _bits(g):
    return (g.S.tobytes(), g.pt.tobytes(), g.status, g.its_done, g.lm_trials, g.stop, np.float64(g.chi2_initial).tobytes(),
            np.float64(g.chi2_final).tobytes(), np.float64(g.lambda_final).tobytes())


@pytest.mark.parametrize("name", pc.SCHEDULE)
def test_schedule_parity_at_three_iterations(ba, name):
    """its = 3: the estimate returned depends on every lambda, rho and nu of the schedule"""
    r = _ref(name, 3)
    assert ref.decidable(r.trace)
    g = ba.posegraph_optimize([pc.case(name, its=3)])[0]
    assert (g.its_done, g.lm_trials, g.stop) == (r.its_done, r.lm_trials, r.stop)
    _close(g, r, name + " its=3")


@pytest.mark.parametrize("name", pc.CASES)
def test_result_parity_at_twenty_iterations(ba, name):
    p = pc.case(name)
    assert p.its == 20
    r = _ref(name, 20)
    g = ba.posegraph_optimize([p])[0]
    if ref.decidable(r.trace):
        assert (g.its_done, g.lm_trials) == (r.its_done, r.lm_trials)
    else:
        assert 1 <= g.its_done <= 20
    _close(g, r, name)
    fx = p.fixed.astype(bool)
    assert g.S[fx].tobytes() == p.S[fx].tobytes()                       # fixed vertices: bit-identical
    assert not np.array_equal(g.S[~fx][:, :7], p.S[~fx][:, :7])
    if p.fix_scale:
        assert g.S[:, 7].tobytes() == p.S[:, 7].tobytes()               # every scale bit-identical while the poses change


def test_rejected_first_step_stops_after_ten_trials(ba):
    p = pc.case("REJECT")
    r = _ref("REJECT", 20)
    assert (r.its_done, r.lm_trials, r.stop) == (1, 10, 1) and ref.decidable(r.trace)
    g = ba.posegraph_optimize([p])[0]
    assert (g.its_done, g.lm_trials, g.stop) == (1, 10, 1)
    assert g.S.tobytes() == p.S.tobytes()
    assert abs(g.chi2_final - r.chi2_final) <= pc.TOL_CHI * r.chi2_final


@pytest.mark.parametrize("name", ["ARROW", "BAND", "NEST"])
def test_the_linear_solve_by_itself(ba, name):
    """H, b and the x of the first trial as the kernel formed them: normwise backward error of x within 100 n u (Cholesky's bound
    is of order n u; the 100 is slack for its constant), and H, b against the yardstick's"""
    p = pc.case(name)
    H, b, x = ba.posegraph_system(p)
    n = len(b)
    assert n == 7 * int((p.fixed == 0).sum()) and np.array_equal(H, H.T)
    lam = p.lambda_init
    res = np.abs((H + lam * np.eye(n)) @ x - b).max()
    be = res / (np.abs(H).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())
    print(name, "n", n, "backward error %.2e bound %.2e" % (be, 100 * n * 2.0 ** -53))
    assert be <= 100 * n * 2.0 ** -53
    if p.fix_scale:                                   # zero scale columns: the scale rows of H hold nothing, the pivot is lambda
        assert not H[6::7].any() and not b[6::7].any() and not x[6::7].any()
    if name in ("BAND", "NEST"):
        r = _ref(name, 20)
        dH = np.abs(H - r.H0).max() / np.abs(r.H0).max()
        db = np.abs(b - r.b0).max() / np.abs(r.b0).max()
        print(name, "|dH|/|H| %.2e |db|/|b| %.2e" % (dH, db))
        assert dH <= pc.TOL_CHI and db <= pc.TOL_CHI


def test_batch_equals_single_calls_and_a_repeated_call(ba):
    ps = [pc.case(n) for n in pc.CASES + ["REJECT"]]
    batch = ba.posegraph_optimize(ps)
    again = ba.posegraph_optimize(ps)
    rev = ba.posegraph_optimize(ps[::-1])[::-1]
    for k, p in enumerate(ps):
        one = ba.posegraph_optimize([p])[0]
        assert _bits(batch[k]) == _bits(one) == _bits(again[k]) == _bits(rev[k]), k


def test_small_call_after_a_large_one_equals_a_fresh_handle(ba):
    """arena reuse: 4 graphs of 60 vertices, then 1 graph of 5 vertices with 3 map points on the same handle -- bit for bit what a
    fresh handle returns for the small call (nothing the large call left in the arena or the staging is read)"""
    ba.posegraph_optimize([synth.make_posegraph(70 + k, 60, loops=[(55, 3)]) for k in range(4)])
    p = synth.make_posegraph(75, 5, span=2, n_pt=3)
    assert (p.n_vertices, p.n_pt) == (5, 3)
    got = ba.posegraph_optimize([p])[0]
    fresh = backend.LocalBA(0, hooks=True)
    try:
        want = fresh.posegraph_optimize([p])[0]
    finally:
        fresh.close()
    assert got.chi2_final < got.chi2_initial and _bits(got) == _bits(want)            # the small call did move its estimates


def test_launch_counts(ba):
    ba.posegraph_optimize([pc.case("ARROW"), pc.case("BAND")])
    assert ba.get_profile()["kernel_launches"] == 1
    ba.posegraph_optimize([pc.case("ARROW"), pc.case("BIG")])
    assert ba.get_profile()["kernel_launches"] == 2


def test_map_points_follow_their_reference_vertex(ba):
    p = pc.case("BIG")
    g = ba.posegraph_optimize([p, pc.case("ARROW")])[0]
    want = ref.move_points(p.S, g.S, p.pt, p.pt_ref.astype(int))
    err = np.abs(g.pt - want) / np.maximum(1.0, np.abs(want))
    print("map points: max scaled error %.2e, largest move %.2e" % (err.max(), np.abs(g.pt - p.pt).max()))
    assert err.max() <= 1e-12
    assert np.abs(g.pt - p.pt).max() > 1e-3
    fx = np.nonzero(p.fixed)[0]
    at_fixed = np.isin(p.pt_ref, fx)
    assert at_fixed.any() and np.abs(g.pt[at_fixed] - p.pt[at_fixed]).max() <= 1e-12 * np.abs(p.pt).max()


def _bad_graphs():
    p = pc.case("ARROW")
    nan_S = p.S.copy(); nan_S[3, 1] = np.nan
    zq_S = p.S.copy(); zq_S[2, 3:7] = 0
    s0_S = p.S.copy(); s0_S[4, 7] = 0.0
    inf_M = p.edge_S.copy(); inf_M[1, 0] = np.inf
    zq_M = p.edge_S.copy(); zq_M[2, 3:7] = 0
    s0_M = p.edge_S.copy(); s0_M[0, 7] = -1.0
    ei_big = p.edge_i.copy(); ei_big[3] = 12
    ej_neg = p.edge_j.copy(); ej_neg[3] = -1
    ej_same = p.edge_j.copy(); ej_same[5] = p.edge_i[5]
    two_fixed = p.fixed.copy(); two_fixed[1] = 1          # edge (1, 0) now joins two fixed vertices
    q = pc.case("BIG")
    ref_bad = q.pt_ref.copy(); ref_bad[7] = 150
    return [(p.copy(S=nan_S), "S is not finite"), (p.copy(S=zq_S), "zero quaternion in S"), (p.copy(S=s0_S), "scale of S is not positive"),
            (p.copy(edge_S=inf_M), "edge_S is not finite"), (p.copy(edge_S=zq_M), "zero quaternion in edge_S"),
            (p.copy(edge_S=s0_M), "scale of edge_S is not positive"), (p.copy(edge_i=ei_big), "edge index out of range"),
            (p.copy(edge_j=ej_neg), "edge index out of range"), (p.copy(edge_j=ej_same), "edge_i == edge_j"),
            (p.copy(fixed=two_fixed), "edge between two fixed vertices"), (p.copy(its=0), "its must be at least 1"),
            (p.copy(lambda_init=0.0), "lambda_init must be positive"), (q.copy(pt_ref=ref_bad), "pt_ref out of range"),
            (p.copy(fixed=np.ones(12, dtype=np.uint8), edge_i=p.edge_i[:0], edge_j=p.edge_j[:0], edge_S=p.edge_S[:0]), "no free vertex")]


def test_bad_arguments_fail_with_a_message(ba):
    good = pc.case("ARROW")
    want = _bits(ba.posegraph_optimize([good])[0])
    for q, msg in _bad_graphs():
        with pytest.raises(RuntimeError, match="graph 1: " + msg):
            ba.posegraph_optimize([good, q])
    for field, val, msg in (("n_vertices", -1, "negative count"), ("n_edges", -1, "negative count"), ("n_pt", -1, "negative count"),
                            ("edge_S", None, "NULL array"), ("S", None, "NULL array"), ("n_pt", 3, "NULL array")):
        packed = ba.posegraph_pack([good])
        if field == "n_pt" and val == 3:
            packed[1][0].pt = None
        setattr(packed[1][0], field, val)
        with pytest.raises(RuntimeError, match="graph 0: " + msg):
            ba.posegraph_call(packed)
    # a factor beyond the size bound: 1 500 vertices, every one tied to vertex 1 -- 1.1 million blocks, twice in one call
    n = 1500
    star = synth.make_posegraph(5, n, span=1, loops=[(i, 1) for i in range(3, n)], fixed_at=0)
    with pytest.raises(RuntimeError, match="graph 1: the envelope of the factor exceeds the bound"):
        ba.posegraph_optimize([star, star])
    assert ba.posegraph_optimize([]) == []
    assert _bits(ba.posegraph_optimize([good])[0]) == want


def test_refused_while_an_asynchronous_ticket_is_pending(ba):
    p = pc.case("ARROW")
    want = ba.posegraph_optimize([p])[0]
    w = synth.config_c3(seed=7, n_kf=10, n_pt=400, n_obs=2000)
    assert ba.lib.vba_debug_async_hold(ba.h, 1) == 0
    try:
        t = ba.submit([w])
        with pytest.raises(RuntimeError, match="asynchronous batches pending: wait for them first"):
            ba.posegraph_optimize([p])
    finally:
        assert ba.lib.vba_debug_async_hold(ba.h, 0) == 0
    ba.wait(t)
    assert _bits(ba.posegraph_optimize([p])[0]) == _bits(want)


def test_a_posegraph_call_disturbs_no_solver_state(ba):
    """vba_solve of the smoke window on the same handle: bit-identical before and after a pose-graph call"""
    w = synth.config_c3(seed=7, n_kf=10, n_pt=400, n_obs=2000)
    q0, r0 = ba.solve(w)
    ba.posegraph_optimize([pc.case("BAND"), pc.case("BIG")])
    q1, r1 = ba.solve(w)
    for k in ("kf_pose", "kf_vel", "kf_bias", "pt"):
        assert np.array_equal(getattr(q0, k), getattr(q1, k)), k
    assert r0.its_done == r1.its_done and r0.chi2_vis == r1.chi2_vis and np.array_equal(r0.obs_outlier, r1.obs_outlier)
    assert np.array_equal(r0.chi2_trace, r1.chi2_trace)
