"""vba_sim3_ransac (k_sim3_ransac) against tests/sim3_ransac_ref.py in float64, on a real MI355X.

The cases come from tests/sim3_ransac_cases.py; tests/test_sim3_ransac_ref.py asserts on the CPU, for every hypothesis of every
case, that Horn's N has an eigenvalue gap of at least 1e-4 and that no reprojection error lies within 1e-6 of its gate, so every
count, flag and decision below is compared exactly and for every hypothesis: none is excused."""
import numpy as np
import pytest

import sim3_ransac_cases as cases
import sim3_ransac_ref as ref
from mc_slam_amd import abi, backend, synth

pytestmark = pytest.mark.gpu

# Ten times the largest float64-against-longdouble difference of the yardstick over all hypotheses of all cases, rounded up to one
# digit (tests/test_sim3_ransac_ref.py::test_print_float64_against_longdouble prints |dt| 3.699e-13, |dq| 4.310e-14, |ds| 2.578e-15).
# The kernel and the float64 yardstick are two FP64 evaluations of the same formulas (fused multiply-adds, a different route from
# the eigenvector to R), so each may differ from the exact value by about that much.
TOL_T, TOL_Q, TOL_S = 4e-12, 5e-13, 3e-14


@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0)
    yield b
    b.close()


def _dS(got, want):
    return np.abs(got[:3] - want[:3]).max(), np.abs(got[3:7] - want[3:7]).max(), abs(got[7] - want[7])


def _same(a, b):
    """two results of the library, bit for bit"""
    assert (a.status, a.hit, a.its_done, a.best_hyp, a.n_inliers, a.best_inliers) == (b.status, b.hit, b.its_done, b.best_hyp, b.n_inliers, b.best_inliers)
    assert a.S12.tobytes() == b.S12.tobytes() and a.best_S12.tobytes() == b.best_S12.tobytes()
    assert np.array_equal(a.inlier, b.inlier) and np.array_equal(a.hyp_inliers, b.hyp_inliers)


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_against_the_yardstick(ba, case):
    p = cases.make(case)
    r = cases.reference(case)
    g = ba.sim3_ransac([p])[0]
    assert g.status == 0
    assert np.array_equal(g.hyp_inliers, r["hyp_inliers"]), np.nonzero(g.hyp_inliers != r["hyp_inliers"])[0]
    assert (g.hit, g.its_done, g.best_hyp, g.n_inliers, g.best_inliers) == (r["hit"], r["its_done"], r["best_hyp"], r["n_inliers"], r["best_inliers"])
    d_best = _dS(g.best_S12, r["best_S12"])
    print(cases.IDS[cases.CASES.index(case)], "best_S12 |dt| %.2e |dq| %.2e |ds| %.2e" % d_best)
    if r["hit"] >= 0:
        assert np.array_equal(g.inlier, r["inlier"]), np.nonzero(g.inlier != r["inlier"])[0]
        d_hit = _dS(g.S12, r["S12"])
        print("    S12 |dt| %.2e |dq| %.2e |ds| %.2e" % d_hit)
        assert d_hit[0] <= TOL_T and d_hit[1] <= TOL_Q and d_hit[2] <= TOL_S, d_hit
    else:
        assert not g.S12.any() and not g.inlier.any()     # untouched: the buffers start as zeros
    assert d_best[0] <= TOL_T and d_best[1] <= TOL_Q and d_best[2] <= TOL_S, d_best


def test_degenerate_triples(ba):
    """(i, i, i) with a free scale counts 0; (i, i, j) and a collinear triple complete with a count in range; all OTHER hypotheses
    of the call are bit-identical to the same call without the degenerate ones"""
    p0 = cases.make(cases.CASES[7])            # free scale, no hit: every hypothesis is consumed
    assert p0.fix_scale == 0 and cases.reference(cases.CASES[7])["hit"] < 0
    # a collinear triple: pairs n, n+1, n+2 are three points on a line in both frames
    R, t, s = synth.so3_exp(np.array([0.1, -0.2, 0.05])), np.array([0.2, -0.1, 0.3]), 1.1
    line2 = np.array([[0.0, 0.0, 4.0]]) + np.array([[0.0], [1.0], [2.5]]) * np.array([[0.3, -0.2, 0.5]])
    n = p0.n_pairs
    p = p0.copy(p1c=np.vstack([p0.p1c, s * line2 @ R.T + t]), p2c=np.vstack([p0.p2c, line2]),
                max_err1=np.concatenate([p0.max_err1, [9.21] * 3]), max_err2=np.concatenate([p0.max_err2, [9.21] * 3]))
    clean = p0.sample
    deg = {2: [5, 5, 5], 9: [5, 5, 9], 10: [n, n + 1, n + 2], 40: [7, 3, 7]}
    rows, k = [], 0
    for h in range(len(clean) + len(deg)):
        if h in deg:
            rows.append(deg[h])
        else:
            rows.append(clean[k]); k += 1
    keep = np.array([h for h in range(len(rows)) if h not in deg])
    g = ba.sim3_ransac([p.copy(sample=np.array(rows, dtype=np.int32), min_inliers=10 ** 6)])[0]
    g0 = ba.sim3_ransac([p.copy(sample=clean, min_inliers=10 ** 6)])[0]
    assert g.hit == -1 and g.its_done == len(rows)
    assert g.hyp_inliers[2] == 0
    y, _, _, _ = ref.counts(p, [deg[2]])
    assert y[0] == 0
    for h in (9, 10, 40):
        assert 0 <= g.hyp_inliers[h] <= p.n_pairs
    assert np.array_equal(g.hyp_inliers[keep], g0.hyp_inliers)
    # per hypothesis the ABI hands out the count alone; an estimate and flags come back for the hit, so make the best hypothesis
    # the hit of both calls (min_inliers just below its count) and compare those bit for bit, too
    c = g0.hyp_inliers
    m = int(c.max()) - 1
    a = ba.sim3_ransac([p.copy(sample=np.array(rows, dtype=np.int32), min_inliers=m)])[0]
    b = ba.sim3_ransac([p.copy(sample=clean, min_inliers=m)])[0]
    assert a.hit == keep[b.hit] and a.n_inliers == b.n_inliers
    assert a.S12.tobytes() == b.S12.tobytes() and np.array_equal(a.inlier, b.inlier)


def test_a_later_tie_replaces_the_best(ba):
    case = cases.CASES[7]                      # no hit
    p, r = cases.make(case), cases.reference(case)
    top = int(np.argmax(r["hyp_inliers"]))
    s = p.sample.copy()
    s[3] = s[7] = p.sample[top]
    q = p.copy(sample=s)
    y = ref.ransac(q)
    g = ba.sim3_ransac([q])[0]
    assert y["hit"] == -1 and y["hyp_inliers"][3] == y["hyp_inliers"][7] == y["hyp_inliers"].max()
    assert np.array_equal(g.hyp_inliers, y["hyp_inliers"])
    last = int(np.nonzero(y["hyp_inliers"] == y["hyp_inliers"].max())[0][-1])
    assert last >= 7 and g.best_hyp == y["best_hyp"] == last and g.hit == -1
    if top < 3:                                # nothing after 7 reaches the maximum again
        assert g.best_hyp == 7


def _resume(ba, p, step, stop_at_hit=True):
    """the hypotheses of p in calls of `step`, carrying best_inliers / best_S12: (results, state)"""
    best, S, out = p.best_inliers, p.best_S12, []
    for o in range(0, p.n_hyp, step):
        g = ba.sim3_ransac([p.copy(sample=p.sample[o:o + step], best_inliers=best, best_S12=S)])[0]
        out.append((o, g))
        best, S = g.best_inliers, g.best_S12
        if g.hit >= 0 and stop_at_hit:
            break
    return out, best, S


@pytest.mark.parametrize("k", [4, 7])           # a late hit (56 of 64), no hit (64 of 64)
def test_one_call_equals_thirteen_calls_of_five(ba, k):
    p = cases.make(cases.CASES[k])
    assert p.n_hyp == 64
    g = ba.sim3_ransac([p])[0]
    parts, best, S = _resume(ba, p, 5)
    o, last = parts[-1]
    if g.hit >= 0:
        assert o + last.hit == g.hit and last.n_inliers == g.n_inliers
        assert last.S12.tobytes() == g.S12.tobytes() and np.array_equal(last.inlier, g.inlier)
    else:
        assert len(parts) == 13 and all(q.hit < 0 for _, q in parts)
    assert sum(q.its_done for _, q in parts) == g.its_done
    assert best == g.best_inliers and S.tobytes() == g.best_S12.tobytes()
    moved = [o + q.best_hyp for o, q in parts if q.best_hyp >= 0]
    assert (moved[-1] if moved else -1) == g.best_hyp
    assert np.array_equal(np.concatenate([q.hyp_inliers for _, q in parts])[:g.its_done], g.hyp_inliers[:g.its_done])


def test_continuing_after_a_hit(ba):
    """the solver's state after a hit blocks every smaller count: the remaining triples are accepted only at c >= the hit's"""
    case = cases.CASES[6]                      # hit at 1 of 64
    p, r = cases.make(case), cases.reference(case)
    g = ba.sim3_ransac([p])[0]
    assert g.hit == r["hit"] == 1
    rest = p.copy(sample=p.sample[g.hit + 1:], best_inliers=g.best_inliers, best_S12=g.best_S12)
    g2 = ba.sim3_ransac([rest])[0]
    c = r["hyp_inliers"][g.hit + 1:]
    assert np.array_equal(g2.hyp_inliers, c)
    assert (g2.hit, g2.its_done, g2.best_hyp, g2.best_inliers) == ref.scan(c, p.min_inliers, g.best_inliers)
    if g2.best_hyp >= 0:
        assert c[g2.best_hyp] >= g.n_inliers
    else:
        assert (c < g.n_inliers).all() and g2.best_S12.tobytes() == g.best_S12.tobytes()


def test_a_batch_equals_single_calls(ba):
    """whatever the position in the batch; the batch mixes n_hyp == 0, n_pairs < min_inliers and ordinary problems"""
    some = [cases.make(cases.CASES[k]) for k in (0, 2, 4, 7, 8, 9)]
    empty = some[2].copy(sample=np.zeros((0, 3), dtype=np.int32), best_inliers=7, best_S12=np.arange(8.0))
    few = cases.make(cases.CASES[3]).copy(min_inliers=40)     # 25 pairs < 40: legal, not short-circuited
    nothing = abi.Sim3RansacProblem(p1c=np.zeros((0, 3)), p2c=np.zeros((0, 3)), max_err1=[], max_err2=[], K1=some[0].K1, K2=some[0].K2,
                                    sample=np.zeros((0, 3), dtype=np.int32))
    batch = [some[3], empty, some[0], few, some[5], nothing, some[1], some[2], some[4]]
    single = [ba.sim3_ransac([p])[0] for p in batch]
    for order in (list(range(len(batch))), list(reversed(range(len(batch))))):
        got = ba.sim3_ransac([batch[i] for i in order])
        for i, g in zip(order, got):
            _same(g, single[i])
    e = single[1]
    assert (e.hit, e.its_done, e.best_hyp, e.best_inliers) == (-1, 0, -1, 7) and np.array_equal(e.best_S12, np.arange(8.0))
    f = single[3]
    assert f.hit == -1 and f.its_done == few.n_hyp and f.best_inliers == ref.ransac(few)["best_inliers"]
    assert (single[5].hit, single[5].its_done) == (-1, 0)
    # without the counts the call copies less back and decides the same
    for g, s in zip(ba.sim3_ransac(batch, want_counts=False), single):
        assert g.hyp_inliers is None and (g.hit, g.best_hyp, g.best_inliers) == (s.hit, s.best_hyp, s.best_inliers)
        assert g.S12.tobytes() == s.S12.tobytes() and np.array_equal(g.inlier, s.inlier)


def test_a_hit_seeds_vba_sim3_optimize(ba):
    case = cases.CASES[11]
    p = cases.make(case)
    g = ba.sim3_ransac([p])[0]
    assert g.hit >= 0
    m = g.inlier.astype(bool)
    pix = lambda K, P: P[:, :2] / P[:, 2:3] * K[:2] + K[2:]
    q = abi.Sim3Problem(S12=g.S12, p1c=p.p1c[m], p2c=p.p2c[m], uv1=pix(p.K1, p.p1c[m]), uv2=pix(p.K2, p.p2c[m]),
                        w1=np.ones(int(m.sum())), w2=np.ones(int(m.sum())), K1=p.K1, K2=p.K2, fix_scale=p.fix_scale)
    r = ba.sim3_optimize([q])[0]
    assert r.status == 0 and r.n_inliers > 0
    assert np.isfinite(r.S12).all()


def test_one_launch_per_call(ba):
    ba.sim3_ransac([cases.make(cases.CASES[k]) for k in (2, 4, 8)])
    assert ba.get_profile()["kernel_launches"] == 1


def test_refusals_and_pending_tickets(ba):
    p = cases.make(cases.CASES[2])
    for bad, msg in ((p.copy(sample=np.array([[0, 1, p.n_pairs]], dtype=np.int32)), "problem 1: hypothesis 0: sample index out of range"),
                     (p.copy(best_inliers=-1), "problem 1: negative best_inliers"),
                     (p.copy(K1=np.array([np.nan, 1, 1, 1])), "problem 1: K1 / K2 is not finite")):
        with pytest.raises(RuntimeError, match=msg):
            ba.sim3_ransac([p, bad])
    w = synth.config_c3(seed=3, n_kf=6, n_pt=120, n_obs=500)
    t = ba.submit([w])
    packed = ba.sim3_ransac_pack([p])
    rc = ba.lib.vba_sim3_ransac(ba.h, packed[0], packed[3], packed[4])
    err = ba.lib.vba_last_error(ba.h).decode()
    ba.wait(t)
    assert rc == -1 and "asynchronous batches pending" in err, (rc, err)
    assert ba.sim3_ransac([p])[0].hit == cases.reference(cases.CASES[2])["hit"]
