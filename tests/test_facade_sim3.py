"""Optimizer::OptimizeSim3 of the host facade against tests/sim3_ref.py fed with the NumPy mirror of the facade's extraction
(float32 camera-frame points, the reference's pair filters)."""
import ctypes as C

import numpy as np
import pytest

import facade_sim3_lib
import sim3_ref
from mc_slam_amd import synth

_pd = C.POINTER(C.c_double)


def _quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def test_g2o_sim3_members_against_the_reference_restatement():
    """map, inverse and operator* of the minimal g2o::Sim3 (the members LoopClosing uses); no GPU involved"""
    L = facade_sim3_lib.lib()
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.normal(size=3), _quat(rng), [1.3]])
    b = np.concatenate([rng.normal(size=3), _quat(rng), [0.7]])
    x = rng.normal(size=3)
    out = np.zeros(19)
    L.fc_sim3_ops(a.ctypes.data_as(_pd), b.ctypes.data_as(_pd), x.ctypes.data_as(_pd), out.ctypes.data_as(_pd))
    A, B = (a[3:7], a[:3], a[7]), (b[3:7], b[:3], b[7])
    np.testing.assert_allclose(out[:3], A[2] * (sim3_ref.q2R(A[0]) @ x) + A[1], atol=1e-14)
    q, t, s = sim3_ref.sim3_mul(A, B)
    np.testing.assert_allclose(out[11:19], np.concatenate([t, q, [s]]), atol=1e-14)
    inv = (out[6:10], out[3:6], out[10])
    q, t, s = sim3_ref.sim3_mul(A, inv)                        # a * a.inverse() = identity
    assert np.abs(t).max() <= 1e-14 and abs(s - 1) <= 1e-15 and np.abs(sim3_ref.q2R(q) - np.eye(3)).max() <= 1e-14


@pytest.mark.gpu
@pytest.mark.parametrize("fix", [False, True])
def test_optimize_sim3_matches_the_reference_on_the_extracted_pairs(fix):
    p = synth.make_sim3_pair(41 + int(fix), 150, fix_scale=fix, outlier_frac=0.15)
    P = facade_sim3_lib.Sim3Pair(p, seed=3)
    try:
        e = P.extracted()
        assert e.n_pairs == 150
        r = sim3_ref.optimize(e, trace=True)
        margin = sim3_ref.gate_margin(r, e.th2)
        print("reference: inliers", r.n_inliers, "n_bad_stage1", r.n_bad_stage1, "gate margin %.2e" % margin)
        assert margin > 1e-6 and r.n_inliers >= 20
        n, m, S = P.optimize()
        assert n == r.n_inliers
        rows = P.rows_of_pairs()
        want = P.matches.copy()
        want[rows[r.outlier != 0]] = -1                          # nulled: the flagged pairs and nothing else
        assert np.array_equal(m, want)
        assert all(m[k] == P.matches[k] for k in P.special_rows)  # the entries the filters skip stay as they were
        dt = np.abs(S[:3] - r.S12[:3]).max()
        dq = min(np.abs(S[3:7] - r.S12[3:7]).max(), np.abs(S[3:7] + r.S12[3:7]).max())
        ds = abs(S[7] - r.S12[7]) / r.S12[7]
        print("|dt| %.2e |dq| %.2e |ds|/s %.2e" % (dt, dq, ds))
        assert dt <= 1e-6 and dq <= 1e-7 and ds <= 1e-7
        if fix:
            assert S[7].tobytes() == p.S12[7].tobytes()
    finally:
        P.close()


@pytest.mark.gpu
def test_fewer_than_ten_survivors_returns_zero_and_leaves_g2oS12():
    p = synth.make_sim3_pair(43, 16, outlier_frac=0.0)
    p.uv1[:9] += 60.0
    P = facade_sim3_lib.Sim3Pair(p, seed=4)
    try:
        r = sim3_ref.optimize(P.extracted())
        assert r.n_inliers == 0 and r.n_bad_stage1 >= 7
        n, m, S = P.optimize()
        assert n == 0 and S.tobytes() == p.S12.tobytes()
        want = P.matches.copy()
        want[P.rows_of_pairs()[r.outlier != 0]] = -1             # vpMatches1 entries are nulled also when 0 is returned
        assert np.array_equal(m, want)
    finally:
        P.close()
