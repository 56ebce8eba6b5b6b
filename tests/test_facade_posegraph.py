"""Optimizer::OptimizeEssentialGraph of the host facade: the extraction (vertices, the four edge rules, map-point references) against
its NumPy mirror on the CPU, and on the GPU the whole call against vba_posegraph_optimize on the extracted arrays plus the
reference's write-back (src/Optimizer.cpp:4488-4546)."""
import numpy as np
import pytest

import facade_posegraph_lib as fl
from mc_slam_amd import backend, synth


@pytest.fixture()
def lm():
    m = fl.LoopMap(seed=1, n=30, n_corr=3, n_pt=60)
    yield m
    m.close()


def test_extraction_follows_the_four_edge_rules(lm):
    nv = lm.call(mode=1)
    assert nv == lm.n - 1                                                     # the bad keyframe has no vertex
    p = lm.packed()
    kf_ids, mp_ids = lm.ids()
    assert list(kf_ids) == [k for k in range(lm.n) if k != lm.bad]
    assert p.its == 20 and p.lambda_init == 1e-16 and p.fix_scale == 0
    assert list(np.nonzero(p.fixed)[0]) == [0] and kf_ids[0] == lm.loop_kf
    for v, k in enumerate(kf_ids):
        want = lm.vertex_S(int(k))
        assert np.abs(p.S[v, :3] - want[:3]).max() <= 1e-12 and abs(p.S[v, 7] - want[7]) == 0
        assert min(np.abs(p.S[v, 3:7] - want[3:7]).max(), np.abs(p.S[v, 3:7] + want[3:7]).max()) <= 1e-7
    want = lm.expected_edges()
    got = [(int(kf_ids[i]), int(kf_ids[j]), S) for i, j, S in zip(p.edge_i, p.edge_j, p.edge_S)]
    assert sorted((i, j) for i, j, _ in got) == sorted((i, j) for i, j, _ in want)
    assert (lm.cur_kf, lm.loop_kf) in [(i, j) for i, j, _ in got] and (lm.n - 2, 1) not in [(i, j) for i, j, _ in got]
    assert len([1 for i, j, _ in got if (i, j) == (lm.cur_kf, lm.loop_kf)]) == 2          # LoopConnections and the loop edge
    key = lambda e: (e[0], e[1], round(float(e[2][0]), 6))
    for (i, j, S), (wi, wj, wS) in zip(sorted(got, key=key), sorted(want, key=key)):
        assert (i, j) == (wi, wj)
        assert np.abs(S[:3] - wS[:3]).max() <= 1e-6 and abs(S[7] - wS[7]) <= 1e-9
    # map points: bad ones and those whose reference keyframe has no vertex are left out; corrected ones use mnCorrectedReference
    eff = lambda pid: lm.corrected_pts.get(pid, int(lm.pt_ref[pid]))
    assert list(mp_ids) == [pid for pid in range(60) if pid != 1 and eff(pid) != lm.bad] and 0 not in mp_ids and len(mp_ids) < 59
    for row, pid in enumerate(mp_ids):
        r = lm.corrected_pts.get(int(pid), int(lm.pt_ref[pid]))
        assert kf_ids[p.pt_ref[row]] == r
        assert np.array_equal(p.pt[row], np.float64(lm.pt[pid]))


@pytest.mark.gpu
def test_the_call_equals_the_backend_on_the_extracted_graph_and_writes_back(lm):
    lm.call(mode=1)
    p = lm.packed()
    kf_ids, mp_ids = lm.ids()
    ba = backend.LocalBA(0)
    want = ba.posegraph_optimize([p])[0]
    ba.close()
    before = {k: lm.pose(k) for k in range(lm.n)}
    assert lm.L.fc_loop_map_updated(lm.m) == 0
    lm.call(mode=0)
    assert lm.L.fc_loop_map_updated(lm.m) == 1
    R = lm.L.fc_last_posegraph_result().contents
    assert (R.its_done, R.lm_trials, R.stop) == (want.its_done, want.lm_trials, want.stop) and R.chi2_final == want.chi2_final
    assert np.array_equal(lm.packed().S, want.S) and np.array_equal(lm.packed().pt, want.pt)
    moved = 0
    for v, k in enumerate(kf_ids):
        nav, T = lm.pose(int(k))
        S = want.S[v]
        Tw = np.eye(4, dtype=np.float32)
        Tw[:3, :3] = np.float32(synth.quat_to_rot(S[3:7] / np.linalg.norm(S[3:7])))
        Tw[:3, 3] = np.float32(S[:3] * (1.0 / S[7]))
        assert np.abs(T - Tw).max() <= 2e-7 * max(1.0, np.abs(Tw).max())                  # Tiw = [R, t / s] in float32
        # UpdateNavStatePVRFromTcw (src/KeyFrame.cpp:19-36): Twb = (Tbc Tcw)^-1
        Rbw, tbw = lm.R_bc @ np.float64(T[:3, :3]), lm.R_bc @ np.float64(T[:3, 3]) + lm.p_bc
        Rwb, Pwb = Rbw.T, -Rbw.T @ tbw
        assert np.abs(nav[:3] - Pwb).max() <= 1e-5 and np.abs(synth.quat_to_rot(nav[3:7]) - Rwb).max() <= 1e-6
        assert abs(np.linalg.norm(nav[7:10]) - np.linalg.norm(before[int(k)][0][7:10])) <= 1e-6     # the body-frame velocity is kept
        moved += int(np.abs(T - before[int(k)][1]).max() > 1e-4)
    assert moved > lm.n // 2
    assert np.array_equal(lm.pose(lm.bad)[1], before[lm.bad][1])                          # no vertex: untouched
    for row, pid in enumerate(mp_ids):
        P, n_upd = lm.point(int(pid))
        assert np.array_equal(P, np.float32(want.pt[row])) and n_upd == 1
    for pid in [q for q in range(60) if q not in mp_ids]:
        P, n_upd = lm.point(pid)
        assert np.array_equal(P, lm.pt[pid]) and n_upd == 0
