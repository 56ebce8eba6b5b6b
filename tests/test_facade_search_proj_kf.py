"""The loop-closure and the relocalisation overload of ORBmatcher::SearchByProjection and LoopClosing::MatchLoopMapPoints
(mc_slam_amd/host/ORBmatcher.cpp, LoopClosing.cpp) on the mock map of tests/facade_search_proj_kf_lib.py, against a sequential Python
restatement around tests/search_proj_kf_ref.py: vpMatched and the frame's mvpMapPoints by id, the return values, the gathered loop
points and the decision at 40 matches."""
import numpy as np
import pytest

import facade_search_proj_kf_lib as fkl
import search_proj_kf_ref as ref_mod
from mc_slam_amd import synth

LOOP, RELOC = fkl.LOOP, fkl.RELOC


def _scene(mode, seed=61, n_keys=150, n_q=320, scale=1.0, **kw):
    return fkl.KfScene(synth.search_proj_kf_scene(seed, mode, n_keys=n_keys, n_q=n_q, twins=0.5, **kw), scale)


def _ref(q):
    w = ref_mod.search_proj_kf_ref(q)
    assert w["margin"] >= 1e-9 and w["margin_r"] >= 1e-9
    return w


def test_refusals_write_nothing(capfd):
    """a vpMatched of the wrong size and a stereo keypoint are refused before anything is packed, as the siblings do (CPU only)"""
    s = _scene(LOOP, n_keys=40, n_q=30)
    try:
        ids = (fkl.QUERY + np.arange(30)).astype(np.int64)
        short = s.initial[:-1].copy()
        assert s.L.fc_search_by_projection_loop(s.m, fkl.TGT, np.ascontiguousarray(s.Scw).ctypes.data_as(fkl._pf), ids.ctypes.data_as(fkl._pl), 30,
                                                short.ctypes.data_as(fkl._pl), len(short), 10) == -1
        assert "vpMatched does not have one entry per keypoint" in capfd.readouterr().err
        assert np.array_equal(short, s.initial[:-1])
        s.L.fc_kf_set_uright(s.m, fkl.TGT, 3, 120.0)
        r, matched = s.loop_call()
        assert r == -1 and "stereo keypoint" in capfd.readouterr().err and np.array_equal(matched, s.initial)
    finally:
        s.close()
    s = _scene(RELOC, n_keys=40, n_q=30)
    try:
        s.L.fc_frame_set_uright(s.m, fkl.TGT, 3, 120.0)
        r, pts = s.reloc_call(10.0, 100)
        assert r == -1 and "stereo keypoint" in capfd.readouterr().err and np.array_equal(pts, s.initial)
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 1.7])
def test_loop_overload(scale):
    """Scw carries a scale: the overload divides it out as :364-368 do; the already-found set is the one of the start"""
    s = _scene(LOOP, scale=scale)
    try:
        assert len(s.found) > 2 and (s.initial >= fkl.OLD).sum() > 5
        want = _ref(s.problem())
        got, matched = s.loop_call()
        assert got == want["n_matches"] > 30
        assert np.array_equal(matched, s.expected_points(want, s.initial))
        assert set(want["state"]) >= {0, 1, 2, 3, 4, 5, 7, 8}
        # a keypoint taken at the start was never given away
        assert np.array_equal(matched[s.initial >= 0], s.initial[s.initial >= 0])
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("th,orb_dist,check_ori", [(10.0, 100, 1), (3.0, 64, 1), (10.0, 100, 0)])
def test_reloc_overload(th, orb_dist, check_ori):
    """the two calls of Tracking::Relocalization, (10, 100) and (3, 64), and one without the orientation filter"""
    s = _scene(RELOC)
    try:
        assert len(s.found) > 2 and len(s.none) > 0
        want = _ref(s.problem(th=th, th_dist=orb_dist, check_orientation=bool(check_ori), angle=s.angle, q_angle=s.q_angle))
        got, pts = s.reloc_call(th, orb_dist, check_ori)
        assert got == want["n_matches"] > 30
        assert np.array_equal(pts, s.expected_points(want, s.initial))
        if check_ori:
            assert want["n_before_filter"] > want["n_matches"] and (want["key_match"] == -2).sum() > 0
        # a point behind the camera matched
        behind = s.p.truth["behind"]
        assert np.isin(want["state"][behind], (0, 7)).sum() > 0
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_keys,n_q,accepted", [(150, 320, True), (40, 30, False)])
def test_match_loop_map_points(n_keys, n_q, accepted):
    """the loop points are gathered from the covisible keyframes 4 and 5 and then from the matched keyframe 3, every good point once
    (a point shared by the keyframes 4 and 3 stands where keyframe 4 holds it); one call with th = 10; the decision at 40"""
    s = _scene(LOOP, n_keys=n_keys, n_q=n_q, occupied=0.05)
    try:
        L, p = s.L, s.p
        # the already-found queries of the scene's mock stand in vpMatched; here that is the start of mvpCurrentMatchedPoints
        holders = {4: [i for i in range(n_q) if i % 3 == 0], 5: [i for i in range(n_q) if i % 3 == 1], 3: [i for i in range(n_q) if i % 3 == 2]}
        shared = holders[4][::5]
        holders[3] = shared[:len(shared) // 2] + holders[3] + shared[len(shared) // 2:]
        for kf in (3, 4, 5):
            L.fc_add_keyframe(s.m, kf, s.d(s.nav), s.d(p.K), -1, 0)
            for j, i in enumerate(holders[kf]):
                L.fc_kf_add_keypoint(s.m, kf, fkl.QUERY + i, float(j), 1.0, 0, 1)
                if j % 11 == 0:
                    L.fc_kf_add_keypoint(s.m, kf, -1, float(j), 2.0, 0, 1)     # a keypoint without a point
        cov = np.array([4, 5], dtype=np.int64)
        L.fc_set_covisible(s.m, 3, cov.ctypes.data_as(fkl._pl), 2)
        bad = s.skip & ~np.isin(np.arange(n_q), s.found)                       # bad points are not gathered at all
        order = [i for i in holders[4] + holders[5] + [i for i in holders[3] if i not in shared] if not bad[i]]
        assert len(set(order)) == len(order) and len(shared) > 1
        o = np.array(order, dtype=np.int64)
        q = s.problem(q_pos=p.q_pos[o], q_desc=p.q_desc[o], q_normal=p.q_normal[o], q_skip=s.skip[o].astype(np.uint8), q_dist_min=s.dist_min[o],
                      q_dist_max=s.dist_max[o], q_pred_max=s.pred_max[o].astype(np.float64))
        want = _ref(q)
        matched = s.initial.copy()
        loop_ids = np.full(n_q + 8, -7, dtype=np.int64)
        out3 = np.zeros(3, dtype=np.int32)
        assert L.fc_match_loop_map_points(s.m, fkl.TGT, 3, np.ascontiguousarray(s.Scw).ctypes.data_as(fkl._pf), matched.ctypes.data_as(fkl._pl), len(matched),
                                          loop_ids.ctypes.data_as(fkl._pl), len(loop_ids), out3.ctypes.data_as(fkl._pi)) == 0
        assert out3[2] == len(order) and np.array_equal(loop_ids[:len(order)], fkl.QUERY + o) and (loop_ids[len(order):] == -7).all()
        assert np.array_equal(matched, s.expected_points(want, s.initial, ids=fkl.QUERY + o))
        total = int((s.initial >= 0).sum()) + want["n_matches"]
        assert (out3[0], out3[1]) == (int(accepted), total) and (total >= 40) == accepted and want["n_matches"] > 0
    finally:
        s.close()
