"""Both ORBmatcher::SearchByProjection overloads of the tracking thread, Tracking::SearchLocalPoints and the matching half of
Tracking::TrackWithMotionModel (mc_slam_amd/host/ORBmatcher.cpp, Tracking.cpp) on the mock frame and map of
tests/facade_tracking_lib.py, against a sequential Python restatement of the whole functions around tests/search_proj_ref.py: the
frame's mvpMapPoints by id, the return values, the mTrack* members, the mnVisible counts and the retry with twice the radius."""
import numpy as np
import pytest

import facade_tracking_lib as ftl
import search_proj_ref as ref_mod
from mc_slam_amd import abi, synth

LAST, LOCAL = abi.SEARCH_PROJ_LAST_FRAME, abi.SEARCH_PROJ_LOCAL_MAP


def _scene(mode, seed=61, n_keys=150, n_q=320, **kw):
    return ftl.TrackingScene(synth.search_proj_scene(seed, mode, n_keys=n_keys, n_q=n_q, twins=0.5, **kw), seed)


def _ref(q):
    w = ref_mod.search_proj_ref(q)
    assert w["margin"] >= 1e-9 and w["margin_r"] >= 1e-9
    return w


def test_refusals_write_nothing(capfd):
    """bMono == false and a stereo keypoint are refused before anything is packed, as Fuse does (CPU only)"""
    s = _scene(LAST, n_keys=40, n_q=30)
    try:
        before = s.frame_points()
        assert s.L.fc_search_by_projection_last(s.m, ftl.CUR, ftl.LAST, 15.0, 0, 1) == -1
        assert "bMono is false" in capfd.readouterr().err
        s.L.fc_frame_set_uright(s.m, ftl.CUR, 3, 120.0)
        assert s.L.fc_search_by_projection_last(s.m, ftl.CUR, ftl.LAST, 15.0, 1, 1) == -1
        assert "stereo keypoint" in capfd.readouterr().err
        ids = s.query_ids()
        assert s.L.fc_search_by_projection_map(s.m, ftl.CUR, ids.ctypes.data_as(ftl._pl), len(ids), 3.0, 0.8) == -1
        assert "stereo keypoint" in capfd.readouterr().err
        assert np.array_equal(s.frame_points(), before)
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("check_ori", [1, 0])
def test_last_frame_overload(check_ori):
    s = _scene(LAST)
    try:
        before = s.frame_points()
        assert (before >= ftl.OLD).sum() > 20
        want = _ref(s.problem(check_orientation=bool(check_ori)))
        got = s.L.fc_search_by_projection_last(s.m, ftl.CUR, ftl.LAST, 15.0, 1, check_ori)
        assert got == want["n_matches"] > 30
        assert np.array_equal(s.frame_points(), s.expected_points(want, before))
        if check_ori:
            assert want["n_before_filter"] > want["n_matches"] and (want["key_match"] == -2).sum() > 0
        # an old point without observations was overwritten, one with observations never
        over = (before >= ftl.OLD) & (want["key_match"] >= 0)
        assert over.sum() > 0 and not s.p.occupied[over].any()
    finally:
        s.close()


@pytest.mark.gpu
def test_local_map_overload():
    """the overload reads mbTrackInView: a point out of view or bad is skipped; the others get their mTrack* members from the fused
    isInFrustum"""
    s = _scene(LOCAL, noise=3.0)
    try:
        ids = s.query_ids()
        skip = s.p.q_skip.astype(bool).copy()
        skip[5::9] = True
        for i in range(s.p.n_q):
            s.set_track(ftl.QUERY + i, 2 if s.p.q_blocks[i] else 0, not skip[i])
        s.L.fc_set_mappoint_bad(s.m, ftl.QUERY + 11, 1)
        skip[11] = True
        before = s.frame_points()
        want = _ref(s.problem(skip=skip.astype(np.uint8), th=3.0))
        got = s.L.fc_search_by_projection_map(s.m, ftl.CUR, ids.ctypes.data_as(ftl._pl), len(ids), 3.0, 0.8)
        assert got == want["n_matches"] > 30
        assert np.array_equal(s.frame_points(), s.expected_points(want, before))
        s.check_track_fields(want, skip)
        assert set(want["state"]) >= {0, 1, 7, 8, 9}
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("last_reloc,th", [(0, 1.0), (ftl.CUR - 1, 5.0)])
def test_search_local_points(last_reloc, th):
    """step 1 marks the frame's own points (a bad one leaves the frame and its keypoint is free again), step 2 skips them and the bad
    ones, counts nToMatch and mnVisible, and searches with th = 1, or 5 directly behind a relocalisation"""
    s = _scene(LOCAL, noise=3.0)                                # 3 pixels of noise per level scale: th = 1 loses matches that th = 5 finds
    try:
        p = s.p
        before = s.frame_points()
        held = before[before >= 0]
        bad_old = held[::7]                                            # bad points the frame still holds
        for pid in bad_old:
            s.L.fc_set_mappoint_bad(s.m, int(pid), 1)
        s.L.fc_set_mappoint_bad(s.m, ftl.QUERY + 4, 1)
        for k, i in enumerate(np.nonzero(p.q_skip)[0]):                # the scene's skipped queries: bad, or seen by this frame already
            if k % 2:
                s.L.fc_set_mappoint_bad(s.m, ftl.QUERY + int(i), 1)
            else:
                s.set_track(ftl.QUERY + i, 2 if p.q_blocks[i] else 0, 0, last_seen=ftl.CUR)
        local = np.concatenate([s.query_ids(), held[1::2]])           # the local map also lists points the frame already holds
        # the restatement: step 1
        after1 = before.copy()
        after1[np.isin(before, bad_old)] = -1
        occupied = p.occupied.copy()
        occupied[np.isin(before, bad_old)] = 0
        skip = p.q_skip.astype(bool).copy()
        skip[4] = True
        want = _ref(s.problem(occupied=occupied, skip=skip.astype(np.uint8), th=th))
        n_to_match = int(np.isin(want["state"], ftl.IN_VIEW_LOCAL).sum())
        got = s.L.fc_search_local_points(s.m, ftl.CUR, local.ctypes.data_as(ftl._pl), len(local), last_reloc)
        assert got == n_to_match > 50
        # the radius factor matters in this scene: the other value of th gives another answer
        other = _ref(s.problem(occupied=occupied, skip=skip.astype(np.uint8), th=6.0 - th))
        assert not np.array_equal(other["key_match"], want["key_match"])
        assert np.array_equal(s.frame_points(), s.expected_points(want, after1))
        s.check_track_fields(want, skip)
        # mnVisible starts at 1: the frame's good points and the points in view gained one, nobody else
        for pid in held:
            t = s.track_state(pid)
            good = pid not in bad_old
            assert (t[5], t[6], t[0]) == ((2, ftl.CUR, 0) if good else (1, 0, 0)), pid
        for i in range(p.n_q):
            assert s.track_state(ftl.QUERY + i)[5] == (2 if (not skip[i] and want["state"][i] in ftl.IN_VIEW_LOCAL) else 1), i
        assert want["n_matches"] > 20
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_q,retry", [(320, False), (24, True)])
def test_track_with_motion_model_matches(n_q, retry):
    """mvpMapPoints is filled with NULL, so nothing is occupied; fewer than 20 matches bring the second search with th = 30"""
    s = _scene(LAST, seed=63, n_q=n_q, noise=12.0)             # 12 pixels of noise per level scale: the radius decides
    try:
        nothing = np.zeros(s.p.n_keys, dtype=np.uint8)
        first = _ref(s.problem(occupied=nothing, th=15.0, check_orientation=True))
        assert (first["n_matches"] < 20) == retry
        want = _ref(s.problem(occupied=nothing, th=30.0, check_orientation=True)) if retry else first
        got = s.L.fc_track_motion_model_matches(s.m, ftl.CUR, ftl.LAST)
        assert got == want["n_matches"]
        assert np.array_equal(s.frame_points(), s.expected_points(want, np.full(s.p.n_keys, -1)))
        if retry:
            assert not np.array_equal(first["key_match"], want["key_match"])
    finally:
        s.close()
