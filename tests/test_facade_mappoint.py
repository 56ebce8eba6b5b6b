"""The map-point refresh of the host facade (mc_slam_amd/host/MapPointUpdate.cpp): UpdateMapPoints and the two LocalMapping loops,
ProcessNewKeyFramePoints (src/LocalMapping.cpp:1144-1171) and UpdateCurrentKeyFramePoints (:1635-1650), on the mock map of
tests/facade_mappoint_lib.py against tests/mappoint_ref.py.

The facade narrows the backend's float64 answer to float32.  The backend is within mappoint_cases.NORMAL_TOL / DIST_TOL of the
float64 yardstick (tests/test_gpu_mappoint.py), far below half a float32 spacing, so the two narrowed values are equal or neighbours:
normal, mfMinDistance and mfMaxDistance are compared within one float32 spacing of the narrowed yardstick, mDescriptor for equality."""
import numpy as np
import pytest

import facade_mappoint_lib as fm
import mappoint_ref as ref_mod

f32 = np.float32


@pytest.fixture()
def mock():
    m = fm.MockMap()
    yield m
    m.close()


def check(mock, ids, what=3):
    """the attributes of the points `ids` against the yardstick on the mirror; returns the yardstick's states"""
    w = ref_mod.mappoint_ref(mock.problem(ids, what))
    for i, p in enumerate(ids):
        a = mock.attributes(p)
        assert (a["normal_updates"], a["desc_updates"]) == (0, 0), p            # the stubs' counters are not touched
        assert a["n_observations"] == len(mock.obs[p]), p
        if what & 1 and w["desc_state"][i] == 0:
            assert np.array_equal(a["desc"], w["desc"][i]), p
        if what & 2 and w["normal_state"][i] == 0:
            n, mx, mn = w["normal"][i].astype(f32), f32(w["dist_max"][i]), f32(w["dist_min"][i])
            assert (np.abs(a["normal"] - n) <= np.spacing(np.abs(n))).all(), (p, a["normal"], n)
            assert abs(a["max"] - mx) <= np.spacing(mx) and abs(a["min"] - mn) <= np.spacing(mn), p
    return w


def untouched(mock, p):
    a = mock.attributes(p)
    return not a["normal"].any() and (a["min"], a["max"]) == (0, 0) and not a["desc"].any() and (a["normal_updates"], a["desc_updates"]) == (0, 0)


def test_refusals_need_no_backend(mock, capfd):
    """a bit of `what` outside the two parts is refused; an empty list, a list of NULL and bad points and what = 0 are done at once"""
    capfd.readouterr()
    assert mock.update_map_points([100, 102], 4) == -1
    assert capfd.readouterr().err.strip() == "UpdateMapPoints: what has a bit outside VBA_MAPPOINT_DESC | VBA_MAPPOINT_NORMAL"
    assert mock.update_map_points([], 3) == 0 and mock.update_map_points([None, 101, None], 3) == 0 and mock.update_map_points([100, 104], 0) == 0
    assert all(untouched(mock, p) for p in mock.ids)


@pytest.mark.gpu
def test_process_new_keyframe_points(mock):
    """the AddObservations in keypoint order, the recent list, ONE call for the new observers: the duplicated point 100 is refreshed
    once and listed once, the bad point 101 is skipped, point 103 (already in the keyframe) is listed and not refreshed, point 102
    reads keypoint 0 of its reference keyframe"""
    upd, recent = mock.mirror_process_new_keyframe()
    ret, got_recent = mock.process_new_keyframe_points()
    assert ret == len(upd) > 15 and got_recent == recent and recent == [103, 100]
    assert 100 in upd and 102 in upd and 101 not in upd and upd.count(100) == 1
    w = check(mock, upd)
    assert (w["desc_state"] == 0).all() and (w["normal_state"] == 0).all() and w["n_desc"].min() >= 1
    assert any(fm.BAD_KF in mock.obs[p] for p in upd)                           # the bad keyframe: out of a descriptor set, in the normal
    i = upd.index(102)
    assert mock.ref[102] not in mock.obs[102] and mock.problem(upd).ref_scale[i] == float(fm.SCALE[6])
    for p in mock.ids:
        if p not in upd:
            assert untouched(mock, p), p
    assert mock.attributes(101)["n_observations"] == len(mock.seen[101])        # no observation added to the bad point


@pytest.mark.gpu
def test_update_current_keyframe_points(mock):
    """after ProcessNewKeyFramePoints: every good point of the current keyframe, the recent ones included, in ONE call"""
    upd, recent = mock.mirror_process_new_keyframe()
    assert mock.process_new_keyframe_points()[0] == len(upd)
    pts = [p for p in mock.cur_points if p is not None and p not in mock.bad]
    assert mock.update_current_keyframe_points() == len(pts) == len(upd) + 2
    check(mock, sorted(set(pts)))
    assert not untouched(mock, 103) and untouched(mock, 101)


@pytest.mark.gpu
def test_update_map_points_one_part(mock):
    """what = VBA_MAPPOINT_NORMAL, the form of a BA write-back: the descriptor stays as it was; then the descriptor part alone"""
    ids = [104, 105, None, 101, 106, 102]
    good = [104, 105, 106, 102]
    assert mock.update_map_points(ids, 2) == len(good)
    check(mock, good, 2)
    assert all(not mock.attributes(p)["desc"].any() for p in good) and untouched(mock, 101)
    before = {p: mock.attributes(p) for p in good}
    assert mock.update_map_points(ids, 1) == len(good)
    w = check(mock, good, 1)
    assert w["desc_state"].tolist() == [0, 0, 3, 0]                             # point 106 is seen by the bad keyframe alone: nothing is written
    for i, p in enumerate(good):
        a = mock.attributes(p)
        assert a["desc"].any() == (w["desc_state"][i] == 0) and np.array_equal(a["normal"], before[p]["normal"]) and (a["min"], a["max"]) == (before[p]["min"], before[p]["max"])
