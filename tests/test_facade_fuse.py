"""Both ORBmatcher::Fuse overloads and LocalMapping::SearchInNeighbors (mc_slam_amd/host/ORBmatcher.cpp, LocalMapping.cpp) on the mock
map of tests/facade_fuse_lib.py, against its sequential Python restatement of the whole functions, apply loop included: the return
value, every keyframe's mvpMapPoints by id, every point's observations, nObs, bad flag, replaced-by pointer, descriptor updates and
whether the map still lists it."""
import numpy as np
import pytest

import facade_fuse_lib as ffl
from mc_slam_amd import abi


@pytest.fixture()
def scene():
    s = ffl.FuseScene()
    yield s
    s.close()


def _same_state(s):
    mvp_f, pts_f = s.facade_state()
    mvp_m, pts_m = s.mirror_state()
    for k in ffl.KFS:
        assert mvp_f[k] == mvp_m[k], k
    for pid in pts_m:
        assert pts_f[pid] == pts_m[pid], pid


def test_grid_and_initial_state(scene):
    """the facade's grid is the one of abi.grid_csr (what the restatement searches), and the mirror starts equal to the map (CPU only)"""
    for k in ffl.KFS:
        begin, feat, inv = scene.grid(k)
        p = scene.problem(k, *scene.pose(k), [], 3.0, True)
        assert np.array_equal(begin, p.cell_begin) and np.array_equal(feat, p.cell_feat) and (float(inv[0]), float(inv[1])) == (p.grid_inv_w, p.grid_inv_h)
        assert len(feat) <= p.n_keys and len(feat) > 150
    _same_state(scene)
    assert len(scene.pts) > 300 and sum(p.n_obs >= 3 for p in scene.pts.values()) > 20 and sum(p.n_obs == 1 for p in scene.pts.values()) > 20


def test_stereo_keyframes_are_refused(scene, capfd):
    """the backend is monocular: a keyframe with one stereo keypoint fails both overloads before anything is packed (CPU only)"""
    scene.L.fc_kf_set_uright(scene.m, 3, 7, 12.5)
    assert scene.fuse(3, [i for i in scene.mvp[1] if i is not None]) == -1
    assert "stereo keypoint" in capfd.readouterr().err
    assert scene.fuse_sim3(3, scene.T[3], [i for i in scene.mvp[1] if i is not None], 4.0)[0] == -1
    _same_state(scene)


@pytest.mark.gpu
def test_fuse_equals_the_restatement(scene):
    """the points of keyframe 1 into keyframe 3, with a point listed twice, a NULL entry and a bad point"""
    ids = list(scene.mvp[1])
    good = [i for i in ids if i is not None]
    ids = ids + [good[3], good[10]]
    scene.L.fc_set_mappoint_bad(scene.m, good[5], 1); scene.pts[good[5]].bad = True
    assert None in ids
    want, counts = scene.ref_fuse(3, ids)
    print("Fuse: %d fused  %s" % (want, counts))
    assert scene.fuse(3, ids) == want
    assert want >= 40 and counts["add"] > 0 and counts["keep_in_kf"] > 0 and counts["keep_new"] > 0 and counts["skipped_live"] > 0
    _same_state(scene)


@pytest.mark.gpu
def test_fuse_sim3_equals_the_restatement(scene):
    """the points of the keyframes 1 and 5 into keyframe 4 under Scw = 1.1 * Tcw: the decomposition gives the pose back"""
    ids = [i for i in scene.mvp[1] + scene.mvp[5] if i is not None]
    S = scene.T[4].copy()
    S[:3, :] *= np.float32(1.1)
    want, rep = scene.ref_fuse_sim3(4, S, ids, 4.0)
    n, got = scene.fuse_sim3(4, S, ids, 4.0)
    print("Fuse (Sim3): %d fused, %d to replace" % (want, sum(r is not None for r in rep)))
    assert n == want and got == rep
    assert want >= 40 and sum(r is not None for r in rep) > 10 and sum(r is None for r in rep) > 10
    _same_state(scene)


@pytest.mark.gpu
def test_search_in_neighbors_equals_the_restatement(scene):
    want, counts, cand = scene.ref_search_in_neighbors(1, [2, 3, 4, 5])
    print("SearchInNeighbors: %d fused  %s  %d candidates" % (want, counts, len(cand)))
    assert scene.search_in_neighbors(1, [2, 3, 4, 5]) == want
    assert want >= 150 and min(counts.values()) > 0
    _same_state(scene)
    assert sum(p.bad for p in scene.pts.values()) > 50 and sum(p.n_desc for p in scene.pts.values()) > 50
