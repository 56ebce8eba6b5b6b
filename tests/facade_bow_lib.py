"""ctypes harness for the bag-of-words matchers of the host facade (both ORBmatcher::SearchByBoW overloads, their batch forms and the
matching half of Tracking::TrackReferenceKeyFrame: mc_slam_amd/host/ORBmatcher.cpp, Tracking.cpp, through the fc_* hooks), and a mock
map built from synthetic pairs (mc_slam_amd.synth.search_bow_scene).

The mock: every side of every pair is a keyframe or a frame of its own with the side's keypoints, descriptors, angles and feature
vector.  Keypoint i of keyframe K holds map point 10000 K + i where the side's flag says "good"; every fifth other keypoint holds a
map point that is bad (the matcher must treat it like none), the rest hold none.  The keypoints of a frame hold no points."""
import ctypes as C

import numpy as np

import facade_tracking_lib
from mc_slam_amd import abi

_pd = C.POINTER(C.c_double)
_pf = C.POINTER(C.c_float)
_pl = C.POINTER(C.c_long)
_pi = C.POINTER(C.c_int)
_pu8 = C.POINTER(C.c_uint8)
_pu32 = C.POINTER(C.c_uint32)
f32 = np.float32
K = np.array([458.0, 457.0, 367.0, 248.0])


def lib():
    L = facade_tracking_lib.lib()
    L.fc_kf_set_matcher_data.argtypes = [C.c_void_p, C.c_long, _pu8, _pf, C.c_int, _pu32, _pi, _pi]
    L.fc_frame_set_bow_data.argtypes = [C.c_void_p, C.c_long, _pu8, _pf, C.c_int, _pu32, _pi, _pi]
    L.fc_mp_set_bad.argtypes = [C.c_void_p, C.c_long, C.c_int]
    L.fc_search_by_bow_frame.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_float, C.c_int, _pl, C.c_int]
    L.fc_search_by_bow_kf.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_float, C.c_int, _pl, C.c_int]
    L.fc_search_by_bow_batch.argtypes = [C.c_void_p, C.c_long, C.c_long, _pl, C.c_int, C.c_float, C.c_int, _pl, C.c_int, _pi]
    L.fc_track_reference_kf_matches.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_long]
    L.fc_frame_get.argtypes = [C.c_void_p, C.c_long, _pd, _pf, _pd, _pd, _pu8, C.c_int]
    return L


class BowMap:
    def __init__(self):
        self.L = lib()
        self.m = self.L.fc_create()
        self.n = {}
        self.nav = np.zeros(22)
        self.nav[6] = 1.0
        self._d = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_pd)

    def close(self):
        self.L.fc_destroy(self.m)

    def _bow_args(self, desc, angle, ids, begin, feat):
        self._keep = (np.ascontiguousarray(desc), np.ascontiguousarray(angle, dtype=f32), np.ascontiguousarray(ids, dtype=np.uint32),
                      np.ascontiguousarray(begin, dtype=np.int32), np.ascontiguousarray(feat, dtype=np.int32))
        d, a, i, b, f = self._keep
        return d.ctypes.data_as(_pu8), a.ctypes.data_as(_pf), len(i), i.ctypes.data_as(_pu32), b.ctypes.data_as(_pi), f.ctypes.data_as(_pi)

    def add_keyframe(self, kf, desc, good, angle, ids, begin, feat):
        """a keyframe with one keypoint per descriptor row; returns the good flags as the facade must see them"""
        L, n = self.L, len(desc)
        assert L.fc_add_keyframe(self.m, kf, self._d(self.nav), self._d(K), -1, 0) == 0
        zero3 = np.zeros(3, dtype=f32)
        other = 0
        for i in range(n):
            pid = -1
            if good[i] or (other := other + 1) % 5 == 0:
                pid = 10000 * kf + i
                assert L.fc_add_mappoint(self.m, pid, zero3.ctypes.data_as(_pf), kf) == 0
                if not good[i]:
                    L.fc_mp_set_bad(self.m, pid, 1)
            assert L.fc_kf_add_keypoint(self.m, kf, pid, float(i), 1.0, 0, 1) == i
        assert L.fc_kf_set_matcher_data(self.m, kf, *self._bow_args(desc, np.zeros(n) if angle is None else angle, ids, begin, feat)) == n
        self.n[kf] = n

    def add_frame(self, fr, desc, angle, ids, begin, feat):
        L, n = self.L, len(desc)
        L.fc_add_frame(self.m, fr, self._d(self.nav), self._d(K))
        for i in range(n):
            L.fc_frame_add_obs(self.m, fr, -1, float(i), 1.0, 0)
        assert L.fc_frame_set_bow_data(self.m, fr, *self._bow_args(desc, np.zeros(n) if angle is None else angle, ids, begin, feat)) == n
        self.n[fr] = n

    def add_side1(self, kf, p: abi.SearchBowProblem):
        self.add_keyframe(kf, p.desc1, p.good_mp1, p.angle1, p.node_id1, p.node_begin1, p.node_feat1)

    def add_side2(self, ident, p: abi.SearchBowProblem):
        if p.kf_kf:
            self.add_keyframe(ident, p.desc2, p.good_mp2, p.angle2, p.node_id2, p.node_begin2, p.node_feat2)
        else:
            self.add_frame(ident, p.desc2, p.angle2, p.node_id2, p.node_begin2, p.node_feat2)

    def search_frame(self, kf, fr, nnratio, check_ori):
        ids = np.full(max(self.n[fr], 1), -7, dtype=np.int64)
        r = self.L.fc_search_by_bow_frame(self.m, kf, fr, nnratio, int(check_ori), ids.ctypes.data_as(_pl), len(ids))
        return r, ids[:self.n[fr]]

    def search_kf(self, kf1, kf2, nnratio, check_ori):
        ids = np.full(max(self.n[kf1], 1), -7, dtype=np.int64)
        r = self.L.fc_search_by_bow_kf(self.m, kf1, kf2, nnratio, int(check_ori), ids.ctypes.data_as(_pl), len(ids))
        return r, ids[:self.n[kf1]]

    def search_batch(self, kf1, frame, kfs, nnratio, check_ori):
        """frame >= 0: the keyframes kfs against the frame; else kf1 against the keyframes kfs.  Returns (rc, [ids per pair], counts)"""
        kfs = np.array(kfs, dtype=np.int64)
        stride = max(max(self.n.values()), 1)
        ids = np.full((len(kfs), stride), -7, dtype=np.int64)
        cnt = np.full(len(kfs), -7, dtype=np.int32)
        r = self.L.fc_search_by_bow_batch(self.m, kf1, frame, kfs.ctypes.data_as(_pl), len(kfs), nnratio, int(check_ori), ids.ctypes.data_as(_pl), stride,
                                          cnt.ctypes.data_as(_pi))
        width = [self.n[frame] if frame >= 0 else self.n[kf1]] * len(kfs)
        return r, [ids[i, :w] for i, w in enumerate(width)], cnt

    def frame_points(self, fr):
        out = np.zeros(max(self.n[fr], 1), dtype=np.int64)
        assert self.L.fc_frame_points(self.m, fr, out.ctypes.data_as(_pl), len(out)) == self.n[fr]
        return out[:self.n[fr]]


def expected_frame_ids(kf, want):
    """vpMapPointMatches by id: the map point of keyframe kf whose match the yardstick leaves at each keypoint of the frame"""
    m21 = want["match21"]
    return np.where(m21 >= 0, 10000 * kf + m21, -1)


def expected_kf_ids(kf2, want):
    """vpMatches12 by id: the map point of keyframe kf2 matched to each keypoint of keyframe 1"""
    m12 = want["match12"]
    return np.where(m12 >= 0, 10000 * kf2 + m12, -1)
