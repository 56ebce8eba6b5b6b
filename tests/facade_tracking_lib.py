"""ctypes harness for the tracking matchers of the host facade (both ORBmatcher::SearchByProjection overloads, Tracking::SearchLocalPoints
and the matching half of Tracking::TrackWithMotionModel: mc_slam_amd/host/ORBmatcher.cpp, Tracking.cpp, through the fc_* hooks), a
mock frame and map built from a synthetic scene (mc_slam_amd.synth.search_proj_scene), and a sequential Python restatement of the
whole functions around the yardstick tests/search_proj_ref.py, fed with the float32 values the facade hands to
vba_search_by_projection.

The mock: the current frame (id CUR) holds the scene's keypoints; a keypoint that the scene marks occupied holds an old point with
three observations, every eighth other keypoint an old point without observations (it does not block and may be overwritten).  Query
i is map point QUERY + i with two observations, or none where the scene says it does not block.  For the last-frame functions the
last frame (id LAST) has one keypoint per query with the query's octave and angle; a skipped query has no point there or is an
outlier."""
import ctypes as C

import numpy as np

import facade_sim3_lib
import search_proj_ref as ref_mod
from mc_slam_amd import abi, synth
from test_facade_newpoints import centre

_pd = C.POINTER(C.c_double)
_pf = C.POINTER(C.c_float)
_pl = C.POINTER(C.c_long)
_pu8 = C.POINTER(C.c_uint8)
f32 = np.float32
CUR, LAST = 7, 6
QUERY, OLD = 1000, 50000
IN_VIEW_LOCAL = (0, 7, 8, 9)


def lib():
    L = facade_sim3_lib.lib()
    L.fc_add_frame.argtypes = [C.c_void_p, C.c_long, _pd, _pd]
    L.fc_frame_set_tcw.argtypes = [C.c_void_p, C.c_long, _pf]
    L.fc_frame_add_obs.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_float, C.c_float, C.c_int]
    L.fc_mp_set_fuse_data.argtypes = [C.c_void_p, C.c_long, _pf, C.c_float, C.c_float, _pu8]
    L.fc_frame_set_tracking_data.argtypes = [C.c_void_p, C.c_long, C.c_long, _pu8, _pf, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]
    L.fc_frame_set_outlier.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int]
    L.fc_frame_set_uright.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_float]
    L.fc_frame_points.argtypes = [C.c_void_p, C.c_long, _pl, C.c_int]
    L.fc_mp_set_track.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_long]
    L.fc_mp_track_state.argtypes = [C.c_void_p, C.c_long, _pd]
    L.fc_search_by_projection_last.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_float, C.c_int, C.c_int]
    L.fc_search_by_projection_map.argtypes = [C.c_void_p, C.c_long, _pl, C.c_int, C.c_float, C.c_float]
    L.fc_search_local_points.argtypes = [C.c_void_p, C.c_long, _pl, C.c_int, C.c_long]
    L.fc_track_motion_model_matches.argtypes = [C.c_void_p, C.c_long, C.c_long]
    return L


class TrackingScene:
    def __init__(self, p: abi.SearchProjProblem, seed=0):
        self.L, self.p = lib(), p
        L = self.L
        r = np.random.default_rng(seed)
        self.m = L.fc_create()
        nav = np.zeros(22); nav[6] = 1.0
        K = p.K.copy()
        d = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_pd)
        L.fc_add_keyframe(self.m, 1, d(nav), d(K), -1, 0)              # the owner of every map point
        T = np.eye(4, dtype=f32)
        T[:3, :3], T[:3, 3] = f32(p.Rcw), f32(p.tcw)
        self.Ow = centre(T[:3, :3], T[:3, 3])
        top = f32(p.scale[-1])
        nq, nk = p.n_q, p.n_keys
        zero3 = np.zeros(3, dtype=f32)
        # the queries' map points
        self.pred_max = f32(p.q_pred_max if p.local else r.uniform(3, 30, nq))
        self.normal = f32(p.q_normal if p.local else np.tile([0, 0, 1.0], (nq, 1)))
        mn = self.pred_max / top
        self.dist_min, self.dist_max = (f32(0.8) * mn).astype(np.float64), (f32(1.2) * self.pred_max).astype(np.float64)
        for i in range(nq):
            pos = np.ascontiguousarray(f32(p.q_pos[i]))
            assert L.fc_add_mappoint(self.m, QUERY + i, pos.ctypes.data_as(_pf), 1) == 0
            L.fc_mp_set_fuse_data(self.m, QUERY + i, np.ascontiguousarray(self.normal[i]).ctypes.data_as(_pf), float(mn[i]), float(self.pred_max[i]),
                                  np.ascontiguousarray(p.q_desc[i]).ctypes.data_as(_pu8))
            L.fc_mp_set_track(self.m, QUERY + i, 2 if p.q_blocks[i] else 0, 0, 0)
        # the current frame
        L.fc_add_frame(self.m, CUR, d(nav), d(K))
        L.fc_frame_set_tcw(self.m, CUR, np.ascontiguousarray(T).ctypes.data_as(_pf))
        self.initial = np.full(nk, -1, dtype=np.int64)
        free = 0
        for k in range(nk):
            if p.occupied[k] or (free := free + 1) % 8 == 0:
                pid = OLD + k
                L.fc_add_mappoint(self.m, pid, zero3.ctypes.data_as(_pf), 1)
                L.fc_mp_set_fuse_data(self.m, pid, zero3.ctypes.data_as(_pf), 1.0, 2.0, np.zeros(32, dtype=np.uint8).ctypes.data_as(_pu8))
                L.fc_mp_set_track(self.m, pid, 3 if p.occupied[k] else 0, 0, 0)
                self.initial[k] = pid
            L.fc_frame_add_obs(self.m, CUR, int(self.initial[k]), float(p.uv[k, 0]), float(p.uv[k, 1]), int(p.oct[k]))
        self.angle = f32(p.angle if p.angle is not None else np.zeros(nk))
        b = p.bounds
        n = L.fc_frame_set_tracking_data(self.m, CUR, CUR, np.ascontiguousarray(p.desc).ctypes.data_as(_pu8), self.angle.ctypes.data_as(_pf), b[0], b[1], b[2], b[3],
                                         int(p.grid_cols), int(p.grid_rows))
        assert n == nk
        # the last frame: one keypoint per query
        if not p.local:
            L.fc_add_frame(self.m, LAST, d(nav), d(K))
            self.outlier = np.zeros(nq, dtype=bool)
            for i in range(nq):
                none = bool(p.q_skip[i]) and i % 2 == 0
                self.outlier[i] = bool(p.q_skip[i]) and not none
                L.fc_frame_add_obs(self.m, LAST, -1 if none else QUERY + i, float(r.uniform(0, 600)), float(r.uniform(0, 400)), int(p.q_oct[i]))
            L.fc_frame_set_tracking_data(self.m, LAST, LAST, np.zeros((nq, 32), dtype=np.uint8).ctypes.data_as(_pu8), f32(p.q_angle).ctypes.data_as(_pf),
                                         b[0], b[1], b[2], b[3], int(p.grid_cols), int(p.grid_rows))
            for i in range(nq):
                L.fc_frame_set_outlier(self.m, LAST, i, int(self.outlier[i]))

    def close(self):
        self.L.fc_destroy(self.m)

    def query_ids(self):
        return np.arange(QUERY, QUERY + self.p.n_q, dtype=np.int64)

    def frame_points(self):
        out = np.zeros(max(self.p.n_keys, 1), dtype=np.int64)
        assert self.L.fc_frame_points(self.m, CUR, out.ctypes.data_as(_pl), len(out)) == self.p.n_keys
        return out[:self.p.n_keys]

    def track_state(self, pid):
        out = np.zeros(7)
        self.L.fc_mp_track_state(self.m, int(pid), out.ctypes.data_as(_pd))
        return out

    def set_track(self, pid, n_obs, in_view, last_seen=0):
        self.L.fc_mp_set_track(self.m, int(pid), int(n_obs), int(in_view), int(last_seen))

    def problem(self, occupied=None, skip=None, **kw):
        """the problem as the facade hands it over: float32 values widened, the distances as MapPoint returns them, Ow as
        Frame::UpdatePoseMatrices forms it"""
        p = self.p
        ch = dict(occupied=p.occupied if occupied is None else occupied, q_skip=p.q_skip if skip is None else skip)
        if p.local:
            ch.update(Ow=self.Ow, q_dist_min=self.dist_min, q_dist_max=self.dist_max, q_pred_max=self.pred_max.astype(np.float64))
        ch.update(kw)
        return p.copy(**ch)

    def expected_points(self, want, before):
        """mvpMapPoints by id after a call whose yardstick answer is `want`, from the ids `before`"""
        out = np.asarray(before).copy()
        km = want["key_match"]
        out[km >= 0] = QUERY + km[km >= 0]
        out[km == -2] = -1
        return out

    def check_track_fields(self, want, skip):
        """the mTrack* members of every query point that was not skipped against the yardstick: mbTrackInView for the states 0 and
        7 .. 9 and then the projection, level and viewing cosine as float32"""
        for i in range(self.p.n_q):
            if skip[i]:
                continue
            t = self.track_state(QUERY + i)
            seen = want["state"][i] in IN_VIEW_LOCAL
            assert bool(t[0]) == seen, i
            if seen:
                assert (f32(t[1]), f32(t[2])) == (f32(want["uv"][i, 0]), f32(want["uv"][i, 1])) and t[3] == want["level"][i], i
                assert f32(t[4]) == f32(want["view_cos"][i]), i
