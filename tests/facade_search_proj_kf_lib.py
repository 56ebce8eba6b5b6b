"""ctypes harness for the loop-closure and the relocalisation overload of ORBmatcher::SearchByProjection and for
LoopClosing::MatchLoopMapPoints in the host facade (mc_slam_amd/host/ORBmatcher.cpp, LoopClosing.cpp, through the fc_* hooks), a mock
map built from a synthetic scene (mc_slam_amd.synth.search_proj_kf_scene), and the problem as the facade hands it to
vba_search_by_projection_kf, for the yardstick tests/search_proj_kf_ref.py.

The mock: the target (keyframe TGT in loop mode, frame TGT in reloc mode) holds the scene's keypoints; a keypoint that the scene marks
occupied holds old point OLD + k.  Query i is map point QUERY + i.  A query the scene marks skipped is bad, or NULL in the source
keyframe (reloc mode), or is listed as already found: in loop mode it then stands in vpMatched in place of an old point."""
import ctypes as C

import numpy as np

import facade_tracking_lib as ftl
from mc_slam_amd import abi
from test_facade_newpoints import centre

_pd, _pf, _pl, _pu8, _pi = ftl._pd, ftl._pf, ftl._pl, ftl._pu8, C.POINTER(C.c_int)
f32 = np.float32
OWNER, SRC, TGT = 1, 2, 7
QUERY, OLD = 1000, 50000
LOOP, RELOC = abi.SEARCH_PROJ_KF_LOOP, abi.SEARCH_PROJ_KF_RELOC


def lib():
    L = ftl.lib()
    L.fc_kf_add_keypoint.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_float, C.c_float, C.c_int, C.c_int]
    L.fc_kf_set_fuse_data.argtypes = [C.c_void_p, C.c_long, _pu8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.fc_kf_set_uright.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_float]
    L.fc_set_covisible.argtypes = [C.c_void_p, C.c_long, _pl, C.c_int]
    L.fc_set_mappoint_bad.argtypes = [C.c_void_p, C.c_long, C.c_int]
    L.fc_search_by_projection_loop.argtypes = [C.c_void_p, C.c_long, _pf, _pl, C.c_int, _pl, C.c_int, C.c_int]
    L.fc_search_by_projection_reloc.argtypes = [C.c_void_p, C.c_long, C.c_long, _pl, C.c_int, C.c_float, C.c_int, C.c_int]
    L.fc_kf_set_angles.argtypes = [C.c_void_p, C.c_long, _pf, C.c_int]
    L.fc_match_loop_map_points.argtypes = [C.c_void_p, C.c_long, C.c_long, _pf, _pl, C.c_int, _pl, C.c_int, _pi]
    return L


def decompose_scw(S):
    """src/ORBmatcher.cpp:364-368 in float32: Rcw, tcw, Ow as float64 arrays of float32 values"""
    S = f32(S)
    scw = np.sqrt(f32(f32(S[0, 0] * S[0, 0] + S[0, 1] * S[0, 1]) + S[0, 2] * S[0, 2]))
    R, t = f32(S[:3, :3] / scw), f32(S[:3, 3] / scw)
    Ow = np.zeros(3, dtype=f32)
    for i in range(3):
        a = f32(0)
        for k in range(3):
            a = f32(a + f32(-R[k, i]) * t[k])
        Ow[i] = a
    return R.astype(np.float64), t.astype(np.float64), Ow.astype(np.float64)


class KfScene:
    def __init__(self, p: abi.SearchProjKfProblem, scale=1.0):
        self.L, self.p = lib(), p
        L = self.L
        self.m = L.fc_create()
        nav = np.zeros(22); nav[6] = 1.0
        d = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_pd)
        self.d, self.nav = d, nav
        L.fc_add_keyframe(self.m, OWNER, d(nav), d(p.K), -1, 0)            # the owner of every map point
        nq, nk = p.n_q, p.n_keys
        top = f32(p.scale[-1])
        self.pred_max = f32(p.q_pred_max)
        self.normal = f32(p.q_normal if p.q_normal is not None else np.tile([0, 0, 1.0], (nq, 1)))
        mn = f32(self.pred_max / top)
        self.dist_min, self.dist_max = (f32(0.8) * mn).astype(np.float64), (f32(1.2) * self.pred_max).astype(np.float64)
        zero3 = np.zeros(3, dtype=f32)
        for i in range(nq):
            pos = np.ascontiguousarray(f32(p.q_pos[i]))
            assert L.fc_add_mappoint(self.m, QUERY + i, pos.ctypes.data_as(_pf), OWNER) == 0
            L.fc_mp_set_fuse_data(self.m, QUERY + i, np.ascontiguousarray(self.normal[i]).ctypes.data_as(_pf), float(mn[i]), float(self.pred_max[i]),
                                  np.ascontiguousarray(p.q_desc[i]).ctypes.data_as(_pu8))
        self.initial = np.full(nk, -1, dtype=np.int64)
        for k in np.nonzero(p.occupied)[0]:
            L.fc_add_mappoint(self.m, OLD + int(k), zero3.ctypes.data_as(_pf), OWNER)
            L.fc_mp_set_fuse_data(self.m, OLD + int(k), zero3.ctypes.data_as(_pf), 1.0, 2.0, np.zeros(32, dtype=np.uint8).ctypes.data_as(_pu8))
            self.initial[k] = OLD + int(k)
        # the scene's skipped queries: every third is "already found", the others are bad
        self.skip = p.q_skip.astype(bool).copy()
        skipped = np.nonzero(self.skip)[0]
        self.found = [int(i) for i in skipped[::3]]
        for i in skipped:
            if int(i) not in self.found:
                L.fc_set_mappoint_bad(self.m, QUERY + int(i), 1)
        T = np.eye(4, dtype=f32)
        T[:3, :3], T[:3, 3] = f32(p.Rcw), f32(p.tcw)
        b = p.bounds
        if p.reloc:
            L.fc_add_frame(self.m, TGT, d(nav), d(p.K))
            L.fc_frame_set_tcw(self.m, TGT, np.ascontiguousarray(T).ctypes.data_as(_pf))
            for k in range(nk):
                L.fc_frame_add_obs(self.m, TGT, int(self.initial[k]), float(p.uv[k, 0]), float(p.uv[k, 1]), int(p.oct[k]))
            self.angle = f32(p.angle if p.angle is not None else np.zeros(nk))
            assert L.fc_frame_set_tracking_data(self.m, TGT, TGT, np.ascontiguousarray(p.desc).ctypes.data_as(_pu8), self.angle.ctypes.data_as(_pf),
                                                b[0], b[1], b[2], b[3], int(p.grid_cols), int(p.grid_rows)) == nk
            self.pose = (f32(p.Rcw).astype(np.float64), f32(p.tcw).astype(np.float64), centre(T[:3, :3], T[:3, 3]))
            # the source keyframe: one keypoint per query; a skipped query that is neither found nor bad-by-choice stays bad; every
            # seventh skipped one has no point at all
            L.fc_add_keyframe(self.m, SRC, d(nav), d(p.K), -1, 0)
            self.none = [int(i) for i in skipped[1::7] if int(i) not in self.found]
            for i in range(nq):
                L.fc_kf_add_keypoint(self.m, SRC, -1 if i in self.none else QUERY + i, float(i % 600), float(i % 400), 0, 1)
            self.q_angle = f32(p.q_angle if p.q_angle is not None else np.zeros(nq))
            L.fc_kf_set_angles(self.m, SRC, self.q_angle.ctypes.data_as(_pf), nq)
        else:
            self.Scw = np.eye(4, dtype=f32)
            self.Scw[:3, :3], self.Scw[:3, 3] = f32(scale) * T[:3, :3], f32(scale) * T[:3, 3]
            self.pose = decompose_scw(self.Scw)
            self.add_target_keyframe()
            # an already-found query stands in vpMatched in place of an old point
            occ = np.nonzero(p.occupied)[0]
            self.found = self.found[:len(occ)]
            for i in skipped:
                if int(i) in skipped[::3] and int(i) not in self.found:
                    L.fc_set_mappoint_bad(self.m, QUERY + int(i), 1)
            for j, i in enumerate(self.found):
                self.initial[occ[j]] = QUERY + i

    def add_target_keyframe(self):
        p, L = self.p, self.L
        L.fc_add_keyframe(self.m, TGT, self.d(self.nav), self.d(p.K), -1, 0)
        for k in range(p.n_keys):
            L.fc_kf_add_keypoint(self.m, TGT, -1, float(p.uv[k, 0]), float(p.uv[k, 1]), int(p.oct[k]), 0)
        b = p.bounds
        assert L.fc_kf_set_fuse_data(self.m, TGT, np.ascontiguousarray(p.desc).ctypes.data_as(_pu8), int(b[0]), int(b[1]), int(b[2]), int(b[3]),
                                     int(p.grid_cols), int(p.grid_rows)) == p.n_keys

    def close(self):
        self.L.fc_destroy(self.m)

    def problem(self, **kw):
        """the problem as the facade hands it over: float32 values widened, the distances as MapPoint returns them, the pose as the
        overload forms it"""
        p = self.p
        ch = dict(Rcw=self.pose[0], tcw=self.pose[1], Ow=self.pose[2], q_skip=self.skip.astype(np.uint8), q_dist_min=self.dist_min,
                  q_dist_max=self.dist_max, q_pred_max=self.pred_max.astype(np.float64), occupied=(self.initial >= 0).astype(np.uint8))
        ch.update(kw)
        return p.copy(**ch)

    def expected_points(self, want, before, ids=None):
        """vpMatched / mvpMapPoints by id after a call whose yardstick answer is `want`, from the ids `before`; ids: the map point id
        behind every query (QUERY + i by default)"""
        out = np.asarray(before).copy()
        km = want["key_match"]
        ids = QUERY + np.arange(self.p.n_q) if ids is None else np.asarray(ids)
        out[km >= 0] = ids[km[km >= 0]]
        out[km == -2] = -1
        return out

    def loop_call(self, th=10):
        ids = (QUERY + np.arange(self.p.n_q)).astype(np.int64)
        matched = self.initial.copy()
        r = self.L.fc_search_by_projection_loop(self.m, TGT, np.ascontiguousarray(self.Scw).ctypes.data_as(_pf), ids.ctypes.data_as(_pl), len(ids),
                                                matched.ctypes.data_as(_pl), len(matched), th)
        return r, matched

    def reloc_call(self, th, orb_dist, check_ori=1):
        found = np.array([QUERY + i for i in self.found] + [OLD], dtype=np.int64)[:max(len(self.found), 1)]
        r = self.L.fc_search_by_projection_reloc(self.m, TGT, SRC, found.ctypes.data_as(_pl), len(self.found), th, orb_dist, check_ori)
        out = np.zeros(max(self.p.n_keys, 1), dtype=np.int64)
        assert self.L.fc_frame_points(self.m, TGT, out.ctypes.data_as(_pl), len(out)) == self.p.n_keys
        return r, out[:self.p.n_keys]
