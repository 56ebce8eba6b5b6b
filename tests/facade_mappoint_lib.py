"""ctypes harness for the map-point refresh of the host facade (UpdateMapPoints, LocalMapping::ProcessNewKeyFramePoints and
UpdateCurrentKeyFramePoints, mc_slam_amd/host/MapPointUpdate.cpp, through the fc_* hooks), a small mock map, and its Python mirror,
from which the abi.MapPointProblem of any list of points follows for tests/mappoint_ref.py.

The map: five keyframes (ids 1 .. 5), keyframe 3 bad, keyframe 5 the current one; 30 map points (ids 100 .. 129) seen by one to four
of the keyframes 1 .. 4.  Keyframe 5 holds a keypoint for most of them as tracking leaves them (matched, not yet observed), point 100
at TWO keypoints (the second occurrence finds it already in the keyframe), point 103 already observed, point 101 bad, and point 102
has keyframe 4 as its reference without being seen by it, so the reference's `observations[pRefKF]` reads keypoint 0 of keyframe 4."""
import ctypes as C

import numpy as np

import facade_fuse_lib
import test_facade_newpoints as newpoints
from mc_slam_amd import abi

_pf = C.POINTER(C.c_float)
_pl = C.POINTER(C.c_long)
_pi = C.POINTER(C.c_int)
_pu8 = C.POINTER(C.c_uint8)
f32 = np.float32
KFS = (1, 2, 3, 4, 5)
BAD_KF, CUR = 3, 5
SCALE = np.array([f32(1.2 ** l) for l in range(8)], dtype=f32)


def lib():
    L = facade_fuse_lib.lib()
    L.fc_update_map_points.argtypes = [C.c_void_p, _pl, C.c_int, C.c_int]
    L.fc_process_new_keyframe_points.argtypes = [C.c_void_p, C.c_long, _pl, C.c_int, _pi]
    L.fc_update_current_keyframe_points.argtypes = [C.c_void_p, C.c_long]
    L.fc_mp_attributes.argtypes = [C.c_void_p, C.c_long, _pf, _pf, _pu8, _pi]
    L.fc_set_mappoint_bad.argtypes = [C.c_void_p, C.c_long, C.c_int]
    return L


class MockMap:
    def __init__(self, seed=9):
        self.L = lib()
        self.m = self.L.fc_create()
        r = np.random.default_rng(seed)
        nav = np.zeros(22); nav[6] = 1.0
        K = np.array([460.0, 460.0, 319.5, 239.5])
        self.center, self.kp, self.desc = {}, {k: [] for k in KFS}, {k: [] for k in KFS}
        for k in KFS:
            R = newpoints.synth.so3_exp(r.normal(size=3) * 0.05)
            c = np.array([0.4 * (k - 3), r.uniform(-0.1, 0.1), r.uniform(-0.2, 0.2)])
            T = np.eye(4, dtype=f32)
            T[:3, :3] = f32(R); T[:3, 3] = f32(-(R @ c))
            assert self.L.fc_add_keyframe(self.m, k, nav.ctypes.data_as(C.POINTER(C.c_double)), K.ctypes.data_as(C.POINTER(C.c_double)), -1, int(k == BAD_KF)) == 0
            self.L.fc_set_pose_tcw(self.m, k, np.ascontiguousarray(T).ctypes.data_as(_pf))
            self.center[k] = newpoints.centre(T[:3, :3], T[:3, 3])
        self.ids = list(range(100, 130))
        self.pos, self.ref, self.obs, self.bad = {}, {}, {}, {101}
        self.proto, self.seen = {}, {}
        for p in self.ids:
            self.pos[p] = f32(np.array([r.uniform(-3, 3), r.uniform(-2, 2), r.uniform(5, 10)]))
            seen = [1, 2] if p == 102 else sorted(int(k) for k in r.choice(4, int(r.integers(1, 5)), replace=False) + 1)
            self.seen[p] = seen
            self.ref[p] = 4 if p == 102 else seen[-1]
            self.proto[p] = r.integers(0, 256, 32, dtype=np.uint8)
            self.obs[p] = {}
        # keyframe 4 needs a keypoint 0 whatever the draw: a keypoint of nothing
        self._keypoint(4, None, r, octave=6)
        for p in self.ids:
            assert self.L.fc_add_mappoint(self.m, p, self.pos[p].ctypes.data_as(_pf), self.ref[p]) == 0
        for p in self.ids:
            for k in self.seen[p]:
                self.obs[p][k] = self._keypoint(k, p, r, observe=1)
        # the current keyframe as tracking leaves it
        self.cur_points = []
        for p in self.ids:
            if p == 103:
                self.obs[p][CUR] = self._keypoint(CUR, p, r, observe=1)
            elif r.random() < 0.85 or p in (100, 101, 102):
                self._keypoint(CUR, p, r, observe=0)
            else:
                continue
            self.cur_points.append(p)
            if len(self.cur_points) % 4 == 0:
                self._keypoint(CUR, None, r)
                self.cur_points.append(None)
        self._keypoint(CUR, 100, r, observe=0)                         # the second keypoint of point 100
        self.cur_points.append(100)
        for k in KFS:
            d = np.ascontiguousarray(np.array(self.desc[k], dtype=np.uint8))
            assert self.L.fc_kf_set_fuse_data(self.m, k, d.ctypes.data_as(_pu8), 0, 640, 0, 480, 64, 48) == len(self.kp[k])
        self.L.fc_set_mappoint_bad(self.m, 101, 1)

    def _keypoint(self, k, p, r, observe=1, octave=None):
        o = int(r.integers(0, 6)) if octave is None else octave
        idx = self.L.fc_kf_add_keypoint(self.m, k, -1 if p is None else p, f32(r.uniform(10, 630)), f32(r.uniform(10, 470)), o, observe)
        assert idx == len(self.kp[k])
        self.kp[k].append(o)
        bits = np.unpackbits(self.proto[p]) if p is not None else r.integers(0, 2, 256).astype(np.uint8)
        bits[r.permutation(256)[:int(r.integers(0, 40))]] ^= 1
        self.desc[k].append(np.packbits(bits))
        return idx

    def close(self):
        self.L.fc_destroy(self.m)

    # ---- the facade
    def _ids(self, ids):
        return (C.c_long * len(ids))(*[-1 if i is None else i for i in ids])

    def update_map_points(self, ids, what):
        return self.L.fc_update_map_points(self.m, self._ids(ids), len(ids), what)

    def process_new_keyframe_points(self):
        rec, n = (C.c_long * 64)(), C.c_int(-7)
        ret = self.L.fc_process_new_keyframe_points(self.m, CUR, rec, 64, C.byref(n))
        return ret, list(rec[:n.value])

    def update_current_keyframe_points(self):
        return self.L.fc_update_current_keyframe_points(self.m, CUR)

    def attributes(self, p):
        """dict(normal [3] float32, min, max (float32), desc [32], normal_updates, desc_updates, n_observations, n_obs)"""
        nrm, mm, d, c = np.zeros(3, dtype=f32), np.zeros(2, dtype=f32), np.zeros(32, dtype=np.uint8), np.zeros(4, dtype=np.int32)
        self.L.fc_mp_attributes(self.m, p, nrm.ctypes.data_as(_pf), mm.ctypes.data_as(_pf), d.ctypes.data_as(_pu8), c.ctypes.data_as(_pi))
        return dict(normal=nrm, min=mm[0], max=mm[1], desc=d, normal_updates=int(c[0]), desc_updates=int(c[1]), n_observations=int(c[2]), n_obs=int(c[3]))

    # ---- the mirror
    def mirror_process_new_keyframe(self):
        """src/LocalMapping.cpp:1144-1171 on the mirror: (the points that get the refresh, the recent list)"""
        upd, recent = [], []
        for i, p in enumerate(self.cur_points):
            if p is None or p in self.bad:
                continue
            if CUR not in self.obs[p]:
                self.obs[p][CUR] = i
                upd.append(p)
            else:
                recent.append(p)
        return upd, recent

    def problem(self, ids, what=3):
        """the abi.MapPointProblem of the points `ids` as UpdateMapPoints must gather it from the mirror"""
        begin, obs_kf, desc, ref, rs = [0], [], [], [], []
        for p in ids:
            o = self.obs[p]
            for k in sorted(o):
                obs_kf.append(k - 1)
                desc.append(self.desc[k][o[k]])
            begin.append(len(obs_kf))
            rk = self.ref[p]
            ref.append(rk - 1)
            rs.append(float(SCALE[self.kp[rk][o.get(rk, 0)]]))           # observations[pRefKF]: 0 when the reference keyframe is no observer
        n = len(ids)
        return abi.MapPointProblem(kf_center=np.array([self.center[k] for k in KFS]), kf_bad=[int(k == BAD_KF) for k in KFS], what=np.full(n, what, dtype=np.uint8),
                                   obs_begin=begin, obs_kf=obs_kf, obs_desc=np.array(desc, dtype=np.uint8).reshape(-1, 32),
                                   pos=np.array([self.pos[p] for p in ids], dtype=np.float64).reshape(-1, 3), ref_kf=ref, ref_scale=rs,
                                   ref_top_scale=np.full(n, float(SCALE[7])))
