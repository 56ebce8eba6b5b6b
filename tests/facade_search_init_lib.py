"""ctypes harness for ORBmatcher::SearchForInitialization and the MonocularInitialization slice of Tracking of the host facade
(mc_slam_amd/host/ORBmatcherInit.cpp, Tracking.cpp through the fc_init_frame_* / fc_search_for_initialization /
fc_monocular_initialization hooks) over the two frames of an abi.SearchInitProblem."""
import ctypes as C

import numpy as np

import facade_lib

_pf = C.POINTER(C.c_float)
_pi = C.POINTER(C.c_int32)
_pu8 = C.POINTER(C.c_uint8)


def lib():
    L = facade_lib.lib()
    L.fc_init_frame_create.argtypes = [C.c_int, _pf, _pi, _pf, _pu8, _pf, _pf, C.c_int, C.c_int]
    L.fc_init_frame_create.restype = C.c_void_p
    L.fc_init_frame_destroy.argtypes = [C.c_void_p]
    L.fc_init_frame_destroy.restype = None
    L.fc_init_frame_set_uright.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.fc_init_frame_set_uright.restype = None
    L.fc_search_for_initialization.argtypes = [C.c_void_p, C.c_void_p, _pf, C.c_int, _pi, C.c_int, _pi, C.c_float, C.c_int, C.c_int]
    L.fc_monocular_initialization.argtypes = [C.c_void_p, C.c_void_p, _pf, _pi, C.c_int, C.c_int, _pi, _pi, _pf, _pf, _pf, _pu8, _pi, _pi]
    return L


class FrameH:
    """a Frame of the facade: keypoints uv [n,2] (float32), octaves, angles, descriptors, K, bounds and grid size"""

    def __init__(self, uv, octave, angle, desc, bounds, cols, rows, K=(500.0, 500.0, 320.0, 240.0)):
        self.L = lib()
        self.n = len(octave)
        uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        o = np.ascontiguousarray(octave, dtype=np.int32)
        a = np.zeros(self.n, dtype=np.float32) if angle is None else np.ascontiguousarray(angle, dtype=np.float32)
        d = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        k, b = np.asarray(K, dtype=np.float32), np.asarray(bounds, dtype=np.float32)
        self.h = self.L.fc_init_frame_create(self.n, uv.ctypes.data_as(_pf), o.ctypes.data_as(_pi), a.ctypes.data_as(_pf), d.ctypes.data_as(_pu8),
                                             k.ctypes.data_as(_pf), b.ctypes.data_as(_pf), int(cols), int(rows))

    def set_uright(self, idx, ur):
        self.L.fc_init_frame_set_uright(self.h, idx, ur)

    def close(self):
        self.L.fc_init_frame_destroy(self.h)


def frames(p, uv1=None, K=(500.0, 500.0, 320.0, 240.0)):
    """(frame 1, frame 2) of an abi.SearchInitProblem; frame 1's own pixels do not matter to the matcher (uv1: what the Initializer reads)"""
    uv1 = p.prev_matched if uv1 is None else uv1
    f1 = FrameH(uv1, p.oct1, p.angle1, p.desc1, p.bounds, p.grid_cols, p.grid_rows, K)
    f2 = FrameH(p.uv2, p.oct2, p.angle2, p.desc2, p.bounds, p.grid_cols, p.grid_rows, K)
    return f1, f2


def search(f1, f2, prev, nnratio=0.9, check_ori=True, window=100):
    """SearchForInitialization: dict(ret, matches12 (as the call leaves vnMatches12), prev_matched)"""
    pm = np.ascontiguousarray(prev, dtype=np.float32).reshape(-1, 2).copy()
    cap = max(f1.n, len(pm), 1)
    m, n_out = np.full(cap, -7, dtype=np.int32), C.c_int32(-7)
    ret = f1.L.fc_search_for_initialization(f1.h, f2.h, pm.ctypes.data_as(_pf), len(pm), m.ctypes.data_as(_pi), cap, C.byref(n_out), nnratio,
                                            int(bool(check_ori)), int(window))
    return dict(ret=ret, matches12=m[:n_out.value].copy(), prev_matched=pm)


def monocular_initialization(f_init, f_cur, prev, matches=None, do_initialize=False, iterations=200):
    """the Tracking slice (and Initialize behind it): dict(ret, alive, matches12, prev_matched, init_ret, R21, t21, vP3D, vbTriangulated,
    sets, info)"""
    n1 = f_init.n
    pm = np.ascontiguousarray(prev, dtype=np.float32).reshape(-1, 2).copy()
    m = np.full(max(n1, 1), 5, dtype=np.int32) if matches is None else np.ascontiguousarray(matches, dtype=np.int32).copy()
    alive, init_ret = C.c_int32(-7), C.c_int32(-7)
    R, t = np.full(9, 7, dtype=np.float32), np.full(3, 7, dtype=np.float32)
    X, tri = np.full((max(n1, 1), 3), 7, dtype=np.float32), np.full(max(n1, 1), 7, dtype=np.uint8)
    sets, info = np.zeros((iterations, 8), dtype=np.int32), np.zeros(10, dtype=np.int32)
    ret = f_init.L.fc_monocular_initialization(f_init.h, f_cur.h, pm.ctypes.data_as(_pf), m.ctypes.data_as(_pi), n1, int(do_initialize), C.byref(alive),
                                               C.byref(init_ret), R.ctypes.data_as(_pf), t.ctypes.data_as(_pf), X.ctypes.data_as(_pf), tri.ctypes.data_as(_pu8),
                                               sets.ctypes.data_as(_pi), info.ctypes.data_as(_pi))
    names = ("ok", "model", "reason", "best_hyp_h", "best_hyp_f", "n_inliers_h", "n_inliers_f", "n_rt", "best_rt", "n_matches")
    return dict(ret=ret, alive=alive.value, matches12=m[:n1].copy(), prev_matched=pm, init_ret=init_ret.value, R21=R.reshape(3, 3), t21=t, vP3D=X[:n1],
                vbTriangulated=tri[:n1], sets=sets, info=dict(zip(names, map(int, info))))
