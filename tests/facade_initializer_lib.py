"""ctypes harness for the Initializer of the host facade (mc_slam_amd/host/Initializer.h through the fc_initializer_* hooks) over an
abi.TwoViewProblem's keypoints and matches.  Beside it, the NumPy mirror of the draw (src/Initializer.cpp:78-101: rand() through
ctypes on libc, DUtils::Random::SeedRandOnce(0) semantics), which feeds tests/two_view_ref.py."""
import ctypes as C

import numpy as np

import facade_lib
from facade_sim3solver_lib import _libc, random_int

_pf = C.POINTER(C.c_float)
_pi = C.POINTER(C.c_int32)
_pu8 = C.POINTER(C.c_uint8)


def lib():
    L = facade_lib.lib()
    L.fc_initializer_create.argtypes = [_pf, _pf, C.c_int, C.c_float, C.c_int]
    L.fc_initializer_create.restype = C.c_void_p
    L.fc_initializer_destroy.argtypes = [C.c_void_p]
    L.fc_initializer_destroy.restype = None
    L.fc_initializer_initialize.argtypes = [C.c_void_p, _pf, C.c_int, _pi, C.c_int, _pf, _pf, _pf, _pu8, _pi, _pi]
    return L


# ---- the mirror
def seed_rand(seed=0):
    """what the first Initialize of a process does (SeedRandOnce)"""
    _libc.srand(seed)


def draw_sets(n_matches, iterations=200):
    """mvSets as :80-101 draw them from the current rand() stream: the removal writes [randi], the eight indices are distinct"""
    out = np.zeros((iterations, 8), dtype=np.int32)
    for it in range(iterations):
        avail = list(range(n_matches))
        for j in range(8):
            randi = random_int(0, len(avail) - 1)
            out[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


def matches12(p):
    """vMatches12 of Tracking::MonocularInitialization: per keypoint of frame 1 its match in frame 2, -1 without one"""
    v = np.full(p.n_keys1, -1, dtype=np.int32)
    v[p.match[:, 0]] = p.match[:, 1]
    return v


class Init:
    """one Initializer of the facade over the reference frame of an abi.TwoViewProblem"""

    def __init__(self, p, sigma=1.0, iterations=200):
        self.L = lib()
        self.iterations = iterations
        self.n1 = p.n_keys1
        K, uv = p.K.astype(np.float32), np.ascontiguousarray(p.uv1, dtype=np.float32)
        self.s = self.L.fc_initializer_create(K.ctypes.data_as(_pf), uv.ctypes.data_as(_pf), p.n_keys1, sigma, iterations)

    def close(self):
        self.L.fc_initializer_destroy(self.s)

    def initialize(self, p):
        """Initialize(current frame of p, its matches): dict(ret, R21, t21, vP3D, vbTriangulated, sets, info)"""
        uv2, vm = np.ascontiguousarray(p.uv2, dtype=np.float32), matches12(p)
        R, t = np.full(9, 7, dtype=np.float32), np.full(3, 7, dtype=np.float32)
        X, tri = np.full((max(self.n1, 1), 3), 7, dtype=np.float32), np.full(max(self.n1, 1), 7, dtype=np.uint8)
        sets, info = np.zeros((self.iterations, 8), dtype=np.int32), np.zeros(10, dtype=np.int32)
        ret = self.L.fc_initializer_initialize(self.s, uv2.ctypes.data_as(_pf), p.n_keys2, vm.ctypes.data_as(_pi), self.n1, R.ctypes.data_as(_pf),
                                               t.ctypes.data_as(_pf), X.ctypes.data_as(_pf), tri.ctypes.data_as(_pu8), sets.ctypes.data_as(_pi),
                                               info.ctypes.data_as(_pi))
        names = ("ok", "model", "reason", "best_hyp_h", "best_hyp_f", "n_inliers_h", "n_inliers_f", "n_rt", "best_rt", "n_matches")
        return dict(ret=ret, R21=R.reshape(3, 3), t21=t, vP3D=X[:self.n1], vbTriangulated=tri[:self.n1], sets=sets, info=dict(zip(names, map(int, info))))
