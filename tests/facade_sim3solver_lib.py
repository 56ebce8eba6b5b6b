"""ctypes harness for the Sim3Solver of the host facade (mc_slam_amd/host/Sim3Solver.h through the fc_sim3solver_* hooks), on two mock
keyframes built by facade_sim3_lib.Sim3Pair.  Beside it, the NumPy mirror of the constructor (src/Sim3Solver.cpp:29-95: filters,
float32 camera-frame points, the gates as the reference's vector<size_t> holds them), of SetRansacParameters (:109-134) and of the
draw (:163-184, rand() through ctypes on libc, seeded by srand), which feed tests/sim3_ransac_ref.py."""
import ctypes as C
import math

import numpy as np

import facade_sim3_lib
from mc_slam_amd import abi

_pd = C.POINTER(C.c_double)
_pf = C.POINTER(C.c_float)
_pl = C.POINTER(C.c_long)
_pi = C.POINTER(C.c_int32)
_pu8 = C.POINTER(C.c_uint8)
_libc = C.CDLL(None)
_libc.rand.restype = C.c_int
_libc.srand.argtypes = [C.c_uint]
RAND_MAX = 2147483647


def lib():
    L = facade_sim3_lib.lib()
    L.fc_sim3solver_create.argtypes = [C.c_void_p, C.c_long, C.c_long, _pl, C.c_int, C.c_int]
    L.fc_sim3solver_create.restype = C.c_void_p
    L.fc_sim3solver_destroy.argtypes = [C.c_void_p]
    L.fc_sim3solver_destroy.restype = None
    L.fc_sim3solver_set_ransac.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int]
    L.fc_sim3solver_set_ransac.restype = None
    L.fc_sim3solver_info.argtypes = [C.c_void_p, _pi]
    L.fc_sim3solver_info.restype = None
    L.fc_sim3solver_arrays.argtypes = [C.c_void_p, _pl, _pd, _pd, _pd, _pd, _pd, _pd]
    L.fc_sim3solver_arrays.restype = None
    L.fc_srand.argtypes = [C.c_uint]
    L.fc_srand.restype = None
    L.fc_sim3solver_draw.argtypes = [C.c_void_p, C.c_int, _pi]
    L.fc_sim3solver_draw.restype = None
    L.fc_sim3solver_iterate.argtypes = [C.c_void_p, C.c_int, _pi, _pu8, _pi, _pf, _pi, C.c_int, _pi]
    L.fc_sim3solver_estimate.argtypes = [C.c_void_p, _pf, _pf, _pf]
    L.fc_sim3solver_estimate.restype = None
    return L


# ---- the mirror
def random_int(lo, hi):
    """DUtils::Random::RandomInt on libc's rand()"""
    d = hi - lo + 1
    return int((_libc.rand() / (RAND_MAX + 1.0)) * d) + lo


def draw(n_pairs, n_hyp):
    """the triples of n_hyp hypotheses as src/Sim3Solver.cpp:163-184 draws them: the removal writes [idx] where [randi] is meant, so
    a triple can hold a pair twice (the vector stays at its capacity, `size` is its logical size)"""
    out = np.zeros((n_hyp, 3), dtype=np.int32)
    for h in range(n_hyp):
        avail = list(range(n_pairs))
        size = n_pairs
        for i in range(3):
            randi = random_int(0, size - 1)
            idx = avail[randi]
            out[h, i] = idx
            avail[idx] = avail[size - 1]
            size -= 1
    return out


def max_iterations(n, probability=0.99, min_inliers=6, max_its=300):
    """mRansacMaxIts of SetRansacParameters (:109-134): epsilon is a float"""
    if min_inliers == n:
        its = 1
    else:
        eps = float(np.float32(min_inliers) / np.float32(n))
        den = math.log(1 - eps ** 3) if eps ** 3 < 1 else float("nan")
        v = math.ceil(math.log(1 - probability) / den) if den == den and den != 0 else None
        its = v if v is not None and -2 ** 31 <= v < 2 ** 31 else -2 ** 31     # the conversion of a value out of int's range
    return max(1, min(its, max_its))


def ransac_problem(pair, fix_scale):
    """what the constructor makes of a facade_sim3_lib.Sim3Pair: the abi.Sim3RansacProblem without triples, and mvnIndices1"""
    idx = np.array([k[2] for k in pair.kp1 if k[2] >= 0])
    sig2 = lambda o: np.float32(1.2 ** (2 * int(o)))                      # KeyFrame::mvLevelSigma2 (float)
    gate = lambda octs: np.array([float(int(9.210 * float(sig2(o)))) for o in octs])
    p = abi.Sim3RansacProblem(p1c=facade_sim3_lib.to_camera(pair.T1, pair.Pw1[idx]), p2c=facade_sim3_lib.to_camera(pair.T2, pair.Pw2[idx]),
                              max_err1=gate(pair.oct1[idx]), max_err2=gate(pair.oct2[idx]), K1=pair.K1.astype(np.float64),
                              K2=pair.K2.astype(np.float64), sample=np.zeros((0, 3), dtype=np.int32), fix_scale=int(fix_scale))
    return p, pair.rows_of_pairs()


def as_sim3_problem(p: abi.Sim3RansacProblem, S12):
    """the abi.Sim3Problem facade_sim3_lib.Sim3Pair builds its keyframes from: keypoints = the projected points, octaves from the gates"""
    pix = lambda K, P: P[:, :2] / P[:, 2:3] * K[:2] + K[2:]
    return abi.Sim3Problem(S12=S12, p1c=p.p1c, p2c=p.p2c, uv1=pix(p.K1, p.p1c), uv2=pix(p.K2, p.p2c), w1=9.210 / p.max_err1, w2=9.210 / p.max_err2,
                           K1=p.K1, K2=p.K2, fix_scale=p.fix_scale)


class Solver:
    """one Sim3Solver of the facade over a Sim3Pair"""

    def __init__(self, pair, fix_scale):
        self.L = lib()
        self.pair = pair
        m = pair.matches.copy()
        self.s = self.L.fc_sim3solver_create(pair.m, 1, 2, m.ctypes.data_as(_pl), len(m), int(fix_scale))
        self.mN1 = len(m)

    def close(self):
        self.L.fc_sim3solver_destroy(self.s)

    def set_ransac(self, probability=0.99, min_inliers=6, max_iterations=300):
        self.L.fc_sim3solver_set_ransac(self.s, probability, min_inliers, max_iterations)

    def info(self):
        o = np.zeros(6, dtype=np.int32)
        self.L.fc_sim3solver_info(self.s, o.ctypes.data_as(_pi))
        return dict(zip(("N", "mN1", "max_its", "iterations", "best_inliers", "min_inliers"), map(int, o)))

    def arrays(self):
        n = self.info()["N"]
        ind = np.zeros(max(n, 1), dtype=np.int64)
        g1, g2, p1, p2, K1, K2 = np.zeros(max(n, 1)), np.zeros(max(n, 1)), np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 3)), np.zeros(4), np.zeros(4)
        d = lambda a: a.ctypes.data_as(_pd)
        self.L.fc_sim3solver_arrays(self.s, ind.ctypes.data_as(_pl), d(g1), d(g2), d(p1), d(p2), d(K1), d(K2))
        return dict(indices1=ind[:n], gate1=g1[:n], gate2=g2[:n], p1c=p1[:n], p2c=p2[:n], K1=K1, K2=K2)

    def draw(self, n):
        t = np.zeros((max(n, 1), 3), dtype=np.int32)
        self.L.fc_sim3solver_draw(self.s, n, t.ctypes.data_as(_pi))
        return t[:n]

    def iterate(self, n_iterations, max_hyp=300):
        """iterate(n_iterations) (find() when n_iterations < 0): dict(found, no_more, inliers [mN1], n_inliers, T12 [4,4], triples)"""
        no_more, n_in, n_hyp = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        inl = np.zeros(max(self.mN1, 1), dtype=np.uint8)
        T = np.zeros(16, dtype=np.float32)
        tri = np.zeros((max_hyp, 3), dtype=np.int32)
        found = self.L.fc_sim3solver_iterate(self.s, n_iterations, C.byref(no_more), inl.ctypes.data_as(_pu8), C.byref(n_in), T.ctypes.data_as(_pf),
                                             tri.ctypes.data_as(_pi), max_hyp, C.byref(n_hyp))
        return dict(found=bool(found), no_more=bool(no_more.value), inliers=inl[:self.mN1].astype(bool), n_inliers=n_in.value,
                    T12=T.reshape(4, 4), triples=tri[:n_hyp.value].copy())

    def estimate(self):
        R, t, s = np.zeros(9, dtype=np.float32), np.zeros(3, dtype=np.float32), C.c_float(0)
        self.L.fc_sim3solver_estimate(self.s, R.ctypes.data_as(_pf), t.ctypes.data_as(_pf), C.byref(s))
        return R.reshape(3, 3), t, s.value
