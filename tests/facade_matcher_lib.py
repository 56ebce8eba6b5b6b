"""ctypes harness for the matcher of the host facade (mc_slam_amd/host/ORBmatcher.h, LocalMapping::ComputeF12 and the
CreateNewMapPoints overload that calls the matcher itself, through the fc_* hooks), and the mock map of
tests/test_facade_newpoints.py with what the matcher reads beside the keypoints: descriptors, angles, feature vectors."""
import ctypes as C

import numpy as np

import test_facade_newpoints as newpoints
from mc_slam_amd import abi

_pf = C.POINTER(C.c_float)
_pl = C.POINTER(C.c_long)
_pi = C.POINTER(C.c_int)
_pu8 = C.POINTER(C.c_uint8)
_pu32 = C.POINTER(C.c_uint32)
f32 = np.float32
N_NODES = 7


def lib():
    L = newpoints.lib()
    L.fc_kf_set_matcher_data.argtypes = [C.c_void_p, C.c_long, _pu8, _pf, C.c_int, _pu32, _pi, _pi]
    L.fc_compute_f12.argtypes = [C.c_void_p, C.c_long, C.c_long, _pf, _pf]
    L.fc_compute_f12.restype = None
    L.fc_search_for_triangulation.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, _pl, C.c_int]
    L.fc_create_new_map_points_matched.argtypes = [C.c_void_p, C.c_long, _pl, C.c_int, _pl, C.c_int]
    return L


class MatcherScene(newpoints.Scene):
    """the mock map of test_facade_newpoints.py; match j of a pair shares a descriptor (a few bits flipped on either side) and the
    vocabulary node j mod 7 in both keyframes, the keypoints that came with map points get random descriptors in node 50"""

    def __init__(self):
        super().__init__()
        lib()
        r = np.random.default_rng(9)
        self.K = {1: self.pa.K1, 2: self.pa.K2, 3: self.pa.K1, 4: self.pb.K2}
        self.pose = {1: (self.pa.Rcw1, self.pa.tcw1), 2: (self.pa.Rcw2, self.pa.tcw2), 4: (self.pb.Rcw2, self.pb.tcw2)}
        n_mp = {1: 3, 2: 5, 3: 5, 4: 5}
        n = {k: n_mp[k] for k in n_mp}
        n[1] += self.pa.n_matches + self.pb.n_matches; n[2] += self.pa.n_matches; n[4] += self.pb.n_matches
        self.uv = {k: np.full((n[k], 2), 100.0, dtype=f32) for k in n}
        self.oct = {k: np.zeros(n[k], dtype=np.uint8) for k in n}
        self.desc = {k: r.integers(0, 256, (n[k], 32), dtype=np.uint8) for k in n}
        self.angle = {k: r.uniform(0, 359, n[k]).astype(f32) for k in n}
        self.node = {k: np.full(n[k], 50) for k in n}

        def flipped(d, k):
            b = np.unpackbits(d)
            b[r.choice(256, k, replace=False)] ^= 1
            return np.packbits(b)

        for other, p in ((2, self.pa), (4, self.pb)):
            for j, (i1, i2) in enumerate(self.matches[other]):
                self.uv[1][i1], self.uv[other][i2] = p.uv1[j], p.uv2[j]
                self.oct[1][i1], self.oct[other][i2] = p.oct1[j], p.oct2[j]
                base = r.integers(0, 256, 32, dtype=np.uint8)
                self.desc[1][i1], self.desc[other][i2] = flipped(base, 8), flipped(base, 8)
                self.angle[other][i2] = f32((self.angle[1][i1] + r.normal() * 4.0) % 359.0)
                self.node[1][i1] = self.node[other][i2] = j % N_NODES
        self.fv = {}
        for k in n:
            m = {}
            for i in r.permutation(n[k]):
                m.setdefault(int(self.node[k][i]), []).append(int(i))
            self.fv[k] = abi.feat_vec_csr(m)
            ids, begin, feat = self.fv[k]
            d, a = np.ascontiguousarray(self.desc[k]), np.ascontiguousarray(self.angle[k])
            assert self.L.fc_kf_set_matcher_data(self.m, k, d.ctypes.data_as(_pu8), a.ctypes.data_as(_pf), len(ids), ids.ctypes.data_as(_pu32),
                                                 np.ascontiguousarray(begin, dtype=np.int32).ctypes.data_as(_pi),
                                                 np.ascontiguousarray(feat, dtype=np.int32).ctypes.data_as(_pi)) == n[k]
        self.n = n

    def f12(self, k1, k2):
        """LocalMapping::ComputeF12 and the epipole of ORBmatcher::SearchForTriangulation, float32"""
        F, e = np.zeros(9, dtype=f32), np.zeros(2, dtype=f32)
        self.L.fc_compute_f12(self.m, k1, k2, F.ctypes.data_as(_pf), e.ctypes.data_as(_pf))
        return F.reshape(3, 3), e

    def has_mp(self, k):
        return np.array([self.L.fc_kf_mappoint_at(self.m, k, i) >= 0 for i in range(self.n[k])], dtype=np.uint8)

    def problem(self, k1, k2, check_orientation):
        """the pair as the facade hands it to vba_search_triangulation, with the facade's float32 F12 and epipole"""
        F, e = self.f12(k1, k2)
        sigma2 = np.array([f32(1.2 ** (2 * l)) for l in range(8)], dtype=np.float64)
        scale = np.array([f32(1.2 ** l) for l in range(8)], dtype=np.float64)
        (id1, b1, f1), (id2, b2, f2) = self.fv[k1], self.fv[k2]
        return abi.SearchTriProblem(desc1=self.desc[k1], desc2=self.desc[k2], has_mp1=self.has_mp(k1), has_mp2=self.has_mp(k2), node_id1=id1,
                                    node_begin1=b1, node_feat1=f1, node_id2=id2, node_begin2=b2, node_feat2=f2, uv1=self.uv[k1], uv2=self.uv[k2],
                                    angle1=self.angle[k1], angle2=self.angle[k2], oct2=self.oct[k2], level_sigma2_2=sigma2, scale_2=scale,
                                    F12=F.astype(np.float64), epipole=e.astype(np.float64), check_orientation=check_orientation)

    def search(self, k1, k2, check_orientation, only_stereo=False):
        pairs = np.full((self.n[k1] + 1, 2), -1, dtype=np.int64)
        n = self.L.fc_search_for_triangulation(self.m, k1, k2, int(check_orientation), int(only_stereo), pairs.ctypes.data_as(_pl), len(pairs))
        return n, pairs[:max(n, 0)]

    def create_matched(self, neigh):
        nb = np.array(neigh, dtype=np.int64)
        ids = np.full(1000, -1, dtype=np.int64)
        n = self.L.fc_create_new_map_points_matched(self.m, 1, nb.ctypes.data_as(_pl), len(neigh), ids.ctypes.data_as(_pl), len(ids))
        return n, ids[:max(n, 0)]
