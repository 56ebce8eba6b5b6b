"""ORBmatcher::SearchBySim3 of the host facade (mc_slam_amd/host/ORBmatcher.cpp, through the fc_search_by_sim3 hooks) on the mock map of
tests/facade_fuse_lib.py, of which two keyframes are used: keyframe 1 with the map points A and keyframe 3 with the map points B of
the same world features.  It is compared with a sequential Python restatement of the whole function (src/ORBmatcher.cpp:1258-1496):
the vbAlreadyMatched flags of :1291-1301 with GetIndexInKeyFrame, both searches through tests/search_sim3_ref.py fed with the
float32 values the facade hands to vba_search_by_sim3, and the agreement loop; the return value and vpMatches12 are equal entry by
entry."""
import ctypes as C

import numpy as np
import pytest

import facade_fuse_lib as ffl
import search_sim3_ref as ref_mod
from mc_slam_amd import abi, synth

_pf, _pl, _pu8 = ffl._pf, ffl._pl, ffl._pu8
f32 = np.float32
KF1, KF2 = 1, 3


class Sim3Scene(ffl.FuseScene):
    def __init__(self):
        super().__init__()
        self.L.fc_search_by_sim3.argtypes = [C.c_void_p, C.c_long, C.c_long, _pl, C.c_int, C.c_float, _pf, _pf, C.c_float]
        self.L.fc_search_by_sim3_flags.argtypes = [C.c_void_p, C.c_long, C.c_long, _pl, C.c_int, _pu8, _pu8]
        # S12 near the relative pose of the two keyframes (p_c1 = R1 R2^T (p_c2 - t2) + t1), with a scale of its own
        T1, T2 = self.T[KF1].astype(np.float64), self.T[KF2].astype(np.float64)
        R12 = T1[:3, :3] @ T2[:3, :3].T
        self.s12 = f32(1.04)
        self.t12 = f32(T1[:3, 3] - R12 @ T2[:3, 3] + [0.004, -0.003, 0.005])
        self.R12 = f32(synth.so3_exp(np.array([0.002, -0.003, 0.001])) @ R12)

    def prior_matches(self):
        """vpMatches12: NULL but for eight keypoints of keyframe 1 matched to the point B of their feature that keyframe 2 observes
        (GetIndexInKeyFrame maps them into keyframe 2) and two matched to points that keyframe 2 does not observe"""
        m = [None] * len(self.mvp[KF1])
        in2 = [i for i, pid in enumerate(self.mvp[KF1]) if pid is not None and 10000 + pid in self.pts and KF2 in self.pts[10000 + pid].obs]
        out2 = [i for i, pid in enumerate(self.mvp[KF1]) if pid is not None and 20000 + pid in self.pts and KF2 not in self.pts[20000 + pid].obs]
        assert len(in2) >= 8 and len(out2) >= 2
        for i in in2[:8]:
            m[i] = 10000 + self.mvp[KF1][i]
        for i in out2[:2]:
            m[i] = 20000 + self.mvp[KF1][i]
        return m

    # ---- the facade
    def search_by_sim3(self, matches, th=7.5):
        a = self._ids(matches)
        n = self.L.fc_search_by_sim3(self.m, KF1, KF2, a.ctypes.data_as(_pl), len(a), self.s12, np.ascontiguousarray(self.R12).ctypes.data_as(_pf),
                                     np.ascontiguousarray(self.t12).ctypes.data_as(_pf), th)
        return n, [None if i < 0 else int(i) for i in a]

    def flags(self, matches):
        a = self._ids(matches)
        f1, f2 = np.full(len(self.mvp[KF1]), 7, dtype=np.uint8), np.full(len(self.mvp[KF2]), 7, dtype=np.uint8)
        assert self.L.fc_search_by_sim3_flags(self.m, KF1, KF2, a.ctypes.data_as(_pl), len(a), f1.ctypes.data_as(_pu8), f2.ctypes.data_as(_pu8)) == len(f1)
        return f1, f2

    # ---- the restatement on the mirror
    def ref_flags(self, matches):
        """:1287-1301"""
        n1, n2 = len(self.mvp[KF1]), len(self.mvp[KF2])
        vb1, vb2 = np.zeros(n1, dtype=np.uint8), np.zeros(n2, dtype=np.uint8)
        for i in range(n1):
            if matches[i] is not None:
                vb1[i] = 1
                idx2 = self.pts[matches[i]].obs.get(KF2, -1)
                if 0 <= idx2 < n2:
                    vb2[idx2] = 1
        return vb1, vb2

    def side(self, k, matched):
        """a keyframe as the facade hands it to vba_search_by_sim3"""
        kp = self.kp[k]
        uv = np.array([[a, b] for a, b, _ in kp], dtype=np.float64).reshape(-1, 2)
        inv_w, inv_h = f32(ffl.COLS) / f32(ffl.W), f32(ffl.ROWS) / f32(ffl.H)
        begin, feat = abi.grid_csr(uv, (0, ffl.W, 0, ffl.H), ffl.COLS, ffl.ROWS, inv_w, inv_h)
        P = [self.pts[i] if i is not None and not self.pts[i].bad else None for i in self.mvp[k]]
        g = lambda fn, w: np.array([fn(p) if p is not None else np.zeros(w) for p in P], dtype=np.float64).reshape(len(P), w)
        Rcw, tcw, _ = self.pose(k)
        return abi.SearchSim3KF(Rcw=Rcw, tcw=tcw, bounds=(0, ffl.W, 0, ffl.H), desc=self.desc[k], uv=uv, oct=np.array([o for _, _, o in kp], dtype=np.uint8),
                                scale=self.scale.astype(np.float64), log_scale_factor=float(np.log(f32(1.2))), grid_cols=ffl.COLS, grid_rows=ffl.ROWS,
                                grid_inv_w=float(inv_w), grid_inv_h=float(inv_h), cell_begin=begin, cell_feat=feat,
                                has_pt=np.array([p is not None for p in P], dtype=np.uint8), matched=matched, pos=g(lambda p: p.pos, 3),
                                dist_min=g(lambda p: [f32(0.8) * p.min], 1), dist_max=g(lambda p: [f32(1.2) * p.max], 1), pred_max=g(lambda p: [p.max], 1),
                                pt_desc=np.array([p.desc if p is not None else np.zeros(32, dtype=np.uint8) for p in P], dtype=np.uint8).reshape(-1, 32))

    def ref_search_by_sim3(self, matches, th=7.5):
        """ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th): (nFound, vpMatches12 afterwards, the searches)"""
        vb1, vb2 = self.ref_flags(matches)
        p = abi.SearchSim3Problem(kf1=self.side(KF1, vb1), kf2=self.side(KF2, vb2), K=self.K.astype(np.float64), s12=float(self.s12),
                                  R12=self.R12.astype(np.float64), t12=self.t12.astype(np.float64), th=th, th_high=100)
        r = ref_mod.search_sim3_ref(p)
        assert r["margin"] >= 1e-9 and r["margin_r"] >= 1e-9
        out, n_found = list(matches), 0
        for i1 in range(len(self.mvp[KF1])):                                     # :1480-1493
            idx2 = int(r["match1"][i1])
            if idx2 >= 0 and int(r["match2"][idx2]) == i1:
                out[i1] = self.mvp[KF2][idx2]
                n_found += 1
        return n_found, out, r


@pytest.fixture()
def scene():
    s = Sim3Scene()
    yield s
    s.close()


def _with_bad_points(scene):
    """one map point of each keyframe goes bad; neither is a prior match"""
    m = scene.prior_matches()
    b1 = [pid for i, pid in enumerate(scene.mvp[KF1]) if pid is not None and m[i] is None][4]
    b2 = [pid for pid in scene.mvp[KF2] if pid is not None and pid not in m][6]
    for pid in (b1, b2):
        scene.L.fc_set_mappoint_bad(scene.m, pid, 1)
        scene.pts[pid].bad = True
    return m, b1, b2


def test_already_matched_flags(scene):
    """vbAlreadyMatched1 / 2 as :1291-1301 build them, GetIndexInKeyFrame included (CPU only)"""
    m = scene.prior_matches()
    f1, f2 = scene.flags(m)
    w1, w2 = scene.ref_flags(m)
    assert np.array_equal(f1, w1) and np.array_equal(f2, w2)
    assert f1.sum() == 10 and f2.sum() == 8                                      # two prior matches are not seen by keyframe 2
    f1, f2 = scene.flags([None] * len(m))
    assert not f1.any() and not f2.any()


def test_stereo_keyframes_are_refused(scene, capfd):
    """the backend is monocular: a stereo keypoint in either keyframe fails the call before anything reaches the library (CPU only)"""
    m = scene.prior_matches()
    scene.L.fc_kf_set_uright(scene.m, KF2, 7, 12.5)
    n, after = scene.search_by_sim3(m)
    assert n == -1 and after == m and "stereo keypoint" in capfd.readouterr().err
    scene.L.fc_kf_set_uright(scene.m, KF2, 7, -1.0)
    scene.L.fc_kf_set_uright(scene.m, KF1, 3, 0.0)
    n, after = scene.search_by_sim3(m)
    assert n == -1 and after == m and "stereo keypoint" in capfd.readouterr().err
    n, after = scene.search_by_sim3(m[:-1])                                      # one entry per keypoint of pKF1
    assert n == -1 and "vpMatches12" in capfd.readouterr().err


@pytest.mark.gpu
def test_search_by_sim3_equals_the_restatement(scene):
    m, b1, b2 = _with_bad_points(scene)
    want, out, r = scene.ref_search_by_sim3(m)
    n, got = scene.search_by_sim3(m)
    print("SearchBySim3: %d found; states of keyframe 1 %s, of keyframe 2 %s" % (want, np.bincount(r["state1"], minlength=9).tolist(),
                                                                                   np.bincount(r["state2"], minlength=9).tolist()))
    assert n == want and got == out
    assert want >= 40 and (r["state1"] == 2).sum() == 10 and (r["state2"] == 2).sum() == 8
    assert r["state1"][scene.mvp[KF1].index(b1)] == 1 and r["state2"][scene.mvp[KF2].index(b2)] == 1      # a bad point is no usable point
    assert sum(a != b for a, b in zip(m, got)) == want and all(g == p for g, p in zip(got, m) if p is not None)   # prior matches stay
    assert (r["match1"] >= 0).sum() > want                                       # one-sided matches were not agreed
    # the function changes vpMatches12 only: the map is as it was
    mvp_f, _ = scene.facade_state()
    assert mvp_f[KF1] == scene.mvp[KF1] and mvp_f[KF2] == scene.mvp[KF2]
