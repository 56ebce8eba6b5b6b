"""LocalMapping::CreateNewMapPoints of the host facade (mc_slam_amd/host/LocalMapping.cpp) on a mock keyframe with three
neighbours and given matches: neighbour 2 and neighbour 4 pass the baseline / median-depth gate, neighbour 3 (two centimetres away)
does not.  The created points must be what the yardstick's decisions give (tests/triangulate_ref.py on the pairs the facade
extracts), and the matcher of the later neighbour must see the points created from the earlier one."""
import ctypes as C

import numpy as np
import pytest

import facade_sim3_lib
import triangulate_ref as ref
from mc_slam_amd import abi, synth

_pd = C.POINTER(C.c_double)
_pf = C.POINTER(C.c_float)
_pl = C.POINTER(C.c_long)
_pi = C.POINTER(C.c_int)
f32 = np.float32


def lib():
    L = facade_sim3_lib.lib()
    L.fc_create_new_map_points.argtypes = [C.c_void_p, C.c_long, _pl, C.c_int, _pi, _pl, _pi, _pl, C.c_int]
    L.fc_get_mappoint_obs.argtypes = [C.c_void_p, C.c_long, _pf, _pl, _pi, _pl, C.c_int]
    L.fc_kf_mappoint_at.argtypes = [C.c_void_p, C.c_long, C.c_int]
    L.fc_kf_mappoint_at.restype = C.c_long
    L.fc_map_n_points.argtypes = [C.c_void_p]
    L.fc_kf_median_depth.argtypes = [C.c_void_p, C.c_long, C.c_int]
    L.fc_kf_median_depth.restype = C.c_float
    return L


def centre(R, t):
    """KeyFrame::GetCameraCenter: -R^T t accumulated in float32, left to right"""
    R, t = f32(R), f32(t)
    out = np.zeros(3, dtype=f32)
    for i in range(3):
        s = f32(0)
        for k in range(3):
            s = f32(s + f32(R[k, i] * t[k]))
        out[i] = -s
    return out.astype(np.float64)


def second_pair(p, seed, n):
    """another neighbour of keyframe 1 of p: 0.3 m to the left, matches of points 2-8 m deep with half a pixel of noise, a fifth of
    them mismatched"""
    r = np.random.default_rng(seed)
    C1 = -p.Rcw1.T @ p.tcw1
    R4 = f32(synth.so3_exp(r.normal(size=3) * 0.02) @ p.Rcw1).astype(np.float64)
    C4 = C1 + p.Rcw1.T @ np.array([-0.3, 0.05, 0.02])
    t4 = f32(-R4 @ C4).astype(np.float64)
    uv1 = np.stack([r.uniform(50, 700, n), r.uniform(50, 430, n)], axis=1)
    Xc = r.uniform(2, 8, n)[:, None] * np.stack([(uv1[:, 0] - p.K1[2]) / p.K1[0], (uv1[:, 1] - p.K1[3]) / p.K1[1], np.ones(n)], axis=1)
    Y = (Xc @ p.Rcw1 + C1) @ R4.T + t4
    uv2 = np.stack([p.K1[0] * Y[:, 0] / Y[:, 2] + p.K1[2], p.K1[1] * Y[:, 1] / Y[:, 2] + p.K1[3]], axis=1) + r.normal(size=(n, 2)) * 0.5
    wrong = r.random(n) < 0.2
    uv2[wrong] = np.stack([r.uniform(50, 700, wrong.sum()), r.uniform(50, 430, wrong.sum())], axis=1)
    return p.copy(Rcw2=R4, tcw2=t4, K2=p.K1, uv1=f32(uv1), uv2=f32(uv2), oct1=r.integers(0, 4, n), oct2=r.integers(0, 4, n))


class Scene:
    def __init__(self):
        self.L = lib()
        self.m = self.L.fc_create()
        pa = synth.make_triangulate(51, 90, "std", same_K=False)
        pb = second_pair(pa, 52, 70)
        # the tables and thresholds as the facade's keyframes hold them
        sigma2 = np.array([f32(1.2 ** (2 * l)) for l in range(8)], dtype=np.float64)
        scale = np.array([f32(1.2 ** l) for l in range(8)], dtype=np.float64)
        tab = dict(level_sigma2_1=sigma2, scale_1=scale, level_sigma2_2=sigma2, scale_2=scale, ratio_factor=float(f32(1.5) * f32(1.2)))
        Ow1 = centre(pa.Rcw1, pa.tcw1)
        self.pa = pa.copy(Ow1=Ow1, Ow2=centre(pa.Rcw2, pa.tcw2), **tab)
        self.pb = pb.copy(Ow1=Ow1, Ow2=centre(pb.Rcw2, pb.tcw2), **tab)
        C1 = -pa.Rcw1.T @ pa.tcw1
        R3, t3 = pa.Rcw1, f32(-pa.Rcw1 @ (C1 + np.array([0.02, 0.0, 0.0]))).astype(np.float64)
        self.kf(1, pa.Rcw1, pa.tcw1, pa.K1)
        self.kf(2, pa.Rcw2, pa.tcw2, pa.K2)
        self.kf(3, R3, t3, pa.K1)
        self.kf(4, pb.Rcw2, pb.tcw2, pb.K2)
        # map points the keyframes already have: five per neighbour about 5 m in front of it (the median depth), three in keyframe 1
        self.next_mp = 0
        rng = np.random.default_rng(5)
        for kid, R, t, n in ((1, pa.Rcw1, pa.tcw1, 3), (2, pa.Rcw2, pa.tcw2, 5), (3, R3, t3, 5), (4, pb.Rcw2, pb.tcw2, 5)):
            for _ in range(n):
                Xc = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4.5, 5.5)])
                Pw = np.ascontiguousarray((Xc - t) @ R, dtype=f32)
                self.L.fc_add_mappoint(self.m, self.next_mp, Pw.ctypes.data_as(_pf), kid)
                self.L.fc_kf_add_keypoint(self.m, kid, self.next_mp, 100.0, 100.0, 0, 1)
                self.next_mp += 1
        # keypoints without map points: keyframe 1 holds those of pair a, then those of pair b; the neighbours hold theirs permuted
        self.matches = {}
        for other, p in ((2, self.pa), (4, self.pb)):
            perm = rng.permutation(p.n_matches)
            idx2 = np.zeros(p.n_matches, dtype=np.int64)
            for j in perm:
                idx2[j] = self.L.fc_kf_add_keypoint(self.m, other, -1, p.uv2[j, 0], p.uv2[j, 1], int(p.oct2[j]), 0)
            idx1 = np.array([self.L.fc_kf_add_keypoint(self.m, 1, -1, p.uv1[j, 0], p.uv1[j, 1], int(p.oct1[j]), 0) for j in range(p.n_matches)])
            self.matches[other] = np.stack([idx1, idx2], axis=1)
        self.matches[3] = np.array([[3, 5], [4, 6]])           # never looked at: the gate drops neighbour 3 first

    def kf(self, kid, R, t, K):
        nav = np.zeros(22); nav[6] = 1.0
        K = np.ascontiguousarray(K, dtype=np.float64)
        self.L.fc_add_keyframe(self.m, kid, nav.ctypes.data_as(_pd), K.ctypes.data_as(_pd), -1, 0)
        T = np.eye(4, dtype=f32)
        T[:3, :3], T[:3, 3] = R, t
        T = np.ascontiguousarray(T.reshape(-1))
        self.L.fc_set_pose_tcw(self.m, kid, T.ctypes.data_as(_pf))

    def create(self, neigh):
        begin = np.zeros(len(neigh) + 1, dtype=np.int32)
        rows = []
        for i, k in enumerate(neigh):
            rows.append(self.matches[k])
            begin[i + 1] = begin[i] + len(self.matches[k])
        mt = np.ascontiguousarray(np.vstack(rows), dtype=np.int64)
        nb = np.array(neigh, dtype=np.int64)
        seen = np.zeros(len(neigh), dtype=np.int32)
        ids = np.full(1000, -1, dtype=np.int64)
        n = self.L.fc_create_new_map_points(self.m, 1, nb.ctypes.data_as(_pl), len(neigh), begin.ctypes.data_as(_pi), mt.ctypes.data_as(_pl),
                                            seen.ctypes.data_as(_pi), ids.ctypes.data_as(_pl), len(ids))
        return n, seen, ids[:max(n, 0)]

    def point(self, pid):
        Pw, ref_kf, n_obs = np.zeros(3, dtype=f32), C.c_long(0), C.c_int(0)
        obs = np.zeros((8, 2), dtype=np.int64)
        k = self.L.fc_get_mappoint_obs(self.m, int(pid), Pw.ctypes.data_as(_pf), C.byref(ref_kf), C.byref(n_obs), obs.ctypes.data_as(_pl), 8)
        return Pw, ref_kf.value, n_obs.value, obs[:k].tolist()

    def close(self):
        self.L.fc_destroy(self.m)


@pytest.fixture()
def scene():
    s = Scene()
    yield s
    s.close()


def test_median_depth_and_the_gate_inputs(scene):
    """ComputeSceneMedianDepth(2) of the neighbours is the middle one of their five depths (CPU only)"""
    for kid in (2, 3, 4):
        assert 4.5 <= scene.L.fc_kf_median_depth(scene.m, kid, 2) <= 5.5
    assert np.linalg.norm(scene.pa.Ow2 - scene.pa.Ow1) / 5.5 > 0.01 and np.linalg.norm(scene.pb.Ow2 - scene.pb.Ow1) / 5.5 > 0.01
    ra, rb = ref.triangulate(scene.pa), ref.triangulate(scene.pb)
    assert ra["n_accepted"] >= 10 and rb["n_accepted"] >= 10 and (ra["reason"] != 0).sum() >= 5 and (rb["reason"] != 0).sum() >= 5
    assert min(ra["margin"].min(), rb["margin"].min()) >= 1e-9


@pytest.mark.gpu
def test_created_points_equal_the_yardsticks_decisions(scene):
    ra, rb = ref.triangulate(scene.pa), ref.triangulate(scene.pb)
    n, seen, ids = scene.create([2, 3, 4])
    assert n == ra["n_accepted"] + rb["n_accepted"] == len(ids)
    # neighbour 3 never reached the matcher; neighbour 4's matcher saw the points created from neighbour 2
    assert seen.tolist() == [3, -1, 3 + ra["n_accepted"]]
    assert scene.L.fc_map_n_points(scene.m) == n
    assert len(set(ids.tolist())) == n and (np.diff(ids) == 1).all()           # the recent list in creation order
    k = 0
    for other, r in ((2, ra), (4, rb)):
        for j in range(len(r["reason"])):                                         # match order
            idx1, idx2 = scene.matches[other][j]
            if r["reason"][j] != 0:
                assert scene.L.fc_kf_mappoint_at(scene.m, 1, int(idx1)) == -1 and scene.L.fc_kf_mappoint_at(scene.m, other, int(idx2)) == -1
                continue
            Pw, ref_kf, n_obs, obs = scene.point(ids[k])
            assert Pw.tobytes() == f32(r["x3d"][j]).tobytes(), (other, j, Pw, r["x3d"][j])
            assert ref_kf == 1 and n_obs == 2 and obs == [[1, idx1], [other, idx2]]
            assert scene.L.fc_kf_mappoint_at(scene.m, 1, int(idx1)) == ids[k] and scene.L.fc_kf_mappoint_at(scene.m, other, int(idx2)) == ids[k]
            k += 1
    assert k == n


@pytest.mark.gpu
def test_no_neighbour_passes_the_gate(scene):
    n, seen, ids = scene.create([3])
    assert n == 0 and seen.tolist() == [-1] and scene.L.fc_map_n_points(scene.m) == 0
