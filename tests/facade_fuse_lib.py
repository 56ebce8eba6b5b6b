"""ctypes harness for map-point fusion in the host facade (both ORBmatcher::Fuse overloads and LocalMapping::SearchInNeighbors,
mc_slam_amd/host/ORBmatcher.cpp, LocalMapping.cpp, through the fc_* hooks), a small mock map, and a sequential Python restatement of
the whole functions (src/ORBmatcher.cpp:958-1254, src/LocalMapping.cpp:1588-1632, MapPoint::Replace src/MapPoint.cpp:245-292) on a
Python mirror of that map.  The restatement searches with tests/fuse_ref.py, fed with the float32 values the facade hands to
vba_fuse.

The map: five keyframes (ids 1 .. 5) around 260 world features, 640 x 480 pixels, the 64 x 48 grid.  A feature has up to three
map points: A (seen by the keyframes 1 and 2), B (3, 4 and mostly 5) and, for some features, C (5 only, in place of B), so fusing
meets keypoints that hold another point of the same feature (with more or with fewer observations), keypoints without a point,
and two points of one call that want the same keypoint."""
import ctypes as C

import numpy as np

import fuse_ref
import test_facade_newpoints as newpoints
from mc_slam_amd import abi, synth

_pf = C.POINTER(C.c_float)
_pl = C.POINTER(C.c_long)
_pi = C.POINTER(C.c_int)
_pu8 = C.POINTER(C.c_uint8)
f32 = np.float32
W, H, COLS, ROWS = 640, 480, 64, 48
KFS = (1, 2, 3, 4, 5)


def lib():
    L = newpoints.lib()
    L.fc_kf_set_fuse_data.argtypes = [C.c_void_p, C.c_long, _pu8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.fc_kf_grid.argtypes = [C.c_void_p, C.c_long, _pi, _pi, _pf]
    L.fc_kf_set_uright.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_float]
    L.fc_mp_set_fuse_data.argtypes = [C.c_void_p, C.c_long, _pf, C.c_float, C.c_float, _pu8]
    L.fc_fuse.argtypes = [C.c_void_p, C.c_long, _pl, C.c_int, C.c_float]
    L.fc_fuse_sim3.argtypes = [C.c_void_p, C.c_long, _pf, _pl, C.c_int, C.c_float, _pl]
    L.fc_search_in_neighbors.argtypes = [C.c_void_p, C.c_long, _pl, C.c_int]
    L.fc_mp_fuse_state.argtypes = [C.c_void_p, C.c_long, _pl]
    return L


class MirrorPoint:
    def __init__(self, pid, pos, normal, dmin, dmax, desc):
        self.id, self.pos, self.normal, self.min, self.max, self.desc = pid, pos, normal, dmin, dmax, desc
        self.obs, self.n_obs, self.bad, self.replaced, self.n_desc = {}, 0, False, None, 0

    def add_observation(self, kf, idx):
        if kf in self.obs:
            return
        self.obs[kf] = idx
        self.n_obs += 1


class FuseScene:
    def __init__(self, seed=5):
        self.L = lib()
        self.m = self.L.fc_create()
        r = np.random.default_rng(seed)
        self.K = f32([460.0, 460.0, 319.5, 239.5])
        self.scale = np.array([f32(1.2 ** l) for l in range(8)], dtype=f32)
        self.inv_sigma2 = np.array([f32(1.0) / f32(1.2 ** (2 * l)) for l in range(8)], dtype=f32)
        n_feat = 260
        X = np.stack([r.uniform(-4, 4, n_feat), r.uniform(-3, 3, n_feat), r.uniform(5, 11, n_feat)], axis=1)
        base = r.integers(0, 256, (n_feat, 32), dtype=np.uint8)
        lev = r.choice(5, size=n_feat, p=[0.4, 0.3, 0.15, 0.1, 0.05])
        self.T, self.kp, self.desc, self.mvp = {}, {}, {}, {}
        nav = np.zeros(22); nav[6] = 1.0
        Kd = self.K.astype(np.float64)
        cam = {}
        for k in KFS:
            R = synth.so3_exp(r.normal(size=3) * 0.04)
            c = np.array([0.35 * (k - 3), r.uniform(-0.1, 0.1), r.uniform(-0.2, 0.2)])
            T = np.eye(4, dtype=f32)
            T[:3, :3] = f32(R); T[:3, 3] = f32(-(R @ c))
            self.T[k] = T
            cam[k] = (R, c)
            assert self.L.fc_add_keyframe(self.m, k, nav.ctypes.data_as(C.POINTER(C.c_double)), Kd.ctypes.data_as(C.POINTER(C.c_double)), -1, 0) == 0
            self.L.fc_set_pose_tcw(self.m, k, np.ascontiguousarray(T).ctypes.data_as(_pf))
        has_a, has_b, has_c = r.random(n_feat) < 0.75, r.random(n_feat) < 0.75, r.random(n_feat) < 0.15
        self.pts = {}

        def flipped(d, k):
            b = np.unpackbits(d)
            b[r.choice(256, k, replace=False)] ^= 1
            return np.packbits(b)

        def make_point(pid, f, ref):
            pos = f32(X[f] + r.normal(size=3) * 0.004)
            o = r.normal(size=3)
            c = cam[ref][1] + o / np.linalg.norm(o) * r.uniform(0.1, 0.3)   # the mean view: off the keyframe's own centre, so no predicted level sits on an integer
            d = np.linalg.norm(pos - c)
            mx = f32(d) * self.scale[lev[f]]
            p = MirrorPoint(pid, pos, f32((pos - c) / d), f32(mx / self.scale[7]), mx, flipped(base[f], 6))
            self.pts[pid] = p
            assert self.L.fc_add_mappoint(self.m, pid, p.pos.ctypes.data_as(_pf), ref) == 0
            return p

        for f in range(n_feat):
            if has_a[f]:
                make_point(10000 + f, f, 1)
            if has_b[f]:
                make_point(20000 + f, f, 3)
            if has_c[f]:
                make_point(30000 + f, f, 5)
        for k in KFS:
            R, c = cam[k]
            kp, desc, mvp = [], [], []
            for f in r.permutation(n_feat):
                Y = R @ (X[f] - c)
                u, v = Kd[0] * Y[0] / Y[2] + Kd[2], Kd[1] * Y[1] / Y[2] + Kd[3]
                if not (8 < u < W - 8 and 8 < v < H - 8) or r.random() < 0.15:
                    continue
                u, v = u + r.normal() * 0.5, v + r.normal() * 0.5
                if k in (1, 2):
                    pid = 10000 + f if has_a[f] and r.random() < 0.85 else None
                elif k == 5 and has_c[f]:
                    pid = 30000 + f
                else:
                    pid = 20000 + f if has_b[f] and r.random() < (0.85 if k != 5 else 0.5) else None
                idx = self.L.fc_kf_add_keypoint(self.m, k, -1 if pid is None else pid, f32(u), f32(v), int(lev[f]), 1)
                assert idx == len(kp)
                kp.append((f32(u), f32(v), int(lev[f]))); desc.append(flipped(base[f], 6)); mvp.append(pid)
                if pid is not None:
                    self.pts[pid].obs[k] = idx
            for _ in range(40):                                            # keypoints of nothing in the map
                u, v = f32(r.uniform(0, W - 1)), f32(r.uniform(0, H - 1))
                self.L.fc_kf_add_keypoint(self.m, k, -1, u, v, 0, 1)
                kp.append((u, v, 0)); desc.append(r.integers(0, 256, 32, dtype=np.uint8)); mvp.append(None)
            self.kp[k], self.desc[k], self.mvp[k] = kp, np.array(desc, dtype=np.uint8), mvp
            d = np.ascontiguousarray(self.desc[k])
            assert self.L.fc_kf_set_fuse_data(self.m, k, d.ctypes.data_as(_pu8), 0, W, 0, H, COLS, ROWS) == len(kp)
        for p in self.pts.values():
            p.n_obs = len(p.obs)
            assert self.L.fc_mp_set_fuse_data(self.m, p.id, p.normal.ctypes.data_as(_pf), p.min, p.max, np.ascontiguousarray(p.desc).ctypes.data_as(_pu8)) == 0

    def close(self):
        self.L.fc_destroy(self.m)

    # ---- the facade
    def grid(self, k):
        begin, feat, inv = np.zeros(COLS * ROWS + 1, dtype=np.int32), np.zeros(len(self.kp[k]), dtype=np.int32), np.zeros(2, dtype=f32)
        n = self.L.fc_kf_grid(self.m, k, begin.ctypes.data_as(_pi), feat.ctypes.data_as(_pi), inv.ctypes.data_as(_pf))
        return begin, feat[:n], inv

    def _ids(self, ids):
        return np.array([-1 if i is None else i for i in ids], dtype=np.int64)

    def fuse(self, k, ids, th=3.0):
        a = self._ids(ids)
        return self.L.fc_fuse(self.m, k, a.ctypes.data_as(_pl), len(a), th)

    def fuse_sim3(self, k, S, ids, th):
        a, rep = self._ids(ids), np.full(len(ids), -7, dtype=np.int64)
        n = self.L.fc_fuse_sim3(self.m, k, np.ascontiguousarray(S, dtype=f32).ctypes.data_as(_pf), a.ctypes.data_as(_pl), len(a), th, rep.ctypes.data_as(_pl))
        return n, [None if i < 0 else int(i) for i in rep]

    def search_in_neighbors(self, k, targets):
        t = np.array(targets, dtype=np.int64)
        return self.L.fc_search_in_neighbors(self.m, k, t.ctypes.data_as(_pl), len(t))

    def facade_state(self):
        """(mvpMapPoints of every keyframe by id, per point: observations, nObs, bad, replaced-by, descriptor updates, listed by the map)"""
        mvp = {k: [(lambda i: None if i < 0 else int(i))(self.L.fc_kf_mappoint_at(self.m, k, j)) for j in range(len(self.kp[k]))] for k in KFS}
        pts = {}
        for pid in self.pts:
            P, ref, nobs = np.zeros(3, dtype=f32), C.c_long(0), C.c_int(0)
            obs = np.zeros((16, 2), dtype=np.int64)
            n = self.L.fc_get_mappoint_obs(self.m, pid, P.ctypes.data_as(_pf), C.byref(ref), C.byref(nobs), obs.ctypes.data_as(_pl), 16)
            st = np.zeros(5, dtype=np.int64)
            self.L.fc_mp_fuse_state(self.m, pid, st.ctypes.data_as(_pl))
            pts[pid] = (dict((int(a), int(b)) for a, b in obs[:n]), int(st[2]), bool(st[0]), None if st[1] < 0 else int(st[1]), int(st[3]), int(st[4]))
        return mvp, pts

    # ---- the restatement on the mirror
    def mirror_state(self):
        return ({k: list(self.mvp[k]) for k in KFS},
                {i: (dict(p.obs), p.n_obs, p.bad, p.replaced, p.n_desc, 0 if p.bad and p.replaced is not None else 1) for i, p in self.pts.items()})

    def problem(self, k, Rcw, tcw, Ow, ids, th, check_reproj):
        """the keyframe and the point list as the facade hands them to vba_fuse (skip marks the NULL entries only: the restatement
        applies the other tests of :980-984 / :1154 itself, point by point)"""
        kp = self.kp[k]
        uv = np.array([[a, b] for a, b, _ in kp], dtype=np.float64).reshape(-1, 2)
        inv_w, inv_h = f32(COLS) / f32(W), f32(ROWS) / f32(H)
        begin, feat = abi.grid_csr(uv, (0, W, 0, H), COLS, ROWS, inv_w, inv_h)
        P = [self.pts[i] if i is not None else None for i in ids]
        g = lambda fn, w: np.array([fn(p) if p is not None else np.zeros(w) for p in P], dtype=np.float64).reshape(len(P), w)
        return abi.FuseProblem(Rcw=Rcw, tcw=tcw, Ow=Ow, K=self.K.astype(np.float64), bounds=(0, W, 0, H), desc=self.desc[k], uv=uv,
                               oct=np.array([o for _, _, o in kp], dtype=np.uint8), scale=self.scale.astype(np.float64),
                               inv_level_sigma2=self.inv_sigma2.astype(np.float64), log_scale_factor=float(np.log(f32(1.2))), grid_cols=COLS,
                               grid_rows=ROWS, grid_inv_w=float(inv_w), grid_inv_h=float(inv_h), cell_begin=begin, cell_feat=feat,
                               pos=g(lambda p: p.pos, 3), normal=g(lambda p: p.normal, 3), dist_min=g(lambda p: [f32(0.8) * p.min], 1),
                               dist_max=g(lambda p: [f32(1.2) * p.max], 1), pred_max=g(lambda p: [p.max], 1),
                               pt_desc=np.array([p.desc if p is not None else np.zeros(32, dtype=np.uint8) for p in P], dtype=np.uint8).reshape(-1, 32),
                               skip=np.array([p is None for p in P], dtype=np.uint8), th=th, check_reproj=check_reproj)

    def _search(self, prob):
        r = fuse_ref.fuse_ref(prob)
        assert r["margin"] >= 1e-9 and r["margin_r"] >= 1e-9
        return r

    def pose(self, k):
        """GetRotation, GetTranslation and GetCameraCenter (float32 arithmetic, left to right)"""
        T = self.T[k]
        Ow = np.zeros(3, dtype=f32)
        for i in range(3):
            s = f32(0)
            for j in range(3):
                s = f32(s + f32(T[j, i] * T[j, 3]))
            Ow[i] = -s
        return T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64), Ow.astype(np.float64)

    def replace(self, a, b):
        """MapPoint::Replace: a->Replace(b)"""
        if a.id == b.id:
            return
        obs, a.obs, a.bad, a.replaced = a.obs, {}, True, b.id
        for kf in sorted(obs):
            idx = obs[kf]
            if kf not in b.obs:
                self.mvp[kf][idx] = b.id
                b.add_observation(kf, idx)
            else:
                self.mvp[kf][idx] = None
        b.n_desc += 1

    def ref_fuse(self, k, ids, th=3.0):
        """ORBmatcher::Fuse(pKF, vpMapPoints, th), point by point"""
        r = self._search(self.problem(k, *self.pose(k), ids, th, True))
        n_fused, counts = 0, dict(add=0, keep_in_kf=0, keep_new=0, skipped_live=0)
        for i, pid in enumerate(ids):
            if pid is None:
                continue
            p = self.pts[pid]
            if p.bad or k in p.obs:
                counts["skipped_live"] += r["state"][i] == 0
                continue
            if r["state"][i] != 0:
                continue
            best = int(r["best_idx"][i])
            in_kf = self.mvp[k][best]
            if in_kf is not None:
                q = self.pts[in_kf]
                if not q.bad:
                    if q.n_obs > p.n_obs:
                        self.replace(p, q); counts["keep_in_kf"] += 1
                    else:
                        self.replace(q, p); counts["keep_new"] += 1
            else:
                p.add_observation(k, best)
                self.mvp[k][best] = pid
                counts["add"] += 1
            n_fused += 1
        return n_fused, counts

    def ref_fuse_sim3(self, k, S, ids, th):
        """ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)"""
        S = np.asarray(S, dtype=f32)
        scw = np.sqrt(f32(f32(f32(S[0, 0] * S[0, 0]) + f32(S[0, 1] * S[0, 1])) + f32(S[0, 2] * S[0, 2])))
        R, t = (S[:3, :3] / scw).astype(f32), (S[:3, 3] / scw).astype(f32)
        Ow = np.zeros(3, dtype=f32)
        for i in range(3):
            a = f32(0)
            for j in range(3):
                a = f32(a + f32(-R[j, i] * t[j]))
            Ow[i] = a
        found = set(i for i in self.mvp[k] if i is not None and not self.pts[i].bad)
        r = self._search(self.problem(k, R.astype(np.float64), t.astype(np.float64), Ow.astype(np.float64), ids, th, False))
        n_fused, rep = 0, [None] * len(ids)
        for i, pid in enumerate(ids):
            if pid is None or self.pts[pid].bad or pid in found or r["state"][i] != 0:
                continue
            best = int(r["best_idx"][i])
            in_kf = self.mvp[k][best]
            if in_kf is not None:
                if not self.pts[in_kf].bad:
                    rep[i] = in_kf
            else:
                self.pts[pid].add_observation(k, best)
                self.mvp[k][best] = pid
            n_fused += 1
        return n_fused, rep

    def ref_search_in_neighbors(self, k, targets):
        """steps 2 and 3 of LocalMapping::SearchInNeighbors"""
        matches = list(self.mvp[k])
        total, counts = 0, {}
        for t in targets:
            n, c = self.ref_fuse(t, matches)
            total += n
            for a, b in c.items():
                counts[a] = counts.get(a, 0) + int(b)
        cand, seen = [], set()
        for t in targets:
            for pid in self.mvp[t]:
                if pid is None or self.pts[pid].bad or pid in seen:
                    continue
                seen.add(pid)
                cand.append(pid)
        n, c = self.ref_fuse(k, cand)
        for a, b in c.items():
            counts[a] = counts.get(a, 0) + int(b)
        return total + n, counts, cand
