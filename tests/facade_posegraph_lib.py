"""ctypes harness for Optimizer::OptimizeEssentialGraph of the host facade (mc_slam_amd/host/libvba_facade.so): builds a mock map
the way LoopClosing::CorrectLoop leaves it (spanning tree, loop edges, covisibility weights, CorrectedSim3 / NonCorrectedSim3,
LoopConnections, map points with reference keyframes), calls the facade and reads keyframes and map points back.  Beside it, the
NumPy mirror of the facade's extraction (src/Optimizer.cpp:4284-4478: vertices and the four edge rules)."""
import ctypes as C

import numpy as np

import facade_lib
import posegraph_ref as ref
from mc_slam_amd import abi, synth

_pd = C.POINTER(C.c_double)
_pf = C.POINTER(C.c_float)
_pl = C.POINTER(C.c_long)
_pi = C.POINTER(C.c_int)


def lib():
    L = facade_lib.lib()
    L.fc_kf_set_graph.argtypes = [C.c_void_p, C.c_long, C.c_long, _pl, C.c_int, _pl, C.c_int, _pl, _pi, C.c_int]
    L.fc_set_kf_bad.argtypes = [C.c_void_p, C.c_long, C.c_int]
    L.fc_set_mappoint_bad.argtypes = [C.c_void_p, C.c_long, C.c_int]
    L.fc_mappoint_set_corrected.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_long]
    L.fc_optimize_essential_graph.argtypes = [C.c_void_p, C.c_long, C.c_long, _pl, _pd, C.c_int, _pl, _pd, C.c_int, _pl, C.c_int, C.c_int, C.c_int]
    L.fc_last_posegraph.restype = C.POINTER(abi.vba_posegraph_problem)
    L.fc_last_posegraph_result.restype = C.POINTER(abi.vba_posegraph_result)
    L.fc_last_posegraph_ids.argtypes = [_pl, C.c_int, _pl, C.c_int]
    L.fc_loop_map_updated.argtypes = [C.c_void_p]
    L.fc_get_nav.argtypes = [C.c_void_p, C.c_long, _pd, _pf]
    L.fc_get_mappoint.argtypes = [C.c_void_p, C.c_long, _pf, _pi, _pi]
    return L


def _longs(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(_pl)


def _mul(a, b):
    q, t, s = ref.sim3_mul(ref.unpack(a), ref.unpack(b))
    return ref.pack((q, t, s))[0]


def _inv(a):
    return ref.pack(ref.sim3_inv(ref.unpack(a)))[0]


class LoopMap:
    """n keyframes on the generator's drifted loop (ids 0..n-1, parent = predecessor), keyframe `bad` flagged bad, covisibility
    weights 150 / 120 / 60 to the three predecessors, a loop edge cur -> loop, LoopConnections from the last keyframes to the first
    ones with weights on both sides of minFeat, CorrectedSim3 / NonCorrectedSim3 for the last `n_corr` keyframes, n_pt map points
    of which every fifth was corrected by the current keyframe."""

    def __init__(self, seed=1, n=30, n_corr=3, n_pt=60, fix_scale=False, bad=7):
        self.L = lib()
        self.n, self.fix_scale, self.bad = n, fix_scale, bad
        g = synth.make_posegraph(seed, n, span=1, loops=[(n - 1, 0)], fix_scale=fix_scale, n_corrected=n_corr, n_pt=n_pt)
        self.loop_kf, self.cur_kf = 0, n - 1
        self.m = self.L.fc_create()
        # ConfigParam's T_bc is process-wide state that other harnesses set too: this one sets its own, a real lever arm
        self.R_bc, self.p_bc = synth.extrinsics()[:2]
        Rb, pb = np.ascontiguousarray(self.R_bc, dtype=np.float64).reshape(-1), np.ascontiguousarray(self.p_bc, dtype=np.float64)
        self.L.fc_set_tbc(Rb.ctypes.data_as(_pd), pb.ctypes.data_as(_pd))
        nav = np.zeros(22); nav[6] = 1.0; nav[7:10] = [0.1, 0.2, -0.1]
        K = np.array([450.0, 450.0, 370.0, 240.0])
        drift = synth.make_posegraph(seed, n, span=1, loops=[(n - 1, 0)], fix_scale=fix_scale, n_corrected=0).S   # uncorrected poses
        self.Tcw = []
        for k in range(n):
            self.L.fc_add_keyframe(self.m, k, nav.ctypes.data_as(_pd), K.ctypes.data_as(_pd), -1, 0)
            T = np.eye(4)
            T[:3, :3] = synth.quat_to_rot(drift[k, 3:7]); T[:3, 3] = drift[k, :3] / drift[k, 7]      # SE3 [R, t / s]
            T = np.ascontiguousarray(np.float32(T))
            self.Tcw.append(T)
            self.L.fc_set_pose_tcw(self.m, k, T.reshape(-1).ctypes.data_as(_pf))
        self.L.fc_set_kf_bad(self.m, bad, 1)
        self.weights = {}
        for k in range(n):
            cov = [(k - d, w) for d, w in ((1, 150), (2, 120), (3, 60)) if k - d >= 0] + [(k + d, w) for d, w in ((1, 150), (2, 120), (3, 60)) if k + d < n]
            cov.sort(key=lambda c: (-c[1], c[0]))
            self.weights[k] = cov
            ch, chp = _longs([k + 1] if k + 1 < n else [])
            le, lep = _longs([self.loop_kf] if k == self.cur_kf else ([self.cur_kf] if k == self.loop_kf else []))
            ci, cip = _longs([c[0] for c in cov])
            cw = np.ascontiguousarray([c[1] for c in cov], dtype=np.int32)
            self.L.fc_kf_set_graph(self.m, k, k - 1, chp, len(ch), lep, len(le), cip, cw.ctypes.data_as(_pi), len(cov))
        corr_ids = list(range(n - n_corr, n))
        self.corr = {k: g.S[k].copy() for k in corr_ids}
        self.nonc = {k: drift[k].copy() for k in corr_ids}
        # LoopConnections: the corrected keyframes now see the first keyframes; (cur, loop) passes whatever its weight, (n-2, 1) is
        # refused (weight 0 < minFeat)
        self.conn = [(self.cur_kf, self.loop_kf), (n - 2, 1)]
        self.pt = np.float32(g.pt)
        self.pt_ref = g.pt_ref.copy()
        self.pt_ref[0] = bad                                  # a point whose reference keyframe has no vertex: it stays
        self.corrected_pts = {}
        for p in range(n_pt):
            P = np.ascontiguousarray(self.pt[p])
            self.L.fc_add_mappoint(self.m, p, P.ctypes.data_as(_pf), int(self.pt_ref[p]))
            if p % 5 == 4:
                self.corrected_pts[p] = (p * 7) % n if (p * 7) % n != bad else 0
                self.L.fc_mappoint_set_corrected(self.m, p, self.cur_kf, self.corrected_pts[p])
        self.L.fc_set_mappoint_bad(self.m, 1, 1)

    def close(self):
        self.L.fc_destroy(self.m)

    def call(self, mode):
        ni, nip = _longs(sorted(self.nonc)); ci, cip = _longs(sorted(self.corr)); cn, cnp = _longs(np.array(self.conn).reshape(-1))
        nS = np.ascontiguousarray([self.nonc[k] for k in sorted(self.nonc)]); cS = np.ascontiguousarray([self.corr[k] for k in sorted(self.corr)])
        return self.L.fc_optimize_essential_graph(self.m, self.loop_kf, self.cur_kf, nip, nS.ctypes.data_as(_pd), len(ni), cip, cS.ctypes.data_as(_pd),
                                                  len(ci), cnp, len(self.conn), int(self.fix_scale), mode)

    def packed(self) -> abi.PoseGraphProblem:
        """the arrays the facade handed (or would hand) to vba_posegraph_optimize, copied out"""
        P = self.L.fc_last_posegraph().contents
        a = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt).copy() if n else np.zeros(0, dtype=dt)
        nv, ne, npt = P.n_vertices, P.n_edges, P.n_pt
        return abi.PoseGraphProblem(S=a(P.S, 8 * nv, np.float64), fixed=a(P.fixed, nv, np.uint8), edge_i=a(P.edge_i, ne, np.int32),
                                    edge_j=a(P.edge_j, ne, np.int32), edge_S=a(P.edge_S, 8 * ne, np.float64), fix_scale=P.fix_scale, its=P.its,
                                    lambda_init=P.lambda_init, pt=a(P.pt, 3 * npt, np.float64), pt_ref=a(P.pt_ref, npt, np.int32))

    def ids(self):
        P = self.L.fc_last_posegraph().contents
        k = np.zeros(max(P.n_vertices, 1), dtype=np.int64); p = np.zeros(max(P.n_pt, 1), dtype=np.int64)
        self.L.fc_last_posegraph_ids(k.ctypes.data_as(_pl), len(k), p.ctypes.data_as(_pl), len(p))
        return k[:P.n_vertices], p[:P.n_pt]

    def pose(self, k):
        nav = np.zeros(22); T = np.zeros(16, dtype=np.float32)
        self.L.fc_get_nav(self.m, k, nav.ctypes.data_as(_pd), T.ctypes.data_as(_pf))
        return nav, T.reshape(4, 4)

    def point(self, p):
        P = np.zeros(3, dtype=np.float32); a = C.c_int(); b = C.c_int()
        self.L.fc_get_mappoint(self.m, p, P.ctypes.data_as(_pf), C.byref(a), C.byref(b))
        return P, b.value

    # ---- the mirror of the extraction ----
    def vertex_S(self, k):
        """vScw[k]: CorrectedSim3 where it has the keyframe, else Sim3(Rcw, tcw, 1) from the float32 pose"""
        if k in self.corr:
            return self.corr[k]
        T = np.float64(self.Tcw[k])
        q = ref.R2q(T[None, :3, :3])[0]        # (normalised; Quaterniond(R) of a float32 rotation is unit to 1e-7)
        return np.concatenate([T[:3, 3], q, [1.0]])

    def expected_edges(self):
        """(i, j, Sji) of the four rules (src/Optimizer.cpp:4331-4478) as a list; keyframe ids, not vertex indices"""
        good = [k for k in range(self.n) if k != self.bad]
        vS = {k: self.vertex_S(k) for k in good}
        wt = lambda a, b: dict(self.weights[a]).get(b, 0)
        out, inserted = [], set()
        for i, j in self.conn:
            if (i != self.cur_kf or j != self.loop_kf) and wt(i, j) < 100:
                continue
            out.append((i, j, _mul(vS[j], _inv(vS[i]))))
            inserted.add((min(i, j), max(i, j)))
        for i in range(self.n):                                  # (bad keyframes are walked too: their edges find no vertex)
            if i == self.bad:
                continue
            Swi = _inv(self.nonc[i] if i in self.nonc else vS[i])
            src = lambda k: self.nonc[k] if k in self.nonc else vS.get(k)
            par = i - 1
            if par >= 0 and par != self.bad:
                out.append((i, par, _mul(src(par), Swi)))
            loops = [self.loop_kf] if i == self.cur_kf else ([self.cur_kf] if i == self.loop_kf else [])
            for l in loops:
                if l < i:
                    out.append((i, l, _mul(src(l), Swi)))
            cov = self.weights[i]
            n_ok = sum(1 for c in cov if c[1] >= 100)
            sel = [] if n_ok == len(cov) else [c[0] for c in cov[:n_ok]]
            for k in sel:
                if k != par and k != i + 1 and k not in loops and k != self.bad and k < i and (min(i, k), max(i, k)) not in inserted:
                    out.append((i, k, _mul(src(k), Swi)))
        return out
