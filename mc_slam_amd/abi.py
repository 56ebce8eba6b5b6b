"""ctypes mirror of include/vislam_ba.h (the C-ABI of the local-BA backend).

`Problem` keeps the caller-owned arrays of one local-BA window as numpy arrays (the layout the host
facade hands over after graph extraction, src/Optimizer.cpp:49-451 of the reference) and exposes them as
a `vba_problem` struct without copying.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

VARIANT_SE3_XYZ, VARIANT_PRV_XYZ, VARIANT_PRV_IDP = 0, 1, 2
PROTO_LOCAL, PROTO_SINGLE = 0, 1
SOLVER_LDLT, SOLVER_PCG = 0, 1
ALGO_GN, ALGO_LM = 0, 1
IMU_MEAS_STRIDE = 61
TRACE_MAX = 64
PROF_N = 8
PROF_NAMES = ["linearize", "control", "schur", "factor", "trsv", "update", "misc", "_"]

# float-rounded Huber deltas exactly as the reference builds them (const float th = sqrt(...)):
# src/Optimizer.cpp:241-242, 327
HUBER_VIS = float(np.float32(np.sqrt(5.991)))
HUBER_PRV = float(np.float32(np.sqrt(100 * 21.666)))
HUBER_BIAS = float(np.float32(np.sqrt(100 * 16.812)))
# src/IMU/imudata.cpp:25-31
GYR_BIAS_RW2 = 2.0e-5 * 2.0e-5
ACC_BIAS_RW2 = 5.0e-3 * 5.0e-3
GYR_MEAS_COV = 1.7e-4 * 1.7e-4 / 0.005
ACC_MEAS_COV = 2.0e-3 * 2.0e-3 / 0.005 * 100

_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int32)
_pu8 = C.POINTER(C.c_uint8)


class vba_problem(C.Structure):
    _fields_ = [
        ("variant", C.c_int32), ("n_kf", C.c_int32), ("n_kf_free", C.c_int32),
        ("n_pt", C.c_int32), ("n_obs", C.c_int32), ("n_imu", C.c_int32),
        ("kf_pose", _pd), ("kf_vel", _pd), ("kf_bias", _pd), ("pt", _pd),
        ("pt_ref_kf", _pi), ("pt_obs_begin", _pi), ("obs_kf", _pi),
        ("obs_uv", _pd), ("obs_w", _pd),
        ("K", C.c_double * 4), ("T_cb", C.c_double * 7), ("g_w", C.c_double * 3),
        ("imu_kf_i", _pi), ("imu_kf_j", _pi), ("imu_meas", _pd), ("imu_info_prv", _pd),
        ("inv_bg_rw2", C.c_double), ("inv_ba_rw2", C.c_double),
        ("huber_vis", C.c_double), ("huber_prv", C.c_double), ("huber_bias", C.c_double),
        ("algo", C.c_int32), ("its_stage1", C.c_int32), ("its_stage2", C.c_int32),
        ("chi2_th", C.c_double), ("depth_min", C.c_double), ("rho_min", C.c_double),
        ("protocol", C.c_int32), ("robust", C.c_int32), ("kf_fix", _pu8), ("solver", C.c_int32),
    ]


class vba_result(C.Structure):
    _fields_ = [
        ("chi2_vis", C.c_double), ("chi2_prv", C.c_double), ("chi2_bias", C.c_double),
        ("its_done", C.c_int32 * 2), ("n_outliers", C.c_int32), ("status", C.c_int32),
        ("obs_outlier", _pu8), ("obs_chi2", _pd),
        ("n_trace", C.c_int32), ("chi2_trace", C.c_double * TRACE_MAX),
        ("lambda_final", C.c_double), ("lin_iterations", C.c_int32),
    ]


class vba_profile(C.Structure):
    _fields_ = [
        ("ms", C.c_double * PROF_N), ("launches", C.c_int64 * PROF_N),
        ("bytes", C.c_double * PROF_N), ("total_ms", C.c_double), ("factor_flops", C.c_double),
        ("kernel_launches", C.c_int64),
    ]


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


@dataclass
class Problem:
    """One local-BA window in the flat SoA form of `vba_problem`."""
    variant: int
    n_kf_free: int
    kf_pose: np.ndarray            # [n_kf,7]
    pt: np.ndarray                 # [n_pt,3]
    pt_obs_begin: np.ndarray       # [n_pt+1]
    obs_kf: np.ndarray             # [n_obs]
    obs_uv: np.ndarray             # [n_obs,2]
    obs_w: np.ndarray              # [n_obs]
    K: np.ndarray                  # [4]
    kf_vel: Optional[np.ndarray] = None    # [n_kf,3]
    kf_bias: Optional[np.ndarray] = None   # [n_kf,12]
    pt_ref_kf: Optional[np.ndarray] = None
    T_cb: np.ndarray = field(default_factory=lambda: np.array([0, 0, 0, 0, 0, 0, 1.0]))
    g_w: np.ndarray = field(default_factory=lambda: np.zeros(3))
    imu_kf_i: Optional[np.ndarray] = None
    imu_kf_j: Optional[np.ndarray] = None
    imu_meas: Optional[np.ndarray] = None      # [n_imu,61]
    imu_info_prv: Optional[np.ndarray] = None  # [n_imu,81]
    algo: int = ALGO_GN
    its_stage1: int = 5
    its_stage2: int = 10
    chi2_th: float = 5.991
    depth_min: float = 0.0
    rho_min: float = 2e-6
    huber_vis: float = HUBER_VIS
    huber_prv: float = HUBER_PRV
    huber_bias: float = HUBER_BIAS
    protocol: int = 0                          # PROTO_LOCAL / PROTO_SINGLE
    robust: int = 1
    kf_fix: Optional[np.ndarray] = None        # [n_kf] uint8: bit0 PR, bit1 V, bit2 Bias fixed
    solver: int = 0                            # SOLVER_LDLT / SOLVER_PCG
    truth: dict = field(default_factory=dict)  # generator ground truth (not part of the ABI)

    def __post_init__(self):
        self.kf_pose = _f64(self.kf_pose, (-1, 7))
        self.pt = _f64(self.pt, (-1, 3))
        self.pt_obs_begin = _i32(self.pt_obs_begin)
        self.obs_kf = _i32(self.obs_kf)
        self.obs_uv = _f64(self.obs_uv, (-1, 2))
        self.obs_w = _f64(self.obs_w)
        self.K = _f64(self.K)
        n_kf = self.n_kf
        self.kf_vel = _f64(self.kf_vel if self.kf_vel is not None else np.zeros((n_kf, 3)), (-1, 3))
        self.kf_bias = _f64(self.kf_bias if self.kf_bias is not None else np.zeros((n_kf, 12)), (-1, 12))
        self.pt_ref_kf = _i32(self.pt_ref_kf if self.pt_ref_kf is not None else np.zeros(self.n_pt))
        self.T_cb = _f64(self.T_cb)
        self.g_w = _f64(self.g_w)
        self.imu_kf_i = _i32(self.imu_kf_i if self.imu_kf_i is not None else [])
        self.imu_kf_j = _i32(self.imu_kf_j if self.imu_kf_j is not None else [])
        self.imu_meas = _f64(self.imu_meas if self.imu_meas is not None else np.zeros((0, IMU_MEAS_STRIDE)),
                             (-1, IMU_MEAS_STRIDE))
        self.imu_info_prv = _f64(self.imu_info_prv if self.imu_info_prv is not None else np.zeros((0, 81)), (-1, 81))

    n_kf = property(lambda self: self.kf_pose.shape[0])
    n_pt = property(lambda self: self.pt.shape[0])
    n_obs = property(lambda self: self.obs_kf.shape[0])
    n_imu = property(lambda self: self.imu_kf_i.shape[0])

    def copy(self) -> "Problem":
        import copy as _c
        q = _c.copy(self)
        for k in ("kf_pose", "kf_vel", "kf_bias", "pt"):
            setattr(q, k, getattr(self, k).copy())
        return q

    def as_struct(self) -> vba_problem:
        s = vba_problem()
        s.variant, s.n_kf, s.n_kf_free = self.variant, self.n_kf, self.n_kf_free
        s.n_pt, s.n_obs, s.n_imu = self.n_pt, self.n_obs, self.n_imu
        p = lambda a, t: a.ctypes.data_as(t)
        s.kf_pose, s.kf_vel, s.kf_bias, s.pt = (p(self.kf_pose, _pd), p(self.kf_vel, _pd),
                                                p(self.kf_bias, _pd), p(self.pt, _pd))
        s.pt_ref_kf, s.pt_obs_begin, s.obs_kf = p(self.pt_ref_kf, _pi), p(self.pt_obs_begin, _pi), p(self.obs_kf, _pi)
        s.obs_uv, s.obs_w = p(self.obs_uv, _pd), p(self.obs_w, _pd)
        s.K[:] = self.K.tolist()
        s.T_cb[:] = self.T_cb.tolist()
        s.g_w[:] = self.g_w.tolist()
        s.imu_kf_i, s.imu_kf_j = p(self.imu_kf_i, _pi), p(self.imu_kf_j, _pi)
        s.imu_meas, s.imu_info_prv = p(self.imu_meas, _pd), p(self.imu_info_prv, _pd)
        s.inv_bg_rw2, s.inv_ba_rw2 = 1.0 / GYR_BIAS_RW2, 1.0 / ACC_BIAS_RW2
        s.huber_vis, s.huber_prv, s.huber_bias = self.huber_vis, self.huber_prv, self.huber_bias
        s.algo, s.its_stage1, s.its_stage2 = self.algo, self.its_stage1, self.its_stage2
        s.chi2_th, s.depth_min, s.rho_min = self.chi2_th, self.depth_min, self.rho_min
        s.protocol, s.robust = self.protocol, self.robust
        s.solver = self.solver
        if self.kf_fix is not None:
            self.kf_fix = np.ascontiguousarray(self.kf_fix, dtype=np.uint8)
            assert self.kf_fix.shape == (self.n_kf,)
            s.kf_fix = p(self.kf_fix, _pu8)
        return s


@dataclass
class Result:
    chi2_vis: float
    chi2_prv: float
    chi2_bias: float
    its_done: tuple
    n_outliers: int
    status: int
    obs_outlier: np.ndarray
    obs_chi2: np.ndarray
    chi2_trace: np.ndarray
    lambda_final: float
    lin_iterations: int = 0


class ResultBuf:
    """Caller-allocated result storage for one window."""

    def __init__(self, n_obs: int, want_chi2: bool = True):
        """want_chi2 = False: vba_result.obs_chi2 stays NULL -- the per-edge chi2 is an optional output (the reference's caller reads
        the erase list only: the classification of src/Optimizer.cpp:496-517 happens inside the call)"""
        self.outlier = np.zeros(max(n_obs, 1), dtype=np.uint8)
        self.chi2 = np.zeros(max(n_obs, 1) if want_chi2 else 1, dtype=np.float64)
        self.n_obs = n_obs
        self.want_chi2 = want_chi2
        self.s = vba_result()
        self.s.obs_outlier = self.outlier.ctypes.data_as(_pu8)
        if want_chi2:
            self.s.obs_chi2 = self.chi2.ctypes.data_as(_pd)

    def get(self) -> Result:
        s = self.s
        return Result(s.chi2_vis, s.chi2_prv, s.chi2_bias, (s.its_done[0], s.its_done[1]), s.n_outliers, s.status,
                      self.outlier[:self.n_obs].copy(), self.chi2[:self.n_obs].copy() if self.want_chi2 else None,
                      np.array(s.chi2_trace[:s.n_trace]), s.lambda_final, s.lin_iterations)


# ---- IMU-aided per-frame pose optimisation (include/vislam_ba.h: vba_frame_problem / vba_frame_result) ----
NAV_STRIDE = 22


class vba_frame_problem(C.Structure):
    _fields_ = [
        ("last_is_frame", C.c_int32), ("compute_marg", C.c_int32), ("n_obs", C.c_int32), ("n_obs_last", C.c_int32),
        ("nav", C.c_double * NAV_STRIDE), ("nav_last", C.c_double * NAV_STRIDE),
        ("obs_pw", _pd), ("obs_uv", _pd), ("obs_w", _pd), ("last_pw", _pd), ("last_uv", _pd), ("last_w", _pd),
        ("K", C.c_double * 4), ("T_cb", C.c_double * 7), ("g_w", C.c_double * 3),
        ("imu_meas", C.c_double * IMU_MEAS_STRIDE), ("imu_cov_pvphi", C.c_double * 81),
        ("prior_nav", C.c_double * NAV_STRIDE), ("prior_info", C.c_double * 225),
        ("inv_bg_rw2", C.c_double), ("inv_ba_rw2", C.c_double),
    ]


class vba_frame_result(C.Structure):
    _fields_ = [
        ("n_inliers", C.c_int32), ("status", C.c_int32), ("its_done", C.c_int32 * 4),
        ("outlier", _pu8), ("outlier_last", _pu8), ("chi2_round", C.c_double * 4), ("marg_cov_inv", C.c_double * 225),
    ]


@dataclass
class FrameProblem:
    """One PoseOptimization(Frame*, KeyFrame*|Frame*, IMUPreintegrator, gw, bComputeMarg) call as flat arrays."""
    nav: np.ndarray
    nav_last: np.ndarray
    obs_pw: np.ndarray
    obs_uv: np.ndarray
    obs_w: np.ndarray
    K: np.ndarray
    T_cb: np.ndarray
    g_w: np.ndarray
    imu_meas: np.ndarray
    imu_cov_pvphi: np.ndarray
    last_is_frame: int = 0
    compute_marg: int = 1
    last_pw: Optional[np.ndarray] = None
    last_uv: Optional[np.ndarray] = None
    last_w: Optional[np.ndarray] = None
    prior_nav: Optional[np.ndarray] = None
    prior_info: Optional[np.ndarray] = None
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        self.nav = _f64(self.nav); self.nav_last = _f64(self.nav_last)
        self.obs_pw = _f64(self.obs_pw, (-1, 3)); self.obs_uv = _f64(self.obs_uv, (-1, 2)); self.obs_w = _f64(self.obs_w)
        self.last_pw = _f64(self.last_pw if self.last_pw is not None else np.zeros((0, 3)), (-1, 3))
        self.last_uv = _f64(self.last_uv if self.last_uv is not None else np.zeros((0, 2)), (-1, 2))
        self.last_w = _f64(self.last_w if self.last_w is not None else np.zeros(0))
        self.prior_nav = _f64(self.prior_nav if self.prior_nav is not None else np.zeros(NAV_STRIDE))
        self.prior_info = _f64(self.prior_info if self.prior_info is not None else np.zeros((15, 15)), (15, 15))
        self.K = _f64(self.K); self.T_cb = _f64(self.T_cb); self.g_w = _f64(self.g_w)
        self.imu_meas = _f64(self.imu_meas); self.imu_cov_pvphi = _f64(self.imu_cov_pvphi, (9, 9))

    n_obs = property(lambda self: self.obs_pw.shape[0])
    n_obs_last = property(lambda self: self.last_pw.shape[0])

    def copy(self):
        import copy as _c
        q = _c.copy(self)
        q.nav = self.nav.copy()
        return q

    def as_struct(self) -> vba_frame_problem:
        s = vba_frame_problem()
        s.last_is_frame, s.compute_marg, s.n_obs, s.n_obs_last = self.last_is_frame, self.compute_marg, self.n_obs, self.n_obs_last
        s.nav[:] = self.nav.tolist(); s.nav_last[:] = self.nav_last.tolist()
        p = lambda a: a.ctypes.data_as(_pd)
        s.obs_pw, s.obs_uv, s.obs_w = p(self.obs_pw), p(self.obs_uv), p(self.obs_w)
        s.last_pw, s.last_uv, s.last_w = p(self.last_pw), p(self.last_uv), p(self.last_w)
        s.K[:] = self.K.tolist(); s.T_cb[:] = self.T_cb.tolist(); s.g_w[:] = self.g_w.tolist()
        s.imu_meas[:] = self.imu_meas.tolist(); s.imu_cov_pvphi[:] = self.imu_cov_pvphi.reshape(-1).tolist()
        s.prior_nav[:] = self.prior_nav.tolist(); s.prior_info[:] = self.prior_info.reshape(-1).tolist()
        s.inv_bg_rw2, s.inv_ba_rw2 = 1.0 / GYR_BIAS_RW2, 1.0 / ACC_BIAS_RW2
        return s


@dataclass
class FrameResult:
    n_inliers: int
    status: int
    its_done: tuple
    outlier: np.ndarray
    outlier_last: np.ndarray
    chi2_round: np.ndarray
    marg_cov_inv: np.ndarray
    nav: np.ndarray


class FrameResultBuf:
    def __init__(self, f: FrameProblem):
        self.o = np.zeros(max(f.n_obs, 1), dtype=np.uint8)
        self.ol = np.zeros(max(f.n_obs_last, 1), dtype=np.uint8)
        self.n, self.nl = f.n_obs, f.n_obs_last
        self.s = vba_frame_result()
        self.s.outlier = self.o.ctypes.data_as(_pu8)
        self.s.outlier_last = self.ol.ctypes.data_as(_pu8)

    def get(self, st: vba_frame_problem) -> FrameResult:
        s = self.s
        return FrameResult(s.n_inliers, s.status, tuple(s.its_done), self.o[:self.n].copy(), self.ol[:self.nl].copy(),
                           np.array(s.chi2_round[:]), np.array(s.marg_cov_inv[:]).reshape(15, 15), np.array(st.nav[:]))


# ---- on-disk problem format "VBAP" v2 (include/vislam_ba.h: vba_problem_save / vba_problem_load); v1 = the same without the
# two ints `solver`, `reserved0` behind has_kf_fix: still read ----
_HDR = np.dtype([("magic", "S4"), ("version", "<u4"), ("i", "<i4", 14), ("K", "<f8", 4), ("T_cb", "<f8", 7), ("g_w", "<f8", 3),
                 ("s", "<f8", 8)])
_HDR1 = np.dtype([("magic", "S4"), ("version", "<u4"), ("i", "<i4", 12), ("K", "<f8", 4), ("T_cb", "<f8", 7), ("g_w", "<f8", 3),
                  ("s", "<f8", 8)])


def save_problem(path, p: "Problem"):
    """numpy twin of vba_problem_save (same bytes)."""
    s = p.as_struct()
    hd = np.zeros(1, dtype=_HDR)
    hd["magic"] = b"VBAP"; hd["version"] = 2
    hd["i"] = [p.variant, p.n_kf, p.n_kf_free, p.n_pt, p.n_obs, p.n_imu, p.algo, p.its_stage1, p.its_stage2, p.protocol, p.robust,
               1 if p.kf_fix is not None else 0, p.solver, 0]
    hd["K"], hd["T_cb"], hd["g_w"] = p.K, p.T_cb, p.g_w
    hd["s"] = [s.inv_bg_rw2, s.inv_ba_rw2, p.huber_vis, p.huber_prv, p.huber_bias, p.chi2_th, p.depth_min, p.rho_min]
    with open(path, "wb") as f:
        f.write(hd.tobytes())
        for a in (p.kf_pose, p.kf_vel, p.kf_bias, p.pt, p.pt_ref_kf, p.pt_obs_begin, p.obs_kf, p.obs_uv, p.obs_w, p.imu_kf_i, p.imu_kf_j,
                  p.imu_meas, p.imu_info_prv):
            f.write(np.ascontiguousarray(a).tobytes())
        if p.kf_fix is not None:
            f.write(np.ascontiguousarray(p.kf_fix, dtype=np.uint8).tobytes())


def load_problem(path) -> "Problem":
    """numpy twin of vba_problem_load."""
    raw = open(path, "rb").read()
    if len(raw) < 8 or raw[:4] != b"VBAP" or int(np.frombuffer(raw[4:8], "<u4")[0]) not in (1, 2):
        raise ValueError("not a VBAP v1 / v2 file")
    hdt = _HDR if int(np.frombuffer(raw[4:8], "<u4")[0]) == 2 else _HDR1
    hd = np.frombuffer(raw[:hdt.itemsize], dtype=hdt)[0]
    variant, n_kf, n_free, n_pt, n_obs, n_imu, algo, its1, its2, proto, robust, has_fix = [int(x) for x in hd["i"][:12]]
    solver = int(hd["i"][12]) if hdt is _HDR else 0
    off = [hdt.itemsize]

    def take(n, dt):
        a = np.frombuffer(raw, dtype=dt, count=n, offset=off[0]).copy()
        off[0] += a.nbytes
        return a
    pose, vel, bias, pt = take(7 * n_kf, "<f8"), take(3 * n_kf, "<f8"), take(12 * n_kf, "<f8"), take(3 * n_pt, "<f8")
    ref, beg, okf = take(n_pt, "<i4"), take(n_pt + 1, "<i4"), take(n_obs, "<i4")
    uv, w = take(2 * n_obs, "<f8"), take(n_obs, "<f8")
    ii, ij, meas, info = take(n_imu, "<i4"), take(n_imu, "<i4"), take(61 * n_imu, "<f8"), take(81 * n_imu, "<f8")
    fix = take(n_kf, "u1") if has_fix else None
    if off[0] != len(raw):
        raise ValueError("trailing bytes")
    sc = hd["s"]
    return Problem(variant=variant, n_kf_free=n_free, kf_pose=pose, pt=pt, pt_obs_begin=beg, obs_kf=okf, obs_uv=uv, obs_w=w, K=hd["K"].copy(),
                   kf_vel=vel, kf_bias=bias, pt_ref_kf=ref, T_cb=hd["T_cb"].copy(), g_w=hd["g_w"].copy(), imu_kf_i=ii, imu_kf_j=ij,
                   imu_meas=meas, imu_info_prv=info, algo=algo, its_stage1=its1, its_stage2=its2, chi2_th=float(sc[5]),
                   depth_min=float(sc[6]), rho_min=float(sc[7]), huber_vis=float(sc[2]), huber_prv=float(sc[3]), huber_bias=float(sc[4]),
                   protocol=proto, robust=robust, kf_fix=fix, solver=solver)


# ---- loop-closure Sim3 refinement (include/vislam_ba.h: vba_sim3_problem / vba_sim3_result) ----
def huber_of(th2):
    """const float deltaHuber = sqrt(th2) with th2 a float (src/Optimizer.cpp:4634)"""
    return float(np.float32(np.sqrt(np.float32(th2))))


class vba_sim3_problem(C.Structure):
    _fields_ = [
        ("n_pairs", C.c_int32), ("fix_scale", C.c_int32), ("S12", C.c_double * 8),
        ("p1c", _pd), ("p2c", _pd), ("uv1", _pd), ("uv2", _pd), ("w1", _pd), ("w2", _pd),
        ("K1", C.c_double * 4), ("K2", C.c_double * 4), ("th2", C.c_double), ("huber", C.c_double),
        ("its_stage1", C.c_int32), ("its_stage2_bad", C.c_int32), ("its_stage2_clean", C.c_int32), ("min_inliers", C.c_int32),
    ]


class vba_sim3_result(C.Structure):
    _fields_ = [
        ("n_inliers", C.c_int32), ("status", C.c_int32), ("n_bad_stage1", C.c_int32), ("its_done", C.c_int32 * 2),
        ("chi2_stage", C.c_double * 2), ("outlier", _pu8), ("chi2_12", _pd), ("chi2_21", _pd),
    ]


@dataclass
class Sim3Problem:
    """One Optimizer::OptimizeSim3 call (src/Optimizer.cpp:4579-4785) as flat arrays: the matched pairs that passed its filters."""
    S12: np.ndarray                # [8] t(3) q(4, xyzw) s
    p1c: np.ndarray                # [n,3]
    p2c: np.ndarray                # [n,3]
    uv1: np.ndarray                # [n,2]
    uv2: np.ndarray                # [n,2]
    w1: np.ndarray                 # [n]
    w2: np.ndarray                 # [n]
    K1: np.ndarray                 # [4]
    K2: np.ndarray                 # [4]
    fix_scale: int = 0
    th2: float = 10.0
    huber: Optional[float] = None  # default: huber_of(th2)
    its_stage1: int = 5
    its_stage2_bad: int = 10
    its_stage2_clean: int = 5
    min_inliers: int = 10
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        self.S12 = _f64(self.S12, (8,))
        self.p1c = _f64(self.p1c, (-1, 3)); self.p2c = _f64(self.p2c, (-1, 3))
        self.uv1 = _f64(self.uv1, (-1, 2)); self.uv2 = _f64(self.uv2, (-1, 2))
        self.w1 = _f64(self.w1, (-1,)); self.w2 = _f64(self.w2, (-1,))
        self.K1 = _f64(self.K1, (4,)); self.K2 = _f64(self.K2, (4,))
        if self.huber is None:
            self.huber = huber_of(self.th2)

    n_pairs = property(lambda self: self.p1c.shape[0])

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        q.S12 = self.S12.copy()
        for k, v in changes.items():
            setattr(q, k, v)
        return q

    def as_struct(self) -> vba_sim3_problem:
        s = vba_sim3_problem()
        s.n_pairs, s.fix_scale = self.n_pairs, int(self.fix_scale)
        s.S12[:] = self.S12.tolist()
        p = lambda a: a.ctypes.data_as(_pd)
        s.p1c, s.p2c, s.uv1, s.uv2, s.w1, s.w2 = p(self.p1c), p(self.p2c), p(self.uv1), p(self.uv2), p(self.w1), p(self.w2)
        s.K1[:] = self.K1.tolist(); s.K2[:] = self.K2.tolist()
        s.th2, s.huber = self.th2, self.huber
        s.its_stage1, s.its_stage2_bad, s.its_stage2_clean = self.its_stage1, self.its_stage2_bad, self.its_stage2_clean
        s.min_inliers = self.min_inliers
        return s


@dataclass
class Sim3Result:
    n_inliers: int
    status: int
    n_bad_stage1: int
    its_done: tuple
    chi2_stage: np.ndarray
    outlier: np.ndarray
    chi2_12: Optional[np.ndarray]
    chi2_21: Optional[np.ndarray]
    S12: np.ndarray


class Sim3ResultBuf:
    """Caller-allocated result storage of one candidate."""

    def __init__(self, p: Sim3Problem, want_chi2: bool = True):
        self.n = p.n_pairs
        self.o = np.zeros(max(self.n, 1), dtype=np.uint8)
        self.want_chi2 = want_chi2
        self.s = vba_sim3_result()
        self.s.outlier = self.o.ctypes.data_as(_pu8)
        if want_chi2:
            self.c12 = np.zeros(max(self.n, 1)); self.c21 = np.zeros(max(self.n, 1))
            self.s.chi2_12 = self.c12.ctypes.data_as(_pd)
            self.s.chi2_21 = self.c21.ctypes.data_as(_pd)

    def get(self, st: vba_sim3_problem) -> Sim3Result:
        s = self.s
        return Sim3Result(s.n_inliers, s.status, s.n_bad_stage1, tuple(s.its_done), np.array(s.chi2_stage[:]), self.o[:self.n].copy(),
                          self.c12[:self.n].copy() if self.want_chi2 else None, self.c21[:self.n].copy() if self.want_chi2 else None,
                          np.array(st.S12[:]))


# ---- loop-candidate Sim3 RANSAC (include/vislam_ba.h: vba_sim3_ransac_problem / vba_sim3_ransac_result) ----
class vba_sim3_ransac_problem(C.Structure):
    _fields_ = [
        ("n_pairs", C.c_int32), ("fix_scale", C.c_int32), ("p1c", _pd), ("p2c", _pd), ("max_err1", _pd), ("max_err2", _pd),
        ("K1", C.c_double * 4), ("K2", C.c_double * 4), ("min_inliers", C.c_int32), ("n_hyp", C.c_int32), ("sample", _pi),
        ("best_inliers", C.c_int32), ("best_S12", C.c_double * 8),
    ]


class vba_sim3_ransac_result(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("hit", C.c_int32), ("its_done", C.c_int32), ("best_hyp", C.c_int32), ("n_inliers", C.c_int32),
        ("S12", C.c_double * 8), ("inlier", _pu8), ("hyp_inliers", _pi),
    ]


@dataclass
class Sim3RansacProblem:
    """One Sim3Solver (src/Sim3Solver.cpp) as flat arrays: the pairs that passed the constructor's filters, the triples of one
    iterate() call and the solver's running best."""
    p1c: np.ndarray                # [n,3]
    p2c: np.ndarray                # [n,3]
    max_err1: np.ndarray           # [n]
    max_err2: np.ndarray           # [n]
    K1: np.ndarray                 # [4]
    K2: np.ndarray                 # [4]
    sample: np.ndarray             # [n_hyp,3] int32
    fix_scale: int = 0
    min_inliers: int = 20
    best_inliers: int = 0
    best_S12: np.ndarray = None    # [8] t(3) q(4, xyzw) s
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        self.p1c = _f64(self.p1c, (-1, 3)); self.p2c = _f64(self.p2c, (-1, 3))
        self.max_err1 = _f64(self.max_err1, (-1,)); self.max_err2 = _f64(self.max_err2, (-1,))
        self.K1 = _f64(self.K1, (4,)); self.K2 = _f64(self.K2, (4,))
        self.sample = np.ascontiguousarray(self.sample, dtype=np.int32).reshape(-1, 3)
        self.best_S12 = _f64(np.zeros(8) if self.best_S12 is None else self.best_S12, (8,))

    n_pairs = property(lambda self: self.p1c.shape[0])
    n_hyp = property(lambda self: self.sample.shape[0])

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        q.best_S12 = self.best_S12.copy()
        for k, v in changes.items():
            setattr(q, k, v)
        q.__post_init__()
        return q

    def as_struct(self) -> vba_sim3_ransac_problem:
        s = vba_sim3_ransac_problem()
        s.n_pairs, s.fix_scale = self.n_pairs, int(self.fix_scale)
        p = lambda a: a.ctypes.data_as(_pd)
        s.p1c, s.p2c, s.max_err1, s.max_err2 = p(self.p1c), p(self.p2c), p(self.max_err1), p(self.max_err2)
        s.K1[:] = self.K1.tolist(); s.K2[:] = self.K2.tolist()
        s.min_inliers, s.n_hyp = int(self.min_inliers), self.n_hyp
        s.sample = self.sample.ctypes.data_as(_pi)
        s.best_inliers = int(self.best_inliers)
        s.best_S12[:] = self.best_S12.tolist()
        return s


@dataclass
class Sim3RansacResult:
    status: int
    hit: int
    its_done: int
    best_hyp: int
    n_inliers: int
    S12: np.ndarray                 # of the hit; zeros without one (the ABI leaves the caller's array untouched)
    inlier: np.ndarray              # [n] of the hit; zeros without one
    hyp_inliers: Optional[np.ndarray]
    best_inliers: int               # the problem's in/out state after the call
    best_S12: np.ndarray


class Sim3RansacResultBuf:
    """Caller-allocated result storage of one candidate."""

    def __init__(self, p: Sim3RansacProblem, want_counts: bool = True):
        self.n, self.nh = p.n_pairs, p.n_hyp
        self.o = np.zeros(max(self.n, 1), dtype=np.uint8)
        self.want_counts = want_counts
        self.s = vba_sim3_ransac_result()
        self.s.inlier = self.o.ctypes.data_as(_pu8)
        if want_counts:
            self.c = np.full(max(self.nh, 1), -1, dtype=np.int32)
            self.s.hyp_inliers = self.c.ctypes.data_as(_pi)

    def get(self, st: vba_sim3_ransac_problem) -> Sim3RansacResult:
        s = self.s
        return Sim3RansacResult(s.status, s.hit, s.its_done, s.best_hyp, s.n_inliers, np.array(s.S12[:]), self.o[:self.n].copy(),
                                self.c[:self.nh].copy() if self.want_counts else None, int(st.best_inliers), np.array(st.best_S12[:]))


# ---- two-view triangulation of new map points (include/vislam_ba.h: vba_triangulate_problem / vba_triangulate_result) ----
class vba_triangulate_problem(C.Structure):
    _fields_ = [
        ("Rcw1", C.c_double * 9), ("tcw1", C.c_double * 3), ("Ow1", C.c_double * 3), ("K1", C.c_double * 4),
        ("Rcw2", C.c_double * 9), ("tcw2", C.c_double * 3), ("Ow2", C.c_double * 3), ("K2", C.c_double * 4),
        ("n_levels1", C.c_int32), ("n_levels2", C.c_int32), ("level_sigma2_1", _pd), ("scale_1", _pd), ("level_sigma2_2", _pd), ("scale_2", _pd),
        ("ratio_factor", C.c_double), ("cos_max", C.c_double), ("chi2_th", C.c_double),
        ("n_matches", C.c_int32), ("uv1", _pd), ("uv2", _pd), ("oct1", _pu8), ("oct2", _pu8),
    ]


class vba_triangulate_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_accepted", C.c_int32), ("x3d", _pd), ("reason", _pu8)]


TRI_ACCEPTED, TRI_PARALLAX, TRI_W_ZERO, TRI_Z1, TRI_Z2, TRI_CHI2_1, TRI_CHI2_2, TRI_DIST_ZERO, TRI_SCALE = range(9)


@dataclass
class TriangulateProblem:
    """One keyframe pair of LocalMapping::CreateNewMapPoints (src/LocalMapping.cpp:1334-1517) as flat arrays: keyframe 1 =
    mpCurrentKeyFrame, keyframe 2 = one neighbour, and all their matches."""
    Rcw1: np.ndarray               # [3,3]
    tcw1: np.ndarray               # [3]
    Ow1: np.ndarray                # [3]
    K1: np.ndarray                 # [4] fx fy cx cy
    Rcw2: np.ndarray
    tcw2: np.ndarray
    Ow2: np.ndarray
    K2: np.ndarray
    level_sigma2_1: np.ndarray     # [n_levels1]
    scale_1: np.ndarray            # [n_levels1]
    level_sigma2_2: np.ndarray     # [n_levels2]
    scale_2: np.ndarray            # [n_levels2]
    uv1: np.ndarray                # [n,2]
    uv2: np.ndarray                # [n,2]
    oct1: np.ndarray               # [n] uint8
    oct2: np.ndarray               # [n] uint8
    ratio_factor: float = 1.5 * 1.2
    cos_max: float = 0.9998
    chi2_th: float = 5.991
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        self.Rcw1 = _f64(self.Rcw1, (3, 3)); self.Rcw2 = _f64(self.Rcw2, (3, 3))
        for k in ("tcw1", "Ow1", "tcw2", "Ow2"):
            setattr(self, k, _f64(getattr(self, k), (3,)))
        self.K1 = _f64(self.K1, (4,)); self.K2 = _f64(self.K2, (4,))
        for k in ("level_sigma2_1", "scale_1", "level_sigma2_2", "scale_2"):
            setattr(self, k, _f64(getattr(self, k), (-1,)))
        self.uv1 = _f64(self.uv1, (-1, 2)); self.uv2 = _f64(self.uv2, (-1, 2))
        self.oct1 = np.ascontiguousarray(self.oct1, dtype=np.uint8).reshape(-1)
        self.oct2 = np.ascontiguousarray(self.oct2, dtype=np.uint8).reshape(-1)

    n_matches = property(lambda self: self.uv1.shape[0])
    n_levels1 = property(lambda self: self.level_sigma2_1.shape[0])
    n_levels2 = property(lambda self: self.level_sigma2_2.shape[0])

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        q.__post_init__()
        return q

    def as_struct(self) -> vba_triangulate_problem:
        s = vba_triangulate_problem()
        for k in ("Rcw1", "tcw1", "Ow1", "K1", "Rcw2", "tcw2", "Ow2", "K2"):
            getattr(s, k)[:] = getattr(self, k).ravel().tolist()
        p = lambda a: a.ctypes.data_as(_pd)
        s.n_levels1, s.n_levels2 = self.n_levels1, self.n_levels2
        s.level_sigma2_1, s.scale_1, s.level_sigma2_2, s.scale_2 = p(self.level_sigma2_1), p(self.scale_1), p(self.level_sigma2_2), p(self.scale_2)
        s.ratio_factor, s.cos_max, s.chi2_th = float(self.ratio_factor), float(self.cos_max), float(self.chi2_th)
        s.n_matches = self.n_matches
        s.uv1, s.uv2 = p(self.uv1), p(self.uv2)
        s.oct1, s.oct2 = self.oct1.ctypes.data_as(_pu8), self.oct2.ctypes.data_as(_pu8)
        return s


@dataclass
class TriangulateResult:
    status: int
    n_accepted: int
    x3d: np.ndarray                 # [n,3]
    reason: np.ndarray              # [n] uint8


class TriangulateResultBuf:
    """Caller-allocated result storage of one keyframe pair."""

    def __init__(self, p: TriangulateProblem):
        self.n = p.n_matches
        self.x = np.zeros((max(self.n, 1), 3))
        self.r = np.full(max(self.n, 1), 255, dtype=np.uint8)
        self.s = vba_triangulate_result()
        self.s.x3d = self.x.ctypes.data_as(_pd)
        self.s.reason = self.r.ctypes.data_as(_pu8)

    def get(self) -> TriangulateResult:
        return TriangulateResult(self.s.status, self.s.n_accepted, self.x[:self.n].copy(), self.r[:self.n].copy())


# ---- monocular two-view initialisation (include/vislam_ba.h: vba_two_view_problem / vba_two_view_result) ----
class vba_two_view_problem(C.Structure):
    _fields_ = [
        ("n_keys1", C.c_int32), ("n_keys2", C.c_int32), ("uv1", _pd), ("uv2", _pd), ("n_matches", C.c_int32), ("n_hyp", C.c_int32),
        ("match", _pi), ("sets", _pi), ("K", C.c_double * 4), ("sigma", C.c_double), ("min_parallax", C.c_double),
        ("min_triangulated", C.c_int32), ("pad", C.c_int32),
    ]


class vba_two_view_result(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("ok", C.c_int32), ("model", C.c_int32), ("reason", C.c_int32), ("best_hyp_h", C.c_int32),
        ("best_hyp_f", C.c_int32), ("n_inliers_h", C.c_int32), ("n_inliers_f", C.c_int32), ("n_rt", C.c_int32), ("best_rt", C.c_int32),
        ("rt_good", C.c_int32 * 8), ("score_h", C.c_double), ("score_f", C.c_double), ("rh", C.c_double), ("H21", C.c_double * 9),
        ("F21", C.c_double * 9), ("rt_parallax", C.c_double * 8), ("R21", C.c_double * 9), ("t21", C.c_double * 3),
        ("inlier_h", _pu8), ("inlier_f", _pu8), ("x3d", _pd), ("triangulated", _pu8), ("hyp_score_h", _pd), ("hyp_score_f", _pd),
    ]


TV_MODEL_H, TV_MODEL_F = 1, 2


@dataclass
class TwoViewProblem:
    """One frame pair of Initializer::Initialize (src/Initializer.cpp:36-130) as flat arrays: frame 1 = reference, frame 2 =
    current, ALL their keypoints, the matches and the 8-sets the caller drew."""
    uv1: np.ndarray                # [n_keys1,2]
    uv2: np.ndarray                # [n_keys2,2]
    match: np.ndarray              # [n_matches,2] int32
    sets: np.ndarray               # [n_hyp,8] int32
    K: np.ndarray                  # [4] fx fy cx cy
    sigma: float = 1.0
    min_parallax: float = 1.0
    min_triangulated: int = 50
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        self.uv1 = _f64(self.uv1, (-1, 2)); self.uv2 = _f64(self.uv2, (-1, 2))
        self.match = np.ascontiguousarray(self.match, dtype=np.int32).reshape(-1, 2)
        self.sets = np.ascontiguousarray(self.sets, dtype=np.int32).reshape(-1, 8)
        self.K = _f64(self.K, (4,))

    n_keys1 = property(lambda self: self.uv1.shape[0])
    n_keys2 = property(lambda self: self.uv2.shape[0])
    n_matches = property(lambda self: self.match.shape[0])
    n_hyp = property(lambda self: self.sets.shape[0])

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        q.__post_init__()
        return q

    def as_struct(self) -> vba_two_view_problem:
        s = vba_two_view_problem()
        s.n_keys1, s.n_keys2, s.n_matches, s.n_hyp = self.n_keys1, self.n_keys2, self.n_matches, self.n_hyp
        s.uv1, s.uv2 = self.uv1.ctypes.data_as(_pd), self.uv2.ctypes.data_as(_pd)
        s.match, s.sets = self.match.ctypes.data_as(_pi), self.sets.ctypes.data_as(_pi)
        s.K[:] = self.K.tolist()
        s.sigma, s.min_parallax, s.min_triangulated = float(self.sigma), float(self.min_parallax), int(self.min_triangulated)
        return s


@dataclass
class TwoViewResult:
    status: int
    ok: int
    model: int
    reason: int
    best_hyp_h: int
    best_hyp_f: int
    n_inliers_h: int
    n_inliers_f: int
    n_rt: int
    best_rt: int
    rt_good: np.ndarray             # [8]
    score_h: float
    score_f: float
    rh: float
    H21: np.ndarray                 # [3,3]
    F21: np.ndarray                 # [3,3]
    rt_parallax: np.ndarray         # [8]
    R21: np.ndarray                 # [3,3]
    t21: np.ndarray                 # [3]
    inlier_h: np.ndarray            # [n_matches] uint8
    inlier_f: np.ndarray
    x3d: np.ndarray                 # [n_keys1,3]
    triangulated: np.ndarray        # [n_keys1] uint8
    hyp_score_h: Optional[np.ndarray]
    hyp_score_f: Optional[np.ndarray]


class TwoViewResultBuf:
    """Caller-allocated result storage of one frame pair.  The buffers start from `fill` patterns so that a test can tell what
    the library wrote."""

    def __init__(self, p: TwoViewProblem, want_scores=True, fill=0):
        self.n, self.nk, self.nh, self.want = p.n_matches, p.n_keys1, p.n_hyp, want_scores
        self.ih = np.full(max(self.n, 1), fill, dtype=np.uint8)
        self.jf = np.full(max(self.n, 1), fill, dtype=np.uint8)
        self.x = np.full((max(self.nk, 1), 3), float(fill))
        self.tr = np.full(max(self.nk, 1), fill, dtype=np.uint8)
        self.sh = np.full(max(self.nh, 1), float(fill))
        self.sf = np.full(max(self.nh, 1), float(fill))
        self.s = vba_two_view_result()
        self.s.inlier_h, self.s.inlier_f = self.ih.ctypes.data_as(_pu8), self.jf.ctypes.data_as(_pu8)
        self.s.x3d, self.s.triangulated = self.x.ctypes.data_as(_pd), self.tr.ctypes.data_as(_pu8)
        if want_scores:
            self.s.hyp_score_h, self.s.hyp_score_f = self.sh.ctypes.data_as(_pd), self.sf.ctypes.data_as(_pd)

    def get(self) -> TwoViewResult:
        s = self.s
        a = lambda v, shape=None: np.array(v[:]).reshape(shape) if shape else np.array(v[:])
        return TwoViewResult(s.status, s.ok, s.model, s.reason, s.best_hyp_h, s.best_hyp_f, s.n_inliers_h, s.n_inliers_f, s.n_rt, s.best_rt,
                             a(s.rt_good), s.score_h, s.score_f, s.rh, a(s.H21, (3, 3)), a(s.F21, (3, 3)), a(s.rt_parallax), a(s.R21, (3, 3)),
                             a(s.t21), self.ih[:self.n].copy(), self.jf[:self.n].copy(), self.x[:self.nk].copy(), self.tr[:self.nk].copy(),
                             self.sh[:self.nh].copy() if self.want else None, self.sf[:self.nh].copy() if self.want else None)


# ---- matching for triangulation (include/vislam_ba.h: vba_search_tri_problem / vba_search_tri_result) ----
_pu32 = C.POINTER(C.c_uint32)
_pf = C.POINTER(C.c_float)


class vba_search_tri_problem(C.Structure):
    _fields_ = [
        ("n_keys1", C.c_int32), ("n_keys2", C.c_int32), ("desc1", _pu8), ("desc2", _pu8), ("has_mp1", _pu8), ("has_mp2", _pu8),
        ("n_nodes1", C.c_int32), ("n_nodes2", C.c_int32), ("node_id1", _pu32), ("node_id2", _pu32), ("node_begin1", _pi), ("node_begin2", _pi),
        ("node_feat1", _pi), ("node_feat2", _pi), ("uv1", _pd), ("uv2", _pd), ("angle1", _pf), ("angle2", _pf), ("oct2", _pu8),
        ("n_levels2", C.c_int32), ("level_sigma2_2", _pd), ("scale_2", _pd), ("F12", C.c_double * 9), ("epipole", C.c_double * 2),
        ("th_low", C.c_int32), ("check_orientation", C.c_int32), ("chi2_epi", C.c_double), ("epipole_r2", C.c_double),
    ]


class vba_search_tri_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_matches", C.c_int32), ("n_before_filter", C.c_int32), ("hist", C.c_int32 * 30), ("ind", C.c_int32 * 3),
                ("match12", _pi), ("best_dist", _pu8), ("state", _pu8), ("pairs", _pi)]


ST_MATCHED, ST_HAS_MP, ST_NO_NODE, ST_NO_CANDIDATE, ST_ORIENTATION = range(5)


def feat_vec_csr(fv):
    """a feature vector {node id: [keypoint indices]} as (node_id, node_begin, node_feat), nodes in ascending order like the std::map"""
    ids = sorted(fv)
    begin = np.zeros(len(ids) + 1, dtype=np.int32)
    for k, i in enumerate(ids):
        begin[k + 1] = begin[k] + len(fv[i])
    feat = np.array([a for i in ids for a in fv[i]], dtype=np.int32)
    return np.array(ids, dtype=np.uint32), begin, feat


@dataclass
class SearchTriProblem:
    """One keyframe pair of ORBmatcher::SearchForTriangulation (src/ORBmatcher.cpp:760-955) as flat arrays: keyframe 1 =
    mpCurrentKeyFrame, keyframe 2 = one neighbour, feature vectors in CSR form."""
    desc1: np.ndarray              # [n1,32] uint8
    desc2: np.ndarray              # [n2,32] uint8
    has_mp1: np.ndarray            # [n1] uint8
    has_mp2: np.ndarray            # [n2] uint8
    node_id1: np.ndarray           # [nodes1] uint32, strictly ascending
    node_begin1: np.ndarray        # [nodes1 + 1] int32
    node_feat1: np.ndarray         # int32
    node_id2: np.ndarray
    node_begin2: np.ndarray
    node_feat2: np.ndarray
    uv1: np.ndarray                # [n1,2]
    uv2: np.ndarray                # [n2,2]
    angle1: np.ndarray             # [n1] float32
    angle2: np.ndarray             # [n2] float32
    oct2: np.ndarray               # [n2] uint8
    level_sigma2_2: np.ndarray     # [n_levels2]
    scale_2: np.ndarray            # [n_levels2]
    F12: np.ndarray                # [3,3]
    epipole: np.ndarray            # [2]
    th_low: int = 50
    check_orientation: bool = True
    chi2_epi: float = 3.84
    epipole_r2: float = 100.0
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        u8 = lambda a, shape: np.ascontiguousarray(a, dtype=np.uint8).reshape(shape)
        self.desc1 = u8(self.desc1, (-1, 32)); self.desc2 = u8(self.desc2, (-1, 32))
        self.has_mp1 = u8(self.has_mp1, (-1,)); self.has_mp2 = u8(self.has_mp2, (-1,)); self.oct2 = u8(self.oct2, (-1,))
        for k in ("node_id1", "node_id2"):
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=np.uint32).reshape(-1))
        for k in ("node_begin1", "node_begin2", "node_feat1", "node_feat2"):
            setattr(self, k, _i32(getattr(self, k)).reshape(-1))
        self.uv1 = _f64(self.uv1, (-1, 2)); self.uv2 = _f64(self.uv2, (-1, 2))
        self.angle1 = np.ascontiguousarray(self.angle1, dtype=np.float32).reshape(-1)
        self.angle2 = np.ascontiguousarray(self.angle2, dtype=np.float32).reshape(-1)
        self.level_sigma2_2 = _f64(self.level_sigma2_2, (-1,)); self.scale_2 = _f64(self.scale_2, (-1,))
        self.F12 = _f64(self.F12, (3, 3)); self.epipole = _f64(self.epipole, (2,))

    n_keys1 = property(lambda self: self.desc1.shape[0])
    n_keys2 = property(lambda self: self.desc2.shape[0])
    n_levels2 = property(lambda self: self.level_sigma2_2.shape[0])

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        q.__post_init__()
        return q

    def as_struct(self) -> vba_search_tri_problem:
        s = vba_search_tri_problem()
        p = lambda a, t: a.ctypes.data_as(t)
        s.n_keys1, s.n_keys2 = self.n_keys1, self.n_keys2
        s.desc1, s.desc2, s.has_mp1, s.has_mp2 = p(self.desc1, _pu8), p(self.desc2, _pu8), p(self.has_mp1, _pu8), p(self.has_mp2, _pu8)
        s.n_nodes1, s.n_nodes2 = self.node_id1.shape[0], self.node_id2.shape[0]
        s.node_id1, s.node_id2 = p(self.node_id1, _pu32), p(self.node_id2, _pu32)
        s.node_begin1, s.node_begin2 = p(self.node_begin1, _pi), p(self.node_begin2, _pi)
        s.node_feat1, s.node_feat2 = p(self.node_feat1, _pi), p(self.node_feat2, _pi)
        s.uv1, s.uv2, s.angle1, s.angle2, s.oct2 = p(self.uv1, _pd), p(self.uv2, _pd), p(self.angle1, _pf), p(self.angle2, _pf), p(self.oct2, _pu8)
        s.n_levels2 = self.n_levels2
        s.level_sigma2_2, s.scale_2 = p(self.level_sigma2_2, _pd), p(self.scale_2, _pd)
        s.F12[:] = self.F12.ravel().tolist()
        s.epipole[:] = self.epipole.tolist()
        s.th_low, s.check_orientation = int(self.th_low), int(bool(self.check_orientation))
        s.chi2_epi, s.epipole_r2 = float(self.chi2_epi), float(self.epipole_r2)
        return s


@dataclass
class SearchTriResult:
    status: int
    n_matches: int
    n_before_filter: int
    hist: np.ndarray                # [30]
    ind: np.ndarray                 # [3]
    match12: np.ndarray             # [n1] int32
    best_dist: np.ndarray           # [n1] uint8
    state: np.ndarray               # [n1] uint8
    pairs: np.ndarray               # [n_matches,2] int32


class SearchTriResultBuf:
    """Caller-allocated result storage of one keyframe pair."""

    def __init__(self, p: SearchTriProblem):
        self.n = p.n_keys1
        m = max(self.n, 1)
        self.m12 = np.full(m, -7, dtype=np.int32)
        self.bd = np.full(m, 7, dtype=np.uint8)
        self.st = np.full(m, 255, dtype=np.uint8)
        self.pr = np.full((m, 2), -7, dtype=np.int32)
        self.s = vba_search_tri_result()
        self.s.match12, self.s.best_dist, self.s.state, self.s.pairs = (self.m12.ctypes.data_as(_pi), self.bd.ctypes.data_as(_pu8),
                                                                        self.st.ctypes.data_as(_pu8), self.pr.ctypes.data_as(_pi))

    def get(self) -> SearchTriResult:
        s = self.s
        return SearchTriResult(s.status, s.n_matches, s.n_before_filter, np.array(s.hist[:]), np.array(s.ind[:]), self.m12[:self.n].copy(),
                               self.bd[:self.n].copy(), self.st[:self.n].copy(), self.pr[:max(min(s.n_matches, self.n), 0)].copy())


# ---- projection search for map-point fusion (include/vislam_ba.h: vba_fuse_problem / vba_fuse_result) ----
_pu16 = C.POINTER(C.c_uint16)
_pi8 = C.POINTER(C.c_int8)


class vba_fuse_problem(C.Structure):
    _fields_ = [
        ("Rcw", C.c_double * 9), ("tcw", C.c_double * 3), ("Ow", C.c_double * 3), ("K", C.c_double * 4), ("bounds", C.c_double * 4),
        ("n_keys", C.c_int32), ("n_levels", C.c_int32), ("desc", _pu8), ("uv", _pd), ("oct", _pu8), ("scale", _pd), ("inv_level_sigma2", _pd),
        ("log_scale_factor", C.c_double), ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("grid_inv_w", C.c_double), ("grid_inv_h", C.c_double),
        ("cell_begin", _pi), ("cell_feat", _pi), ("n_pt", C.c_int32), ("th_low", C.c_int32), ("pos", _pd), ("normal", _pd), ("dist_min", _pd),
        ("dist_max", _pd), ("pred_max", _pd), ("pt_desc", _pu8), ("skip", _pu8), ("th", C.c_double), ("cos_view", C.c_double),
        ("check_reproj", C.c_int32), ("chi2_reproj", C.c_double),
    ]


class vba_fuse_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_found", C.c_int32), ("best_idx", _pi), ("best_dist", _pu16), ("level", _pi8), ("uv", _pd), ("state", _pu8)]


(FU_FOUND, FU_SKIPPED, FU_BEHIND, FU_NOT_IN_IMAGE, FU_DISTANCE, FU_VIEW_ANGLE, FU_LEVEL, FU_EMPTY_AREA, FU_NO_MATCH) = range(9)


def grid_csr(uv, bounds, cols, rows, inv_w, inv_h):
    """Frame::AssignFeaturesToGrid with PosInGrid as (cell_begin, cell_feat): posX = round((x - mnMinX) * mfGridElementWidthInv) in
    float32 with C round, a keypoint outside 0 .. cols - 1 x 0 .. rows - 1 is in no cell; cell (ix, iy) stands at ix * rows + iy and
    lists its keypoints in ascending index order, as the push_back loop leaves them"""
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)

    def c_round(t):
        return (np.sign(t) * np.floor(np.abs(t) + np.float32(0.5))).astype(np.int64)

    px = c_round((uv[:, 0] - np.float32(bounds[0])) * np.float32(inv_w))
    py = c_round((uv[:, 1] - np.float32(bounds[2])) * np.float32(inv_h))
    ok = (px >= 0) & (px < cols) & (py >= 0) & (py < rows)
    cell = (px * rows + py)[ok]
    idx = np.nonzero(ok)[0]
    begin = np.zeros(cols * rows + 1, dtype=np.int32)
    begin[1:] = np.cumsum(np.bincount(cell, minlength=cols * rows))
    return begin, idx[np.argsort(cell, kind="stable")].astype(np.int32)


@dataclass
class FuseProblem:
    """One ORBmatcher::Fuse call (src/ORBmatcher.cpp:958-1254, the search half) as flat arrays: one keyframe with its grid in CSR form
    and one list of map points."""
    Rcw: np.ndarray                # [3,3]
    tcw: np.ndarray                # [3]
    Ow: np.ndarray                 # [3]
    K: np.ndarray                  # [4] fx fy cx cy
    bounds: np.ndarray             # [4] mnMinX mnMaxX mnMinY mnMaxY
    desc: np.ndarray               # [n_keys,32] uint8
    uv: np.ndarray                 # [n_keys,2]
    oct: np.ndarray                # [n_keys] uint8
    scale: np.ndarray              # [n_levels]
    inv_level_sigma2: np.ndarray   # [n_levels]
    log_scale_factor: float
    grid_cols: int
    grid_rows: int
    grid_inv_w: float
    grid_inv_h: float
    cell_begin: np.ndarray         # [cols * rows + 1] int32
    cell_feat: np.ndarray          # int32
    pos: np.ndarray                # [n_pt,3]
    normal: np.ndarray             # [n_pt,3]
    dist_min: np.ndarray           # [n_pt]
    dist_max: np.ndarray           # [n_pt]
    pred_max: np.ndarray           # [n_pt]
    pt_desc: np.ndarray            # [n_pt,32] uint8
    skip: np.ndarray               # [n_pt] uint8
    th: float = 3.0
    th_low: int = 50
    cos_view: float = 0.5
    check_reproj: bool = True
    chi2_reproj: float = 5.99
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        u8 = lambda a, shape: np.ascontiguousarray(a, dtype=np.uint8).reshape(shape)
        self.Rcw = _f64(self.Rcw, (3, 3)); self.tcw = _f64(self.tcw, (3,)); self.Ow = _f64(self.Ow, (3,))
        self.K = _f64(self.K, (4,)); self.bounds = _f64(self.bounds, (4,))
        self.desc = u8(self.desc, (-1, 32)); self.oct = u8(self.oct, (-1,)); self.uv = _f64(self.uv, (-1, 2))
        self.scale = _f64(self.scale, (-1,)); self.inv_level_sigma2 = _f64(self.inv_level_sigma2, (-1,))
        self.cell_begin = _i32(self.cell_begin).reshape(-1); self.cell_feat = _i32(self.cell_feat).reshape(-1)
        self.pos = _f64(self.pos, (-1, 3)); self.normal = _f64(self.normal, (-1, 3))
        self.dist_min = _f64(self.dist_min, (-1,)); self.dist_max = _f64(self.dist_max, (-1,)); self.pred_max = _f64(self.pred_max, (-1,))
        self.pt_desc = u8(self.pt_desc, (-1, 32)); self.skip = u8(self.skip, (-1,))

    n_keys = property(lambda self: self.desc.shape[0])
    n_pt = property(lambda self: self.pos.shape[0])
    n_levels = property(lambda self: self.scale.shape[0])

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        q.__post_init__()
        return q

    def as_struct(self) -> vba_fuse_problem:
        s = vba_fuse_problem()
        p = lambda a, t: a.ctypes.data_as(t)
        s.Rcw[:] = self.Rcw.ravel().tolist(); s.tcw[:] = self.tcw.tolist(); s.Ow[:] = self.Ow.tolist()
        s.K[:] = self.K.tolist(); s.bounds[:] = self.bounds.tolist()
        s.n_keys, s.n_levels, s.n_pt = self.n_keys, self.n_levels, self.n_pt
        s.desc, s.uv, s.oct = p(self.desc, _pu8), p(self.uv, _pd), p(self.oct, _pu8)
        s.scale, s.inv_level_sigma2 = p(self.scale, _pd), p(self.inv_level_sigma2, _pd)
        s.log_scale_factor = float(self.log_scale_factor)
        s.grid_cols, s.grid_rows, s.grid_inv_w, s.grid_inv_h = int(self.grid_cols), int(self.grid_rows), float(self.grid_inv_w), float(self.grid_inv_h)
        s.cell_begin, s.cell_feat = p(self.cell_begin, _pi), p(self.cell_feat, _pi)
        s.pos, s.normal, s.dist_min, s.dist_max, s.pred_max = p(self.pos, _pd), p(self.normal, _pd), p(self.dist_min, _pd), p(self.dist_max, _pd), p(self.pred_max, _pd)
        s.pt_desc, s.skip = p(self.pt_desc, _pu8), p(self.skip, _pu8)
        s.th, s.th_low, s.cos_view = float(self.th), int(self.th_low), float(self.cos_view)
        s.check_reproj, s.chi2_reproj = int(bool(self.check_reproj)), float(self.chi2_reproj)
        return s


@dataclass
class FuseResult:
    status: int
    n_found: int
    best_idx: np.ndarray            # [n_pt] int32
    best_dist: np.ndarray           # [n_pt] uint16
    level: np.ndarray               # [n_pt] int8
    uv: np.ndarray                  # [n_pt,2]
    state: np.ndarray               # [n_pt] uint8


class FuseResultBuf:
    """Caller-allocated result storage of one problem."""

    def __init__(self, p: FuseProblem):
        self.n = p.n_pt
        m = max(self.n, 1)
        self.bi = np.full(m, -7, dtype=np.int32)
        self.bd = np.full(m, 7, dtype=np.uint16)
        self.lv = np.full(m, 77, dtype=np.int8)
        self.uv = np.full((m, 2), -7.0)
        self.st = np.full(m, 255, dtype=np.uint8)
        self.s = vba_fuse_result()
        self.s.status, self.s.n_found = -7, -7
        self.s.best_idx, self.s.best_dist, self.s.level, self.s.uv, self.s.state = (self.bi.ctypes.data_as(_pi), self.bd.ctypes.data_as(_pu16),
                                                                                  self.lv.ctypes.data_as(_pi8), self.uv.ctypes.data_as(_pd),
                                                                                  self.st.ctypes.data_as(_pu8))

    def get(self) -> FuseResult:
        n = self.n
        return FuseResult(self.s.status, self.s.n_found, self.bi[:n].copy(), self.bd[:n].copy(), self.lv[:n].copy(), self.uv[:n].copy(), self.st[:n].copy())


# ---- Sim3 projection matching (include/vislam_ba.h: vba_search_sim3_problem / vba_search_sim3_result) ----
class vba_search_sim3_kf(C.Structure):
    _fields_ = [
        ("Rcw", C.c_double * 9), ("tcw", C.c_double * 3), ("bounds", C.c_double * 4), ("n_keys", C.c_int32), ("n_levels", C.c_int32),
        ("desc", _pu8), ("uv", _pd), ("oct", _pu8), ("scale", _pd), ("log_scale_factor", C.c_double), ("grid_cols", C.c_int32),
        ("grid_rows", C.c_int32), ("grid_inv_w", C.c_double), ("grid_inv_h", C.c_double), ("cell_begin", _pi), ("cell_feat", _pi),
        ("has_pt", _pu8), ("matched", _pu8), ("pos", _pd), ("dist_min", _pd), ("dist_max", _pd), ("pred_max", _pd), ("pt_desc", _pu8),
    ]


class vba_search_sim3_problem(C.Structure):
    _fields_ = [("kf1", vba_search_sim3_kf), ("kf2", vba_search_sim3_kf), ("K", C.c_double * 4), ("s12", C.c_double), ("R12", C.c_double * 9),
                ("t12", C.c_double * 3), ("th", C.c_double), ("th_high", C.c_int32)]


class vba_search_sim3_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_found", C.c_int32), ("match1", _pi), ("match2", _pi), ("best_dist1", _pu16), ("best_dist2", _pu16),
                ("level1", _pi8), ("level2", _pi8), ("state1", _pu8), ("state2", _pu8), ("match12", _pi)]


(SS_FOUND, SS_NO_POINT, SS_MATCHED, SS_BEHIND, SS_NOT_IN_IMAGE, SS_DISTANCE, SS_LEVEL, SS_EMPTY_AREA, SS_NO_MATCH) = range(9)


@dataclass
class SearchSim3KF:
    """One keyframe of a SearchBySim3 call as flat arrays: as a search target (pose, bounds, keypoints, scale table, grid in CSR
    form) and as a source (its own map points, per keypoint)."""
    Rcw: np.ndarray                # [3,3]
    tcw: np.ndarray                # [3]
    bounds: np.ndarray             # [4] mnMinX mnMaxX mnMinY mnMaxY
    desc: np.ndarray               # [n_keys,32] uint8
    uv: np.ndarray                 # [n_keys,2]
    oct: np.ndarray                # [n_keys] uint8
    scale: np.ndarray              # [n_levels]
    log_scale_factor: float
    grid_cols: int
    grid_rows: int
    grid_inv_w: float
    grid_inv_h: float
    cell_begin: np.ndarray         # [cols * rows + 1] int32
    cell_feat: np.ndarray          # int32
    has_pt: np.ndarray             # [n_keys] uint8
    matched: np.ndarray            # [n_keys] uint8
    pos: np.ndarray                # [n_keys,3]
    dist_min: np.ndarray           # [n_keys]
    dist_max: np.ndarray           # [n_keys]
    pred_max: np.ndarray           # [n_keys]
    pt_desc: np.ndarray            # [n_keys,32] uint8

    def __post_init__(self):
        u8 = lambda a, shape: np.ascontiguousarray(a, dtype=np.uint8).reshape(shape)
        self.Rcw = _f64(self.Rcw, (3, 3)); self.tcw = _f64(self.tcw, (3,)); self.bounds = _f64(self.bounds, (4,))
        self.desc = u8(self.desc, (-1, 32)); self.oct = u8(self.oct, (-1,)); self.uv = _f64(self.uv, (-1, 2))
        self.scale = _f64(self.scale, (-1,))
        self.cell_begin = _i32(self.cell_begin).reshape(-1); self.cell_feat = _i32(self.cell_feat).reshape(-1)
        self.has_pt = u8(self.has_pt, (-1,)); self.matched = u8(self.matched, (-1,))
        self.pos = _f64(self.pos, (-1, 3))
        self.dist_min = _f64(self.dist_min, (-1,)); self.dist_max = _f64(self.dist_max, (-1,)); self.pred_max = _f64(self.pred_max, (-1,))
        self.pt_desc = u8(self.pt_desc, (-1, 32))

    n_keys = property(lambda self: self.desc.shape[0])
    n_levels = property(lambda self: self.scale.shape[0])

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        q.__post_init__()
        return q

    def fill(self, s: vba_search_sim3_kf):
        p = lambda a, t: a.ctypes.data_as(t)
        s.Rcw[:] = self.Rcw.ravel().tolist(); s.tcw[:] = self.tcw.tolist(); s.bounds[:] = self.bounds.tolist()
        s.n_keys, s.n_levels = self.n_keys, self.n_levels
        s.desc, s.uv, s.oct, s.scale = p(self.desc, _pu8), p(self.uv, _pd), p(self.oct, _pu8), p(self.scale, _pd)
        s.log_scale_factor = float(self.log_scale_factor)
        s.grid_cols, s.grid_rows, s.grid_inv_w, s.grid_inv_h = int(self.grid_cols), int(self.grid_rows), float(self.grid_inv_w), float(self.grid_inv_h)
        s.cell_begin, s.cell_feat = p(self.cell_begin, _pi), p(self.cell_feat, _pi)
        s.has_pt, s.matched, s.pos = p(self.has_pt, _pu8), p(self.matched, _pu8), p(self.pos, _pd)
        s.dist_min, s.dist_max, s.pred_max, s.pt_desc = p(self.dist_min, _pd), p(self.dist_max, _pd), p(self.pred_max, _pd), p(self.pt_desc, _pu8)


@dataclass
class SearchSim3Problem:
    """One ORBmatcher::SearchBySim3 call (src/ORBmatcher.cpp:1258-1496): two keyframes and the Sim3 between them."""
    kf1: SearchSim3KF
    kf2: SearchSim3KF
    K: np.ndarray                  # [4] fx fy cx cy of keyframe 1
    s12: float
    R12: np.ndarray                # [3,3]
    t12: np.ndarray                # [3]
    th: float = 7.5
    th_high: int = 100
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        self.K = _f64(self.K, (4,)); self.R12 = _f64(self.R12, (3, 3)); self.t12 = _f64(self.t12, (3,))

    def copy(self, **changes):
        """a copy with fields replaced; kf1 / kf2 take a SearchSim3KF or a dict of changes to the keyframe"""
        import copy as _c
        q = _c.copy(self)
        for k, v in changes.items():
            setattr(q, k, getattr(self, k).copy(**v) if k in ("kf1", "kf2") and isinstance(v, dict) else v)
        q.__post_init__()
        return q

    def as_struct(self) -> vba_search_sim3_problem:
        s = vba_search_sim3_problem()
        self.kf1.fill(s.kf1); self.kf2.fill(s.kf2)
        s.K[:] = self.K.tolist(); s.R12[:] = self.R12.ravel().tolist(); s.t12[:] = self.t12.tolist()
        s.s12, s.th, s.th_high = float(self.s12), float(self.th), int(self.th_high)
        return s


@dataclass
class SearchSim3Result:
    status: int
    n_found: int
    match1: np.ndarray              # [n_keys1] int32
    match2: np.ndarray              # [n_keys2] int32
    best_dist1: np.ndarray          # uint16
    best_dist2: np.ndarray
    level1: np.ndarray              # int8
    level2: np.ndarray
    state1: np.ndarray              # uint8
    state2: np.ndarray
    match12: np.ndarray             # [n_keys1] int32


class SearchSim3ResultBuf:
    """Caller-allocated result storage of one pair."""

    def __init__(self, p: SearchSim3Problem):
        self.n = (p.kf1.n_keys, p.kf2.n_keys)
        m = [max(k, 1) for k in self.n]
        self.ma = [np.full(k, -7, dtype=np.int32) for k in m]
        self.bd = [np.full(k, 7, dtype=np.uint16) for k in m]
        self.lv = [np.full(k, 77, dtype=np.int8) for k in m]
        self.st = [np.full(k, 255, dtype=np.uint8) for k in m]
        self.m12 = np.full(m[0], -7, dtype=np.int32)
        s = self.s = vba_search_sim3_result()
        s.status, s.n_found = -7, -7
        s.match1, s.match2 = (a.ctypes.data_as(_pi) for a in self.ma)
        s.best_dist1, s.best_dist2 = (a.ctypes.data_as(_pu16) for a in self.bd)
        s.level1, s.level2 = (a.ctypes.data_as(_pi8) for a in self.lv)
        s.state1, s.state2 = (a.ctypes.data_as(_pu8) for a in self.st)
        s.match12 = self.m12.ctypes.data_as(_pi)

    def untouched(self):
        """nothing was written since construction"""
        return (self.s.status == -7 and self.s.n_found == -7 and (self.m12 == -7).all() and all((a == -7).all() for a in self.ma) and
                all((a == 7).all() for a in self.bd) and all((a == 77).all() for a in self.lv) and all((a == 255).all() for a in self.st))

    def get(self) -> SearchSim3Result:
        n1, n2 = self.n
        return SearchSim3Result(self.s.status, self.s.n_found, self.ma[0][:n1].copy(), self.ma[1][:n2].copy(), self.bd[0][:n1].copy(),
                                self.bd[1][:n2].copy(), self.lv[0][:n1].copy(), self.lv[1][:n2].copy(), self.st[0][:n1].copy(),
                                self.st[1][:n2].copy(), self.m12[:n1].copy())


# ---- projection matching for tracking (include/vislam_ba.h: vba_search_proj_problem / vba_search_proj_result) ----
_pf = C.POINTER(C.c_float)
SEARCH_PROJ_LAST_FRAME, SEARCH_PROJ_LOCAL_MAP = 0, 1
SEARCH_PROJ_MAX_KEYS = 16384


class vba_search_proj_problem(C.Structure):
    _fields_ = [
        ("mode", C.c_int32), ("check_orientation", C.c_int32), ("Rcw", C.c_double * 9), ("tcw", C.c_double * 3), ("Ow", C.c_double * 3),
        ("K", C.c_double * 4), ("bounds", C.c_double * 4), ("n_keys", C.c_int32), ("n_levels", C.c_int32), ("desc", _pu8), ("uv", _pd),
        ("oct", _pu8), ("angle", _pf), ("scale", _pd), ("log_scale_factor", C.c_double), ("grid_cols", C.c_int32), ("grid_rows", C.c_int32),
        ("grid_inv_w", C.c_double), ("grid_inv_h", C.c_double), ("cell_begin", _pi), ("cell_feat", _pi), ("occupied", _pu8),
        ("n_q", C.c_int32), ("th_high", C.c_int32), ("q_pos", _pd), ("q_desc", _pu8), ("q_skip", _pu8), ("q_blocks", _pu8), ("q_oct", _pu8),
        ("q_angle", _pf), ("q_normal", _pd), ("q_dist_min", _pd), ("q_dist_max", _pd), ("q_pred_max", _pd), ("th", C.c_double),
        ("nn_ratio", C.c_float), ("cos_view", C.c_double),
    ]


class vba_search_proj_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_matches", C.c_int32), ("n_before_filter", C.c_int32), ("hist", C.c_int32 * 30), ("ind", C.c_int32 * 3),
                ("rounds", C.c_int32), ("best_idx", _pi), ("best_dist", _pu16), ("best_dist2", _pu16), ("level", _pi8), ("view_cos", _pd), ("uv", _pd),
                ("bin", _pu8), ("state", _pu8), ("key_match", _pi)]


# the states of the two modes
(SPL_MATCHED, SPL_SKIPPED, SPL_BEHIND, SPL_NOT_IN_IMAGE, SPL_EMPTY_AREA, SPL_NO_MATCH, SPL_ROTATION) = range(7)
(SPM_MATCHED, SPM_SKIPPED, SPM_BEHIND, SPM_NOT_IN_IMAGE, SPM_DISTANCE, SPM_VIEW_ANGLE, SPM_LEVEL, SPM_EMPTY_AREA, SPM_NO_MATCH, SPM_RATIO) = range(10)


@dataclass
class SearchProjProblem:
    """One call of a tracking matcher as flat arrays: one frame with its grid in CSR form and one ORDERED list of queries.  mode
    SEARCH_PROJ_LAST_FRAME is ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cpp:1511-1665), mode
    SEARCH_PROJ_LOCAL_MAP is Frame::isInFrustum with SearchByProjection(F, vpMapPoints, th) (:63-156).  The arrays of the other mode
    may stay None."""
    mode: int
    Rcw: np.ndarray                # [3,3]
    tcw: np.ndarray                # [3]
    K: np.ndarray                  # [4] fx fy cx cy
    bounds: np.ndarray             # [4] mnMinX mnMaxX mnMinY mnMaxY
    desc: np.ndarray               # [n_keys,32] uint8
    uv: np.ndarray                 # [n_keys,2]
    oct: np.ndarray                # [n_keys] uint8
    scale: np.ndarray              # [n_levels]
    grid_cols: int
    grid_rows: int
    grid_inv_w: float
    grid_inv_h: float
    cell_begin: np.ndarray         # [cols * rows + 1] int32
    cell_feat: np.ndarray          # int32
    occupied: np.ndarray           # [n_keys] uint8
    q_pos: np.ndarray              # [n_q,3]
    q_desc: np.ndarray             # [n_q,32] uint8
    q_skip: np.ndarray             # [n_q] uint8
    q_blocks: np.ndarray           # [n_q] uint8
    th: float = 15.0
    th_high: int = 100
    Ow: np.ndarray = None          # [3] local-map mode
    log_scale_factor: float = 0.0
    angle: np.ndarray = None       # [n_keys] float32, last-frame mode with check_orientation
    q_oct: np.ndarray = None       # [n_q] uint8, last-frame mode
    q_angle: np.ndarray = None     # [n_q] float32
    q_normal: np.ndarray = None    # [n_q,3] local-map mode, as the next three
    q_dist_min: np.ndarray = None
    q_dist_max: np.ndarray = None
    q_pred_max: np.ndarray = None
    nn_ratio: float = 0.8
    cos_view: float = 0.5
    check_orientation: bool = True
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        u8 = lambda a, shape: np.ascontiguousarray(a, dtype=np.uint8).reshape(shape)
        opt = lambda a, f, *s: None if a is None else f(a, *s)
        f32 = lambda a, shape: np.ascontiguousarray(a, dtype=np.float32).reshape(shape)
        self.Rcw = _f64(self.Rcw, (3, 3)); self.tcw = _f64(self.tcw, (3,)); self.Ow = _f64(np.zeros(3) if self.Ow is None else self.Ow, (3,))
        self.K = _f64(self.K, (4,)); self.bounds = _f64(self.bounds, (4,))
        self.desc = u8(self.desc, (-1, 32)); self.oct = u8(self.oct, (-1,)); self.uv = _f64(self.uv, (-1, 2))
        self.scale = _f64(self.scale, (-1,)); self.occupied = u8(self.occupied, (-1,))
        self.cell_begin = _i32(self.cell_begin).reshape(-1); self.cell_feat = _i32(self.cell_feat).reshape(-1)
        self.q_pos = _f64(self.q_pos, (-1, 3)); self.q_desc = u8(self.q_desc, (-1, 32))
        self.q_skip = u8(self.q_skip, (-1,)); self.q_blocks = u8(self.q_blocks, (-1,))
        self.angle = opt(self.angle, f32, (-1,)); self.q_angle = opt(self.q_angle, f32, (-1,)); self.q_oct = opt(self.q_oct, u8, (-1,))
        self.q_normal = opt(self.q_normal, _f64, (-1, 3))
        self.q_dist_min = opt(self.q_dist_min, _f64, (-1,)); self.q_dist_max = opt(self.q_dist_max, _f64, (-1,))
        self.q_pred_max = opt(self.q_pred_max, _f64, (-1,))
        self.nn_ratio = float(np.float32(self.nn_ratio))

    n_keys = property(lambda self: self.desc.shape[0])
    n_q = property(lambda self: self.q_pos.shape[0])
    n_levels = property(lambda self: self.scale.shape[0])
    local = property(lambda self: self.mode == SEARCH_PROJ_LOCAL_MAP)

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        q.__post_init__()
        return q

    def as_struct(self) -> vba_search_proj_problem:
        s = vba_search_proj_problem()
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        s.mode, s.check_orientation = int(self.mode), int(bool(self.check_orientation))
        s.Rcw[:] = self.Rcw.ravel().tolist(); s.tcw[:] = self.tcw.tolist(); s.Ow[:] = self.Ow.tolist()
        s.K[:] = self.K.tolist(); s.bounds[:] = self.bounds.tolist()
        s.n_keys, s.n_levels, s.n_q = self.n_keys, self.n_levels, self.n_q
        s.desc, s.uv, s.oct, s.angle, s.scale = p(self.desc, _pu8), p(self.uv, _pd), p(self.oct, _pu8), p(self.angle, _pf), p(self.scale, _pd)
        s.log_scale_factor = float(self.log_scale_factor)
        s.grid_cols, s.grid_rows, s.grid_inv_w, s.grid_inv_h = int(self.grid_cols), int(self.grid_rows), float(self.grid_inv_w), float(self.grid_inv_h)
        s.cell_begin, s.cell_feat, s.occupied = p(self.cell_begin, _pi), p(self.cell_feat, _pi), p(self.occupied, _pu8)
        s.q_pos, s.q_desc, s.q_skip, s.q_blocks = p(self.q_pos, _pd), p(self.q_desc, _pu8), p(self.q_skip, _pu8), p(self.q_blocks, _pu8)
        s.q_oct, s.q_angle, s.q_normal = p(self.q_oct, _pu8), p(self.q_angle, _pf), p(self.q_normal, _pd)
        s.q_dist_min, s.q_dist_max, s.q_pred_max = p(self.q_dist_min, _pd), p(self.q_dist_max, _pd), p(self.q_pred_max, _pd)
        s.th, s.th_high, s.nn_ratio, s.cos_view = float(self.th), int(self.th_high), float(self.nn_ratio), float(self.cos_view)
        return s


@dataclass
class SearchProjResult:
    status: int
    n_matches: int
    n_before_filter: int
    hist: np.ndarray                # [30]
    ind: np.ndarray                 # [3]
    rounds: int
    best_idx: np.ndarray            # [n_q] int32
    best_dist: np.ndarray           # [n_q] uint16
    best_dist2: np.ndarray          # [n_q] uint16
    level: np.ndarray               # [n_q] int8
    view_cos: np.ndarray            # [n_q]
    uv: np.ndarray                  # [n_q,2]
    bin: np.ndarray                 # [n_q] uint8
    state: np.ndarray               # [n_q] uint8
    key_match: np.ndarray           # [n_keys] int32


class SearchProjResultBuf:
    """Caller-allocated result storage of one problem."""

    def __init__(self, p: SearchProjProblem):
        self.n, self.nk = p.n_q, p.n_keys
        m, mk = max(self.n, 1), max(self.nk, 1)
        self.bi = np.full(m, -7, dtype=np.int32)
        self.bd = np.full(m, 7, dtype=np.uint16)
        self.bd2 = np.full(m, 7, dtype=np.uint16)
        self.lv = np.full(m, 77, dtype=np.int8)
        self.vc = np.full(m, -7.0)
        self.uv = np.full((m, 2), -7.0)
        self.bn = np.full(m, 77, dtype=np.uint8)
        self.st = np.full(m, 255, dtype=np.uint8)
        self.km = np.full(mk, -7, dtype=np.int32)
        s = self.s = vba_search_proj_result()
        s.status, s.n_matches, s.n_before_filter, s.rounds = -7, -7, -7, -7
        s.best_idx, s.best_dist, s.best_dist2, s.level = (self.bi.ctypes.data_as(_pi), self.bd.ctypes.data_as(_pu16), self.bd2.ctypes.data_as(_pu16),
                                                          self.lv.ctypes.data_as(_pi8))
        s.view_cos, s.uv, s.bin, s.state, s.key_match = (self.vc.ctypes.data_as(_pd), self.uv.ctypes.data_as(_pd), self.bn.ctypes.data_as(_pu8),
                                                         self.st.ctypes.data_as(_pu8), self.km.ctypes.data_as(_pi))

    def untouched(self):
        """nothing was written since construction"""
        s = self.s
        return ((s.status, s.n_matches, s.n_before_filter, s.rounds) == (-7, -7, -7, -7) and (self.bi == -7).all() and (self.bd == 7).all() and
                (self.bd2 == 7).all() and (self.lv == 77).all() and (self.vc == -7.0).all() and (self.uv == -7.0).all() and (self.bn == 77).all() and
                (self.st == 255).all() and (self.km == -7).all() and not any(s.hist[:]) and not any(s.ind[:]))

    def get(self) -> SearchProjResult:
        s, n = self.s, self.n
        return SearchProjResult(s.status, s.n_matches, s.n_before_filter, np.array(s.hist[:]), np.array(s.ind[:]), s.rounds, self.bi[:n].copy(),
                                self.bd[:n].copy(), self.bd2[:n].copy(), self.lv[:n].copy(), self.vc[:n].copy(), self.uv[:n].copy(), self.bn[:n].copy(),
                                self.st[:n].copy(), self.km[:self.nk].copy())


# ---- projection matching for loop closure and relocalisation (include/vislam_ba.h: vba_search_proj_kf_problem / _result) ----
SEARCH_PROJ_KF_LOOP, SEARCH_PROJ_KF_RELOC = 0, 1
SEARCH_PROJ_KF_MAX_KEYS = 16384


class vba_search_proj_kf_problem(C.Structure):
    _fields_ = [
        ("mode", C.c_int32), ("check_orientation", C.c_int32), ("Rcw", C.c_double * 9), ("tcw", C.c_double * 3), ("Ow", C.c_double * 3),
        ("K", C.c_double * 4), ("bounds", C.c_double * 4), ("n_keys", C.c_int32), ("n_levels", C.c_int32), ("desc", _pu8), ("uv", _pd),
        ("oct", _pu8), ("angle", _pf), ("scale", _pd), ("log_scale_factor", C.c_double), ("grid_cols", C.c_int32), ("grid_rows", C.c_int32),
        ("grid_inv_w", C.c_double), ("grid_inv_h", C.c_double), ("cell_begin", _pi), ("cell_feat", _pi), ("occupied", _pu8),
        ("n_q", C.c_int32), ("th_dist", C.c_int32), ("th", C.c_double), ("cos_view", C.c_double), ("q_pos", _pd), ("q_desc", _pu8),
        ("q_skip", _pu8), ("q_normal", _pd), ("q_dist_min", _pd), ("q_dist_max", _pd), ("q_pred_max", _pd), ("q_angle", _pf),
    ]


class vba_search_proj_kf_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_matches", C.c_int32), ("n_before_filter", C.c_int32), ("hist", C.c_int32 * 30), ("ind", C.c_int32 * 3),
                ("rounds", C.c_int32), ("best_idx", _pi), ("best_dist", _pu16), ("level", _pi8), ("uv", _pd), ("bin", _pu8), ("state", _pu8),
                ("key_match", _pi)]


# the states of the two modes
(SKL_MATCHED, SKL_SKIPPED, SKL_BEHIND, SKL_NOT_IN_IMAGE, SKL_DISTANCE, SKL_VIEW_ANGLE, SKL_LEVEL, SKL_EMPTY_AREA, SKL_NO_MATCH) = range(9)
(SKR_MATCHED, SKR_SKIPPED, SKR_NOT_IN_IMAGE, SKR_DISTANCE, SKR_LEVEL, SKR_EMPTY_AREA, SKR_NO_MATCH, SKR_ROTATION) = range(8)


@dataclass
class SearchProjKfProblem:
    """One call of the loop-closure or the relocalisation matcher as flat arrays: one target (a keyframe in mode SEARCH_PROJ_KF_LOOP,
    ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th), src/ORBmatcher.cpp:354-475; a frame in mode SEARCH_PROJ_KF_RELOC,
    SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist), :1667-1797) with its grid in CSR form and one ORDERED list of
    queries.  The arrays of the other mode may stay None."""
    mode: int
    Rcw: np.ndarray                # [3,3]
    tcw: np.ndarray                # [3]
    Ow: np.ndarray                 # [3]
    K: np.ndarray                  # [4] fx fy cx cy
    bounds: np.ndarray             # [4] mnMinX mnMaxX mnMinY mnMaxY
    desc: np.ndarray               # [n_keys,32] uint8
    uv: np.ndarray                 # [n_keys,2]
    oct: np.ndarray                # [n_keys] uint8
    scale: np.ndarray              # [n_levels]
    log_scale_factor: float
    grid_cols: int
    grid_rows: int
    grid_inv_w: float
    grid_inv_h: float
    cell_begin: np.ndarray         # [cols * rows + 1] int32
    cell_feat: np.ndarray          # int32
    occupied: np.ndarray           # [n_keys] uint8
    q_pos: np.ndarray              # [n_q,3]
    q_desc: np.ndarray             # [n_q,32] uint8
    q_skip: np.ndarray             # [n_q] uint8
    q_dist_min: np.ndarray         # [n_q]
    q_dist_max: np.ndarray         # [n_q]
    q_pred_max: np.ndarray         # [n_q]
    th: float = 10.0
    th_dist: int = 50
    cos_view: float = 0.5
    q_normal: np.ndarray = None    # [n_q,3] loop mode
    angle: np.ndarray = None       # [n_keys] float32, reloc mode with check_orientation
    q_angle: np.ndarray = None     # [n_q] float32, reloc mode with check_orientation
    check_orientation: bool = True
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        u8 = lambda a, shape: np.ascontiguousarray(a, dtype=np.uint8).reshape(shape)
        opt = lambda a, f, *s: None if a is None else f(a, *s)
        f32 = lambda a, shape: np.ascontiguousarray(a, dtype=np.float32).reshape(shape)
        self.Rcw = _f64(self.Rcw, (3, 3)); self.tcw = _f64(self.tcw, (3,)); self.Ow = _f64(self.Ow, (3,))
        self.K = _f64(self.K, (4,)); self.bounds = _f64(self.bounds, (4,))
        self.desc = u8(self.desc, (-1, 32)); self.oct = u8(self.oct, (-1,)); self.uv = _f64(self.uv, (-1, 2))
        self.scale = _f64(self.scale, (-1,)); self.occupied = u8(self.occupied, (-1,))
        self.cell_begin = _i32(self.cell_begin).reshape(-1); self.cell_feat = _i32(self.cell_feat).reshape(-1)
        self.q_pos = _f64(self.q_pos, (-1, 3)); self.q_desc = u8(self.q_desc, (-1, 32)); self.q_skip = u8(self.q_skip, (-1,))
        self.q_dist_min = _f64(self.q_dist_min, (-1,)); self.q_dist_max = _f64(self.q_dist_max, (-1,)); self.q_pred_max = _f64(self.q_pred_max, (-1,))
        self.q_normal = opt(self.q_normal, _f64, (-1, 3))
        self.angle = opt(self.angle, f32, (-1,)); self.q_angle = opt(self.q_angle, f32, (-1,))

    n_keys = property(lambda self: self.desc.shape[0])
    n_q = property(lambda self: self.q_pos.shape[0])
    n_levels = property(lambda self: self.scale.shape[0])
    reloc = property(lambda self: self.mode == SEARCH_PROJ_KF_RELOC)

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        q.__post_init__()
        return q

    def as_struct(self) -> vba_search_proj_kf_problem:
        s = vba_search_proj_kf_problem()
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        s.mode, s.check_orientation = int(self.mode), int(bool(self.check_orientation))
        s.Rcw[:] = self.Rcw.ravel().tolist(); s.tcw[:] = self.tcw.tolist(); s.Ow[:] = self.Ow.tolist()
        s.K[:] = self.K.tolist(); s.bounds[:] = self.bounds.tolist()
        s.n_keys, s.n_levels, s.n_q = self.n_keys, self.n_levels, self.n_q
        s.desc, s.uv, s.oct, s.angle, s.scale = p(self.desc, _pu8), p(self.uv, _pd), p(self.oct, _pu8), p(self.angle, _pf), p(self.scale, _pd)
        s.log_scale_factor = float(self.log_scale_factor)
        s.grid_cols, s.grid_rows, s.grid_inv_w, s.grid_inv_h = int(self.grid_cols), int(self.grid_rows), float(self.grid_inv_w), float(self.grid_inv_h)
        s.cell_begin, s.cell_feat, s.occupied = p(self.cell_begin, _pi), p(self.cell_feat, _pi), p(self.occupied, _pu8)
        s.th_dist, s.th, s.cos_view = int(self.th_dist), float(self.th), float(self.cos_view)
        s.q_pos, s.q_desc, s.q_skip, s.q_normal = p(self.q_pos, _pd), p(self.q_desc, _pu8), p(self.q_skip, _pu8), p(self.q_normal, _pd)
        s.q_dist_min, s.q_dist_max, s.q_pred_max, s.q_angle = p(self.q_dist_min, _pd), p(self.q_dist_max, _pd), p(self.q_pred_max, _pd), p(self.q_angle, _pf)
        return s


@dataclass
class SearchProjKfResult:
    status: int
    n_matches: int
    n_before_filter: int
    hist: np.ndarray                # [30]
    ind: np.ndarray                 # [3]
    rounds: int
    best_idx: np.ndarray            # [n_q] int32
    best_dist: np.ndarray           # [n_q] uint16
    level: np.ndarray               # [n_q] int8
    uv: np.ndarray                  # [n_q,2]
    bin: np.ndarray                 # [n_q] uint8
    state: np.ndarray               # [n_q] uint8
    key_match: np.ndarray           # [n_keys] int32


class SearchProjKfResultBuf:
    """Caller-allocated result storage of one problem."""

    def __init__(self, p: SearchProjKfProblem):
        self.n, self.nk = p.n_q, p.n_keys
        m, mk = max(self.n, 1), max(self.nk, 1)
        self.bi = np.full(m, -7, dtype=np.int32)
        self.bd = np.full(m, 7, dtype=np.uint16)
        self.lv = np.full(m, 77, dtype=np.int8)
        self.uv = np.full((m, 2), -7.0)
        self.bn = np.full(m, 77, dtype=np.uint8)
        self.st = np.full(m, 255, dtype=np.uint8)
        self.km = np.full(mk, -7, dtype=np.int32)
        s = self.s = vba_search_proj_kf_result()
        s.status, s.n_matches, s.n_before_filter, s.rounds = -7, -7, -7, -7
        s.best_idx, s.best_dist, s.level = self.bi.ctypes.data_as(_pi), self.bd.ctypes.data_as(_pu16), self.lv.ctypes.data_as(_pi8)
        s.uv, s.bin, s.state, s.key_match = (self.uv.ctypes.data_as(_pd), self.bn.ctypes.data_as(_pu8), self.st.ctypes.data_as(_pu8),
                                             self.km.ctypes.data_as(_pi))

    def untouched(self):
        """nothing was written since construction"""
        s = self.s
        return ((s.status, s.n_matches, s.n_before_filter, s.rounds) == (-7, -7, -7, -7) and (self.bi == -7).all() and (self.bd == 7).all() and
                (self.lv == 77).all() and (self.uv == -7.0).all() and (self.bn == 77).all() and (self.st == 255).all() and (self.km == -7).all() and
                not any(s.hist[:]) and not any(s.ind[:]))

    def get(self) -> SearchProjKfResult:
        s, n = self.s, self.n
        return SearchProjKfResult(s.status, s.n_matches, s.n_before_filter, np.array(s.hist[:]), np.array(s.ind[:]), s.rounds, self.bi[:n].copy(),
                                  self.bd[:n].copy(), self.lv[:n].copy(), self.uv[:n].copy(), self.bn[:n].copy(), self.st[:n].copy(),
                                  self.km[:self.nk].copy())


# ---- bag-of-words matching (include/vislam_ba.h: vba_search_bow_problem / vba_search_bow_result) ----
SEARCH_BOW_KF_FRAME, SEARCH_BOW_KF_KF = 0, 1
SEARCH_BOW_MAX_KEYS = 16384


class vba_search_bow_problem(C.Structure):
    _fields_ = [
        ("mode", C.c_int32), ("check_orientation", C.c_int32), ("th_low", C.c_int32), ("nn_ratio", C.c_float), ("n_keys1", C.c_int32),
        ("n_keys2", C.c_int32), ("desc1", _pu8), ("desc2", _pu8), ("good_mp1", _pu8), ("good_mp2", _pu8), ("angle1", _pf), ("angle2", _pf),
        ("n_nodes1", C.c_int32), ("n_nodes2", C.c_int32), ("node_id1", _pu32), ("node_id2", _pu32), ("node_begin1", _pi), ("node_begin2", _pi),
        ("node_feat1", _pi), ("node_feat2", _pi),
    ]


class vba_search_bow_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_matches", C.c_int32), ("n_before_filter", C.c_int32), ("hist", C.c_int32 * 30), ("ind", C.c_int32 * 3),
                ("rounds", C.c_int32), ("match12", _pi), ("best_idx", _pi), ("best_dist", _pu16), ("best_dist2", _pu16), ("bin", _pu8), ("state", _pu8),
                ("match21", _pi)]


(SB_MATCHED, SB_NO_MAP_POINT, SB_NO_SHARED_NODE, SB_THRESHOLD, SB_RATIO, SB_ROTATION) = range(6)


@dataclass
class SearchBowProblem:
    """One ORBmatcher::SearchByBoW call as flat arrays: side 1 is the keyframe whose map points are carried over, side 2 the frame
    (mode SEARCH_BOW_KF_FRAME, src/ORBmatcher.cpp:207-350) or the second keyframe (SEARCH_BOW_KF_KF, :609-748); feature vectors in
    CSR form.  good_mp2 and the angles may stay None where the mode does not read them."""
    mode: int
    desc1: np.ndarray              # [n1,32] uint8
    desc2: np.ndarray              # [n2,32] uint8
    good_mp1: np.ndarray           # [n1] uint8
    node_id1: np.ndarray           # [nodes1] uint32, strictly ascending
    node_begin1: np.ndarray        # [nodes1 + 1] int32
    node_feat1: np.ndarray         # int32
    node_id2: np.ndarray
    node_begin2: np.ndarray
    node_feat2: np.ndarray
    good_mp2: np.ndarray = None    # [n2] uint8, KF_KF mode
    angle1: np.ndarray = None      # [n1] float32, with check_orientation
    angle2: np.ndarray = None      # [n2] float32
    th_low: int = 50
    nn_ratio: float = 0.75
    check_orientation: bool = True
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        u8 = lambda a, shape: np.ascontiguousarray(a, dtype=np.uint8).reshape(shape)
        opt = lambda a, f, *s: None if a is None else f(a, *s)
        f32 = lambda a, shape: np.ascontiguousarray(a, dtype=np.float32).reshape(shape)
        self.desc1 = u8(self.desc1, (-1, 32)); self.desc2 = u8(self.desc2, (-1, 32))
        self.good_mp1 = u8(self.good_mp1, (-1,)); self.good_mp2 = opt(self.good_mp2, u8, (-1,))
        self.angle1 = opt(self.angle1, f32, (-1,)); self.angle2 = opt(self.angle2, f32, (-1,))
        self.node_id1 = np.ascontiguousarray(self.node_id1, dtype=np.uint32).reshape(-1)
        self.node_id2 = np.ascontiguousarray(self.node_id2, dtype=np.uint32).reshape(-1)
        self.node_begin1 = _i32(self.node_begin1).reshape(-1); self.node_begin2 = _i32(self.node_begin2).reshape(-1)
        self.node_feat1 = _i32(self.node_feat1).reshape(-1); self.node_feat2 = _i32(self.node_feat2).reshape(-1)
        self.nn_ratio = float(np.float32(self.nn_ratio))

    n_keys1 = property(lambda self: self.desc1.shape[0])
    n_keys2 = property(lambda self: self.desc2.shape[0])
    n_nodes1 = property(lambda self: self.node_id1.shape[0])
    n_nodes2 = property(lambda self: self.node_id2.shape[0])
    kf_kf = property(lambda self: self.mode == SEARCH_BOW_KF_KF)

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        q.__post_init__()
        return q

    def as_struct(self) -> vba_search_bow_problem:
        s = vba_search_bow_problem()
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        s.mode, s.check_orientation, s.th_low, s.nn_ratio = int(self.mode), int(bool(self.check_orientation)), int(self.th_low), float(self.nn_ratio)
        s.n_keys1, s.n_keys2, s.n_nodes1, s.n_nodes2 = self.n_keys1, self.n_keys2, self.n_nodes1, self.n_nodes2
        s.desc1, s.desc2, s.good_mp1, s.good_mp2 = p(self.desc1, _pu8), p(self.desc2, _pu8), p(self.good_mp1, _pu8), p(self.good_mp2, _pu8)
        s.angle1, s.angle2 = p(self.angle1, _pf), p(self.angle2, _pf)
        s.node_id1, s.node_begin1, s.node_feat1 = p(self.node_id1, _pu32), p(self.node_begin1, _pi), p(self.node_feat1, _pi)
        s.node_id2, s.node_begin2, s.node_feat2 = p(self.node_id2, _pu32), p(self.node_begin2, _pi), p(self.node_feat2, _pi)
        return s


@dataclass
class SearchBowResult:
    status: int
    n_matches: int
    n_before_filter: int
    hist: np.ndarray                # [30]
    ind: np.ndarray                 # [3]
    rounds: int
    match12: np.ndarray             # [n1] int32
    best_idx: np.ndarray            # [n1] int32
    best_dist: np.ndarray           # [n1] uint16
    best_dist2: np.ndarray          # [n1] uint16
    bin: np.ndarray                 # [n1] uint8
    state: np.ndarray               # [n1] uint8
    match21: np.ndarray             # [n2] int32


class SearchBowResultBuf:
    """Caller-allocated result storage of one pair."""

    def __init__(self, p: SearchBowProblem):
        self.n, self.n2 = p.n_keys1, p.n_keys2
        m, m2 = max(self.n, 1), max(self.n2, 1)
        self.m12 = np.full(m, -7, dtype=np.int32)
        self.bi = np.full(m, -7, dtype=np.int32)
        self.bd = np.full(m, 7, dtype=np.uint16)
        self.bd2 = np.full(m, 7, dtype=np.uint16)
        self.bn = np.full(m, 77, dtype=np.uint8)
        self.st = np.full(m, 255, dtype=np.uint8)
        self.m21 = np.full(m2, -7, dtype=np.int32)
        s = self.s = vba_search_bow_result()
        s.status, s.n_matches, s.n_before_filter, s.rounds = -7, -7, -7, -7
        s.match12, s.best_idx, s.best_dist, s.best_dist2 = (self.m12.ctypes.data_as(_pi), self.bi.ctypes.data_as(_pi), self.bd.ctypes.data_as(_pu16),
                                                            self.bd2.ctypes.data_as(_pu16))
        s.bin, s.state, s.match21 = self.bn.ctypes.data_as(_pu8), self.st.ctypes.data_as(_pu8), self.m21.ctypes.data_as(_pi)

    def untouched(self):
        """nothing was written since construction"""
        s = self.s
        return ((s.status, s.n_matches, s.n_before_filter, s.rounds) == (-7, -7, -7, -7) and (self.m12 == -7).all() and (self.bi == -7).all() and
                (self.bd == 7).all() and (self.bd2 == 7).all() and (self.bn == 77).all() and (self.st == 255).all() and (self.m21 == -7).all() and
                not any(s.hist[:]) and not any(s.ind[:]))

    def get(self) -> SearchBowResult:
        s, n = self.s, self.n
        return SearchBowResult(s.status, s.n_matches, s.n_before_filter, np.array(s.hist[:]), np.array(s.ind[:]), s.rounds, self.m12[:n].copy(),
                               self.bi[:n].copy(), self.bd[:n].copy(), self.bd2[:n].copy(), self.bn[:n].copy(), self.st[:n].copy(),
                               self.m21[:self.n2].copy())


# ---- matching for the monocular initialisation (include/vislam_ba.h: vba_search_init_problem / vba_search_init_result) ----
SEARCH_INIT_MAX_KEYS = 16384


class vba_search_init_problem(C.Structure):
    _fields_ = [
        ("check_orientation", C.c_int32), ("th_low", C.c_int32), ("nn_ratio", C.c_float), ("window_size", C.c_double), ("n_keys1", C.c_int32),
        ("desc1", _pu8), ("oct1", _pu8), ("angle1", _pf), ("prev_matched", _pf), ("n_keys2", C.c_int32), ("desc2", _pu8), ("uv2", _pd),
        ("oct2", _pu8), ("angle2", _pf), ("bounds", C.c_double * 4), ("grid_cols", C.c_int32), ("grid_rows", C.c_int32),
        ("grid_inv_w", C.c_double), ("grid_inv_h", C.c_double), ("cell_begin", _pi), ("cell_feat", _pi),
    ]


class vba_search_init_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_matches", C.c_int32), ("n_before_filter", C.c_int32), ("n_stolen", C.c_int32), ("hist", C.c_int32 * 30),
                ("ind", C.c_int32 * 3), ("rounds", C.c_int32), ("match12", _pi), ("best_idx", _pi), ("best_dist", _pu16), ("best_dist2", _pu16),
                ("bin", _pu8), ("state", _pu8), ("prev_matched", _pf), ("match21", _pi), ("matched_dist", _pu16)]


(SI_MATCHED, SI_UPPER_LEVEL, SI_EMPTY_AREA, SI_THRESHOLD, SI_RATIO, SI_STOLEN, SI_ROTATION) = range(7)


@dataclass
class SearchInitProblem:
    """One ORBmatcher::SearchForInitialization call (src/ORBmatcher.cpp:477-595) as flat arrays: frame 1 with vbPrevMatched, frame 2
    with its grid in CSR form.  The angles may stay None without check_orientation."""
    desc1: np.ndarray              # [n1,32] uint8
    oct1: np.ndarray               # [n1] uint8
    prev_matched: np.ndarray       # [n1,2] float32
    desc2: np.ndarray              # [n2,32] uint8
    uv2: np.ndarray                # [n2,2]
    oct2: np.ndarray               # [n2] uint8
    bounds: np.ndarray             # [4] mnMinX mnMaxX mnMinY mnMaxY
    grid_cols: int
    grid_rows: int
    grid_inv_w: float
    grid_inv_h: float
    cell_begin: np.ndarray         # [cols * rows + 1] int32
    cell_feat: np.ndarray          # int32
    angle1: np.ndarray = None      # [n1] float32, with check_orientation
    angle2: np.ndarray = None      # [n2] float32
    window_size: float = 100.0
    th_low: int = 50
    nn_ratio: float = 0.9
    check_orientation: bool = True
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        u8 = lambda a, shape: np.ascontiguousarray(a, dtype=np.uint8).reshape(shape)
        opt = lambda a, f, *s: None if a is None else f(a, *s)
        f32 = lambda a, shape: np.ascontiguousarray(a, dtype=np.float32).reshape(shape)
        self.desc1 = u8(self.desc1, (-1, 32)); self.desc2 = u8(self.desc2, (-1, 32))
        self.oct1 = u8(self.oct1, (-1,)); self.oct2 = u8(self.oct2, (-1,))
        self.prev_matched = f32(self.prev_matched, (-1, 2)); self.uv2 = _f64(self.uv2, (-1, 2))
        self.angle1 = opt(self.angle1, f32, (-1,)); self.angle2 = opt(self.angle2, f32, (-1,))
        self.bounds = _f64(self.bounds, (4,))
        self.cell_begin = _i32(self.cell_begin).reshape(-1); self.cell_feat = _i32(self.cell_feat).reshape(-1)
        self.nn_ratio = float(np.float32(self.nn_ratio))

    n_keys1 = property(lambda self: self.desc1.shape[0])
    n_keys2 = property(lambda self: self.desc2.shape[0])
    n_q = property(lambda self: int((self.oct1 == 0).sum()))

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        q.__post_init__()
        return q

    def as_struct(self) -> vba_search_init_problem:
        s = vba_search_init_problem()
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        s.check_orientation, s.th_low, s.nn_ratio, s.window_size = int(bool(self.check_orientation)), int(self.th_low), float(self.nn_ratio), float(self.window_size)
        s.n_keys1, s.n_keys2 = self.n_keys1, self.n_keys2
        s.desc1, s.oct1, s.angle1, s.prev_matched = p(self.desc1, _pu8), p(self.oct1, _pu8), p(self.angle1, _pf), p(self.prev_matched, _pf)
        s.desc2, s.uv2, s.oct2, s.angle2 = p(self.desc2, _pu8), p(self.uv2, _pd), p(self.oct2, _pu8), p(self.angle2, _pf)
        s.bounds[:] = self.bounds.tolist()
        s.grid_cols, s.grid_rows, s.grid_inv_w, s.grid_inv_h = int(self.grid_cols), int(self.grid_rows), float(self.grid_inv_w), float(self.grid_inv_h)
        s.cell_begin, s.cell_feat = p(self.cell_begin, _pi), p(self.cell_feat, _pi)
        return s


@dataclass
class SearchInitResult:
    status: int
    n_matches: int
    n_before_filter: int
    n_stolen: int
    hist: np.ndarray                # [30]
    ind: np.ndarray                 # [3]
    rounds: int
    match12: np.ndarray             # [n1] int32
    best_idx: np.ndarray            # [n1] int32
    best_dist: np.ndarray           # [n1] uint16
    best_dist2: np.ndarray          # [n1] uint16
    bin: np.ndarray                 # [n1] uint8
    state: np.ndarray               # [n1] uint8
    prev_matched: np.ndarray        # [n1,2] float32
    match21: np.ndarray             # [n2] int32
    matched_dist: np.ndarray        # [n2] uint16


class SearchInitResultBuf:
    """Caller-allocated result storage of one pair."""

    def __init__(self, p: SearchInitProblem):
        self.n, self.n2 = p.n_keys1, p.n_keys2
        m, m2 = max(self.n, 1), max(self.n2, 1)
        self.m12 = np.full(m, -7, dtype=np.int32)
        self.bi = np.full(m, -7, dtype=np.int32)
        self.bd = np.full(m, 7, dtype=np.uint16)
        self.bd2 = np.full(m, 7, dtype=np.uint16)
        self.bn = np.full(m, 77, dtype=np.uint8)
        self.st = np.full(m, 255, dtype=np.uint8)
        self.pm = np.full((m, 2), -7.0, dtype=np.float32)
        self.m21 = np.full(m2, -7, dtype=np.int32)
        self.md = np.full(m2, 7, dtype=np.uint16)
        s = self.s = vba_search_init_result()
        s.status, s.n_matches, s.n_before_filter, s.n_stolen, s.rounds = -7, -7, -7, -7, -7
        s.match12, s.best_idx, s.best_dist, s.best_dist2 = (self.m12.ctypes.data_as(_pi), self.bi.ctypes.data_as(_pi), self.bd.ctypes.data_as(_pu16),
                                                            self.bd2.ctypes.data_as(_pu16))
        s.bin, s.state, s.prev_matched = self.bn.ctypes.data_as(_pu8), self.st.ctypes.data_as(_pu8), self.pm.ctypes.data_as(_pf)
        s.match21, s.matched_dist = self.m21.ctypes.data_as(_pi), self.md.ctypes.data_as(_pu16)

    def untouched(self):
        """nothing was written since construction"""
        s = self.s
        return ((s.status, s.n_matches, s.n_before_filter, s.n_stolen, s.rounds) == (-7, -7, -7, -7, -7) and (self.m12 == -7).all() and
                (self.bi == -7).all() and (self.bd == 7).all() and (self.bd2 == 7).all() and (self.bn == 77).all() and (self.st == 255).all() and
                (self.pm == -7.0).all() and (self.m21 == -7).all() and (self.md == 7).all() and not any(s.hist[:]) and not any(s.ind[:]))

    def get(self) -> SearchInitResult:
        s, n = self.s, self.n
        return SearchInitResult(s.status, s.n_matches, s.n_before_filter, s.n_stolen, np.array(s.hist[:]), np.array(s.ind[:]), s.rounds,
                                self.m12[:n].copy(), self.bi[:n].copy(), self.bd[:n].copy(), self.bd2[:n].copy(), self.bn[:n].copy(),
                                self.st[:n].copy(), self.pm[:n].copy(), self.m21[:self.n2].copy(), self.md[:self.n2].copy())


# ---- map-point refresh (include/vislam_ba.h: vba_mappoint_problem / vba_mappoint_result) ----
MAPPOINT_MAX_OBS = 1024
MAPPOINT_DESC, MAPPOINT_NORMAL = 1, 2


class vba_mappoint_problem(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("kf_center", _pd), ("kf_bad", _pu8), ("n_pt", C.c_int32), ("what", _pu8), ("pos", _pd), ("ref_kf", _pi),
                ("ref_scale", _pd), ("ref_top_scale", _pd), ("obs_begin", _pi), ("obs_kf", _pi), ("obs_desc", _pu8)]


class vba_mappoint_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_desc_done", C.c_int32), ("n_normal_done", C.c_int32), ("best_obs", _pi), ("best_median", _pi), ("n_desc", _pi),
                ("desc", _pu8), ("normal", _pd), ("dist_max", _pd), ("dist_min", _pd), ("desc_state", _pu8), ("normal_state", _pu8)]


(MP_DONE, MP_NOT_ASKED, MP_NO_OBSERVATIONS, MP_NO_INPUT) = range(4)   # MP_NO_INPUT: no good keyframe / the point in an observer's centre


@dataclass
class MapPointProblem:
    """One list of map points over one table of keyframes, for MapPoint::ComputeDistinctiveDescriptors and
    MapPoint::UpdateNormalAndDepth (src/MapPoint.cpp:336-413, :450-501): the observations in CSR form, in the order of mObservations.
    obs_desc may stay None when no point asks for the descriptor part; pos, ref_kf and the scales when none asks for the normal part."""
    kf_center: np.ndarray          # [n_kf,3]
    kf_bad: np.ndarray             # [n_kf] uint8
    what: np.ndarray               # [n_pt] uint8: MAPPOINT_DESC | MAPPOINT_NORMAL
    obs_begin: np.ndarray          # [n_pt + 1] int32
    obs_kf: np.ndarray             # [n_obs] int32
    obs_desc: np.ndarray = None    # [n_obs,32] uint8
    pos: np.ndarray = None         # [n_pt,3]
    ref_kf: np.ndarray = None      # [n_pt] int32
    ref_scale: np.ndarray = None   # [n_pt]
    ref_top_scale: np.ndarray = None   # [n_pt]
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        u8 = lambda a, *shape: np.ascontiguousarray(a, dtype=np.uint8).reshape(shape)
        opt = lambda a, f, *s: None if a is None else f(a, *s)
        self.kf_center = _f64(self.kf_center, (-1, 3)); self.kf_bad = u8(self.kf_bad, -1)
        self.what = u8(self.what, -1)
        self.obs_begin = _i32(self.obs_begin).reshape(-1); self.obs_kf = _i32(self.obs_kf).reshape(-1)
        self.obs_desc = opt(self.obs_desc, u8, -1, 32)
        self.pos = opt(self.pos, _f64, (-1, 3)); self.ref_kf = opt(self.ref_kf, lambda a: _i32(a).reshape(-1))
        self.ref_scale = opt(self.ref_scale, _f64, (-1,)); self.ref_top_scale = opt(self.ref_top_scale, _f64, (-1,))

    n_kf = property(lambda self: self.kf_center.shape[0])
    n_pt = property(lambda self: self.what.shape[0])
    n_obs = property(lambda self: self.obs_kf.shape[0])

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        q.__post_init__()
        return q

    def as_struct(self) -> vba_mappoint_problem:
        s = vba_mappoint_problem()
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        s.n_kf, s.n_pt = self.n_kf, self.n_pt
        s.kf_center, s.kf_bad, s.what = p(self.kf_center, _pd), p(self.kf_bad, _pu8), p(self.what, _pu8)
        s.pos, s.ref_kf, s.ref_scale, s.ref_top_scale = p(self.pos, _pd), p(self.ref_kf, _pi), p(self.ref_scale, _pd), p(self.ref_top_scale, _pd)
        s.obs_begin, s.obs_kf, s.obs_desc = p(self.obs_begin, _pi), p(self.obs_kf, _pi), p(self.obs_desc, _pu8)
        return s


@dataclass
class MapPointResult:
    status: int
    n_desc_done: int
    n_normal_done: int
    best_obs: np.ndarray            # [n_pt] int32
    best_median: np.ndarray         # [n_pt] int32
    n_desc: np.ndarray              # [n_pt] int32
    desc: np.ndarray                # [n_pt,32] uint8
    normal: np.ndarray              # [n_pt,3]
    dist_max: np.ndarray            # [n_pt]
    dist_min: np.ndarray            # [n_pt]
    desc_state: np.ndarray          # [n_pt] uint8
    normal_state: np.ndarray        # [n_pt] uint8


class MapPointResultBuf:
    """Caller-allocated result storage of one problem."""

    def __init__(self, p: MapPointProblem):
        self.n = p.n_pt
        m = max(self.n, 1)
        self.bo = np.full(m, -7, dtype=np.int32)
        self.bm = np.full(m, -7, dtype=np.int32)
        self.nd = np.full(m, -7, dtype=np.int32)
        self.de = np.full((m, 32), 77, dtype=np.uint8)
        self.no = np.full((m, 3), -7.0)
        self.dx = np.full(m, -7.0)
        self.dn = np.full(m, -7.0)
        self.ds = np.full(m, 255, dtype=np.uint8)
        self.ns = np.full(m, 255, dtype=np.uint8)
        s = self.s = vba_mappoint_result()
        s.status, s.n_desc_done, s.n_normal_done = -7, -7, -7
        s.best_obs, s.best_median, s.n_desc, s.desc = self.bo.ctypes.data_as(_pi), self.bm.ctypes.data_as(_pi), self.nd.ctypes.data_as(_pi), self.de.ctypes.data_as(_pu8)
        s.normal, s.dist_max, s.dist_min = self.no.ctypes.data_as(_pd), self.dx.ctypes.data_as(_pd), self.dn.ctypes.data_as(_pd)
        s.desc_state, s.normal_state = self.ds.ctypes.data_as(_pu8), self.ns.ctypes.data_as(_pu8)

    def untouched(self):
        """nothing was written since construction"""
        s = self.s
        return ((s.status, s.n_desc_done, s.n_normal_done) == (-7, -7, -7) and (self.bo == -7).all() and (self.bm == -7).all() and (self.nd == -7).all() and
                (self.de == 77).all() and (self.no == -7.0).all() and (self.dx == -7.0).all() and (self.dn == -7.0).all() and (self.ds == 255).all() and
                (self.ns == 255).all())

    def get(self) -> MapPointResult:
        s, n = self.s, self.n
        return MapPointResult(s.status, s.n_desc_done, s.n_normal_done, self.bo[:n].copy(), self.bm[:n].copy(), self.nd[:n].copy(), self.de[:n].copy(),
                              self.no[:n].copy(), self.dx[:n].copy(), self.dn[:n].copy(), self.ds[:n].copy(), self.ns[:n].copy())


# ---- essential-graph optimisation (include/vislam_ba.h: vba_posegraph_problem / vba_posegraph_result) ----
class vba_posegraph_problem(C.Structure):
    _fields_ = [
        ("n_vertices", C.c_int32), ("n_edges", C.c_int32), ("fix_scale", C.c_int32), ("its", C.c_int32),
        ("lambda_init", C.c_double), ("S", _pd), ("fixed", _pu8), ("edge_i", _pi), ("edge_j", _pi), ("edge_S", _pd),
        ("n_pt", C.c_int32), ("pt", _pd), ("pt_ref", _pi),
    ]


class vba_posegraph_result(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("its_done", C.c_int32), ("lm_trials", C.c_int32), ("stop", C.c_int32),
        ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_final", C.c_double),
    ]


@dataclass
class PoseGraphProblem:
    """One Optimizer::OptimizeEssentialGraph call (src/Optimizer.cpp:4243-4552) as flat arrays: the Sim3 vertices, the EdgeSim3
    edges its four pair rules chose, and the map points with their reference vertices."""
    S: np.ndarray                  # [n,8] Siw as t(3) q(4, xyzw) s
    fixed: np.ndarray              # [n] uint8
    edge_i: np.ndarray             # [m] vertex 0
    edge_j: np.ndarray             # [m] vertex 1
    edge_S: np.ndarray             # [m,8] measurement Sji
    fix_scale: int = 0
    its: int = 20
    lambda_init: float = 1e-16
    pt: Optional[np.ndarray] = None      # [k,3]
    pt_ref: Optional[np.ndarray] = None  # [k]
    truth: dict = field(default_factory=dict)

    def __post_init__(self):
        self.S = _f64(self.S, (-1, 8))
        self.fixed = np.ascontiguousarray(self.fixed, dtype=np.uint8).reshape(-1)
        self.edge_i = _i32(self.edge_i).reshape(-1)
        self.edge_j = _i32(self.edge_j).reshape(-1)
        self.edge_S = _f64(self.edge_S, (-1, 8))
        self.pt = _f64(self.pt if self.pt is not None else np.zeros((0, 3)), (-1, 3))
        self.pt_ref = _i32(self.pt_ref if self.pt_ref is not None else []).reshape(-1)

    n_vertices = property(lambda self: self.S.shape[0])
    n_edges = property(lambda self: self.edge_i.shape[0])
    n_pt = property(lambda self: self.pt.shape[0])

    def copy(self, **changes):
        import copy as _c
        q = _c.copy(self)
        q.S = self.S.copy()
        q.pt = self.pt.copy()
        for k, v in changes.items():
            setattr(q, k, v)
        return q

    def as_struct(self) -> vba_posegraph_problem:
        s = vba_posegraph_problem()
        s.n_vertices, s.n_edges, s.fix_scale, s.its = self.n_vertices, self.n_edges, int(self.fix_scale), int(self.its)
        s.lambda_init = self.lambda_init
        s.S, s.fixed = self.S.ctypes.data_as(_pd), self.fixed.ctypes.data_as(_pu8)
        s.edge_i, s.edge_j, s.edge_S = self.edge_i.ctypes.data_as(_pi), self.edge_j.ctypes.data_as(_pi), self.edge_S.ctypes.data_as(_pd)
        s.n_pt = self.n_pt
        s.pt, s.pt_ref = self.pt.ctypes.data_as(_pd), self.pt_ref.ctypes.data_as(_pi)
        return s


@dataclass
class PoseGraphResult:
    status: int
    its_done: int
    lm_trials: int
    stop: int
    chi2_initial: float
    chi2_final: float
    lambda_final: float
    S: np.ndarray                  # [n,8] the optimised estimates
    pt: np.ndarray                 # [k,3] the corrected map points
