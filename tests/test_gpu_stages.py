"""Stage-level checks of one solve iteration of the HIP backend against the extended-precision reference of tests/stage_ref.py.

vba_debug_capture copies, at one chosen enqueue_solve_iteration of a run, the state before the iteration, the Schur-reduced system S
and r, the LDL^T factor with y (L y = r) and x_c, and the state after the update.  Every case checks
  * S (lower triangle, every tile the factor reads) and r against the reference, within c eps (k + kappa) sqrt(h_i h_j);
  * L D L^T against the reference S on the whole lower triangle (a sub-block skipped by the Schur kernels shows here), against the
    captured S (backward error of the factor kernels alone), and D > 0;
  * L y = r and D L^T x_c = y; x_c against the reference solve; the state after the update against state (+) Delta x;
  * that the intended kernel path ran (layout hook: order, chain columns, packed factor, Schur / factor / solve kernels).
Every case prints the worst error of each stage in units of its bound, the path taken and the sensitivity margin of its bounds."""
import ctypes as C

import numpy as np
import pytest

import stage_ref as sr
from mc_slam_amd import abi, synth, backend

pytestmark = pytest.mark.gpu

# capture items (vba_host_run.h, CAP_*)
POSE_A, VEL_A, BIAS_A, PT_A, CTRL_A, LVL_A, VARACT_A, S_B, VEC_B, LF_C, YV_C, VEC_C, POSE_D, VEL_D, BIAS_D, PT_D = range(16)
SCHUR = {0: "k_schur_all_w", 1: "k_schur_all", 2: "k_schur_diag+k_schur_off_w", 3: "k_schur_diag+k_schur_off",
         4: "k_dinv+k_schur_diag3+k_schur_off3_w", 5: "k_dinv+k_schur_diag3+k_schur_off3"}
FACTOR = {1: "k_chol_step", 4: "k_chol_step4<false>", 5: "k_chol_step4<true>", 6: "k_chol_diag_ll2+k_chol_panel_ll", 7: "pcg",
          8: "mixed step kernels"}
TRSV = {0: "k_trsv_p", 1: "k_trsv"}


class Capture:
    """one vba_batch_run with a capture of iteration `call`, on a fresh handle of the hooks flavour"""

    def __init__(self, probs, call, setup=(), path=(), env=None):
        self.ba = backend.LocalBA(0, hooks=True)
        lib = self.lib = self.ba.lib
        h = self.ba.h
        lib.vba_debug_set_path.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
        lib.vba_debug_capture_get.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64]
        lib.vba_debug_window_layout.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64]
        lib.vba_debug_factor_dense.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int64]
        assert lib.vba_debug_set_streams(h, 1) == 0
        for name, val in setup:
            assert getattr(lib, "vba_debug_" + name)(h, val) == 0
        for name, val in path:
            assert lib.vba_debug_set_path(h, name.encode(), val) == 0
        self.ba.upload(probs)
        assert lib.vba_debug_capture(h, call) == 0
        self.ba.run()
        self.probs = probs

    def close(self):
        self.ba.close()

    def layout(self, w):
        p = self.probs[w]
        pdim, _ = sr.dims(p)
        n = 20 + pdim * p.n_kf_free + 6
        out = np.zeros(n, np.int64)
        assert self.lib.vba_debug_window_layout(self.ba.h, w, out.ctypes.data_as(C.POINTER(C.c_int64)), n - 1) == -1   # bounds
        assert self.lib.vba_debug_window_layout(self.ba.h, w, out.ctypes.data_as(C.POINTER(C.c_int64)), n) == 0
        k = 20 + pdim * p.n_kf_free
        return dict(nS=int(out[0]), nb=int(out[1]), pdim=int(out[2]), n_free=int(out[3]), order=int(out[4]), nc=int(out[5]),
                    nc_split=int(out[6]), l_packed=int(out[7]), regime_n=int(out[8]), schur=int(out[10]), factor=int(out[11]),
                    trsv=int(out[12]), ctrl_bytes=int(out[13]), pcg=int(out[14]), pcg_tri=int(out[15]),
                    ctrl_off=dict(stage=int(out[16]), active=int(out[17]), robust_vis=int(out[18]), lam=int(out[19])),
                    vpos=out[20:k].copy(), pad0=out[k:k + 3].tolist(), padn=out[k + 3:k + 6].tolist())

    def get(self, what, w, dtype, count):
        a = np.zeros(count, dtype)
        rc = self.lib.vba_debug_capture_get(self.ba.h, what, w, a.ctypes.data, a.nbytes)
        assert rc == 0, self.lib.vba_last_error(self.ba.h)
        return a

    def factor(self, w, nS):
        F = np.zeros((nS, nS))
        assert self.lib.vba_debug_factor_dense(self.ba.h, w, F.ctypes.data_as(C.POINTER(C.c_double)), nS * nS - 1) == -1
        assert self.lib.vba_debug_factor_dense(self.ba.h, w, F.ctypes.data_as(C.POINTER(C.c_double)), nS * nS) == 0
        return F


def _ctrl(raw, off):
    """the WinCtrl fields the checks read, at the offsets the layout hook reports"""
    i32 = lambda o: int(np.frombuffer(raw[o:o + 4].tobytes(), np.int32)[0])
    return dict(stage=i32(off["stage"]), active=i32(off["active"]), robust_vis=i32(off["robust_vis"]),
                lam=float(np.frombuffer(raw[off["lam"]:off["lam"] + 8].tobytes(), np.float64)[0]))


def _sensitivity(p, red, lvl, robust, tS, n_edges=4):
    """smallest max|dS| / bound tS (oracle order) over a few edges dropped or doubled (float64: the changes are ~1e-3 of S)"""
    base = red["S"].astype(np.float64)
    fix = np.zeros(p.n_kf, np.uint8) if p.kf_fix is None else p.kf_fix
    cand = np.flatnonzero((lvl == 0) & (p.obs_kf < p.n_kf_free) & ((fix[p.obs_kf] & 1) == 0))
    out = []
    for o in np.random.default_rng(3).choice(cand, min(n_edges, cand.size), replace=False):
        for how in ("drop", "double"):
            q, lv = p.copy(), lvl.copy()
            if how == "drop":
                lv[o] = 1
            else:
                q.obs_w[o] *= 2
            H2, b2, c2, _ = sr.linearize(q, robust, lv)
            out.append((np.abs(sr.reduced(q, H2, b2, c2, lv, red["lam"], dtype=np.float64)["S"] - base) / tS).max())
    return min(out)


def check_window(cap, w, expect, stage=None, dtype=sr.LD, need_excluded=False):
    p = cap.probs[w]
    lay = cap.layout(w)
    nS, pdim, nf = lay["nS"], lay["pdim"], p.n_kf_free
    for key, val in expect.items():
        assert lay[key] == val if not callable(val) else val(lay[key]), (key, lay[key], val)
    ctrl = _ctrl(cap.get(CTRL_A, w, np.uint8, lay["ctrl_bytes"]), lay["ctrl_off"])
    assert ctrl["active"] == 1, ctrl
    if stage is not None:
        assert ctrl["stage"] == stage, ctrl
    # the state the iteration linearised at, and the reference built there
    q = p.copy()
    q.kf_pose[...] = cap.get(POSE_A, w, np.float64, 7 * p.n_kf).reshape(-1, 7)
    q.kf_vel = cap.get(VEL_A, w, np.float64, 3 * p.n_kf).reshape(-1, 3)
    q.kf_bias = cap.get(BIAS_A, w, np.float64, 12 * p.n_kf).reshape(-1, 12)
    q.pt[...] = cap.get(PT_A, w, np.float64, 3 * p.n_pt).reshape(-1, 3)
    lvl = cap.get(LVL_A, w, np.uint8, p.n_obs)
    robust = bool(ctrl["robust_vis"])
    beg = np.asarray(p.pt_obs_begin)
    excluded = int(np.logical_and.reduceat(lvl != 0, beg[:-1]).sum()) if p.n_obs else 0   # landmarks with every edge at level 1
    if need_excluded:
        assert excluded > 0 and not robust, (excluded, robust)
    H, b, chi2, lvl = sr.linearize(q, robust, lvl)
    _, L = sr.dims(p)
    var_act, pt_act = sr.active_sets(q, lvl)
    lam = 0.0
    if p.algo == abi.ALGO_LM:
        lam = sr.lambda_init(H, var_act, pt_act, pdim * nf, L)
        assert abs(ctrl["lam"] - lam) <= 1e-12 * lam, (ctrl["lam"], lam)   # computeLambdaInit
    red = sr.reduced(q, H, b, chi2, lvl, lam, dtype=dtype)
    rows, pads = sr.window_rows(lay)
    va = cap.get(VARACT_A, w, np.int32, nS)
    assert np.array_equal(va[rows] != 0, var_act) and not va[pads].any()
    Sref = sr.to_window(red["S"].astype(np.float64), lay)
    rref = sr.to_window(red["r"].astype(np.float64), lay)
    tS = sr.to_window(sr.tol_S(red), lay, pad_value=0.0)
    tr = sr.to_window(sr.tol_r(red), lay)
    low = np.tril(np.ones((nS, nS), bool))
    S = cap.get(S_B, w, np.float64, nS * nS).reshape(nS, nS)
    r = cap.get(VEC_B, w, np.float64, nS)
    res = dict(r=sr.ratio(r - rref, tr))
    path = "order %d nc %d split %d packed %d | %s | %s | %s" % (lay["order"], lay["nc"], lay["nc_split"], lay["l_packed"],
                                                           SCHUR.get(lay["schur"]), FACTOR.get(lay["factor"]), TRSV.get(lay["trsv"]))
    # S and r first, before anything of the factor is looked at: a failure further down then says whether S was already wrong, and
    # in which keyframe blocks (the whole lower triangle here; the asserted figure below counts the tiles the factor reads)
    where = sr.format_blocks(sr.worst_blocks(np.where(low, S - Sref, 0), tS, lay, var_act))
    print("\n  window %d before the factor: r %.3g, S (lower triangle) %.3g of its bound; %s"
          % (w, res["r"], sr.ratio(np.where(low, S - Sref, 0), tS), where))
    if lay["pcg"]:
        # PCG stops at sqrt(r'M^-1 r / r0'M^-1 r0) <= 1e-10 (x0 = 0, r0 = the rhs), M the block-Jacobi or the block-tridiagonal
        # (keyframe chain) part of S.  x_c is held to that rule with M built from the captured S, plus the drift between the recurred
        # and the true residual (c nS eps (|S| |x| + |r|))
        Ssym = np.tril(S) + np.tril(S, -1).T
        res["S"] = sr.ratio(np.where(low, S - Sref, 0), tS)
        x = cap.get(VEC_C, w, np.float64, nS)
        So, ro, xo = Ssym[np.ix_(rows, rows)], r[rows], x[rows]
        M = np.zeros_like(So)
        for a in range(nf):
            for b in ((a - 1, a, a + 1) if lay["pcg_tri"] else (a,)):
                if 0 <= b < nf:
                    M[pdim * a:pdim * a + pdim, pdim * b:pdim * b + pdim] = So[pdim * a:pdim * a + pdim, pdim * b:pdim * b + pdim]
        mnorm = lambda v: np.sqrt(v @ np.linalg.solve(M, v))
        drift = 8 * nS * sr.EPS * (np.abs(So) @ np.abs(xo) + np.abs(ro))
        res["pcg_stop"] = mnorm(ro - So @ xo) / (1e-10 * mnorm(ro) + mnorm(drift))
        tF = np.zeros((nS, nS))
        path = "pcg %s | %s" % ("tridiagonal" if lay["pcg_tri"] else "block-Jacobi", SCHUR.get(lay["schur"]))
    else:
        F = cap.factor(w, nS)
        Lm, d = sr.factor_parts(F)
        # tiles the factor reads: everything when S stays pristine (left-looking), else the tiles of the factor's lists
        nb = lay["nb"]
        tile_on = np.abs(F).reshape(nb, 32, nb, 32).max(axis=(1, 3)) > 0
        read = np.kron(tile_on | np.eye(nb, dtype=bool), np.ones((32, 32), bool)) if not lay["l_packed"] else np.ones((nS, nS), bool)
        read &= low
        res["S"] = sr.ratio(np.where(read, S - Sref, 0), tS)
        where = sr.format_blocks(sr.worst_blocks(np.where(read, S - Sref, 0), tS, lay, var_act))
        assert (d > 0).all(), ("pivot", d.min(), "S", res["S"], "r", res["r"], where)
        tF = sr.ldlt_tol(Lm, d)
        LDL = (Lm * d) @ Lm.T
        res["LDL_vs_ref"] = sr.ratio(np.where(low, LDL - Sref, 0), tS + tF)
        res["LDL_vs_S"] = sr.ratio(np.where(read, LDL - S, 0), tF)
        y = cap.get(YV_C, w, np.float64, nS)
        x = cap.get(VEC_C, w, np.float64, nS)
        ty, tx = sr.solve_tols(Lm, d, y, x)
        res["Ly"] = sr.ratio(r - Lm @ y, ty)
        res["DLx"] = sr.ratio(y - d * (Lm.T @ x), tx)
        E = (tS + tF)[np.ix_(rows, rows)]
        f = (tr + ty + np.abs(Lm) @ tx)[rows]
        xg = x[rows]
        bound, ds, _ = sr.xc_bound(red["S"].astype(np.float64), E, f, xg)
        res["x_c"] = np.linalg.norm(ds * (xg - sr.solve_c(red))) / bound
    assert not x[pads].any()
    # the update: state before (+) [x_c, landmark back-substitution of x_c]
    xg = x[rows]
    dx = sr.full_step(red, xg)
    pose, vel, bias, pt = sr.apply_step(q, (q.kf_pose, q.kf_vel, q.kf_bias, q.pt), dx, var_act, pt_act)
    poseD = cap.get(POSE_D, w, np.float64, 7 * p.n_kf).reshape(-1, 7)
    velD = cap.get(VEL_D, w, np.float64, 3 * p.n_kf).reshape(-1, 3)
    biasD = cap.get(BIAS_D, w, np.float64, 12 * p.n_kf).reshape(-1, 12)
    ptD = cap.get(PT_D, w, np.float64, 3 * p.n_pt).reshape(-1, 3)
    e8 = 8 * sr.EPS
    res["pose"] = sr.ratio(poseD - pose, e8 * (np.abs(pose) + np.abs(q.kf_pose) + 1.0))
    res["vel_bias"] = max(sr.ratio(velD - vel, e8 * (np.abs(vel) + np.abs(q.kf_vel))),
                          sr.ratio(biasD - bias, e8 * (np.abs(bias) + np.abs(q.kf_bias))))
    tl = np.zeros((p.n_pt, 3))
    tl[pt_act, :L] = sr.landmark_step_tol(red, xg, robust_vis=robust)
    tl = tl + e8 * (np.abs(pt) + np.abs(q.pt))
    res["landmarks"] = sr.ratio(ptD - pt, tl)
    if p.n_pt:   # the worst landmark, by name: its active edges, its step and what the update kernel left
        lq = np.array([sr.ratio(ptD[i] - pt[i], tl[i]) for i in range(p.n_pt)])
        i = int(lq.argmax())
        print("  worst landmark %d: %.3g x bound, active %d, edges %d of which at level 0 %d, before %s reference %s gpu %s"
              % (i, lq[i], pt_act[i], beg[i + 1] - beg[i], int((lvl[beg[i]:beg[i + 1]] == 0).sum()), q.pt[i, :L], pt[i, :L], ptD[i, :L]))
    # the bounds must stay far below what one edge does to S: the S bound alone, and S + factor (the bound of LDL_vs_ref)
    margin = _sensitivity(q, red, lvl, robust, (tS + tF)[np.ix_(rows, rows)], n_edges=4 if p.n_obs < 10000 else 1)
    print("\n  window %d (nS %d, k %d, kappa %.3g, landmarks without an active edge %d): %s\n  error / bound: %s\n  sensitivity margin of the S + factor bound: %.2e"
          % (w, nS, red["k"], red["kappa"], excluded, path, " ".join("%s %.3g" % kv for kv in res.items()), margin))
    for key, v in res.items():
        assert v <= 1.0, (key, v, res, where)
    assert margin >= 1e6
    return lay, res


def _idp(**kw):
    base = dict(n_kf=12, n_fixed=2, n_pt=400, n_obs=2000, seed=51)
    base.update(kw)
    return synth.make_window(abi.VARIANT_PRV_IDP, **base)


def _xyz(variant, **kw):
    base = dict(n_kf=12, n_fixed=2, n_pt=400, n_obs=2000, seed=52)
    base.update(kw)
    return synth.make_window(variant, algo=abi.ALGO_LM, **base)


def _run(probs, w, call, expect, setup=(), path=(), stage=None, dtype=sr.LD, need_excluded=False):
    cap = Capture(probs, call, setup, path)
    try:
        return check_window(cap, w, expect, stage, dtype, need_excluded)
    finally:
        cap.close()


# ---- one window: the _w Schur kernels, k_chol_step4<true>, k_trsv_p, the two-sided order -------------------------------------------
def test_idp_one_window_default_path():
    _run([_idp()], 0, 0, dict(schur=0, factor=5, trsv=0, l_packed=0))


def test_idp_one_window_split_schur_and_old_trsv():
    _run([_idp(seed=53)], 0, 1, dict(schur=2, factor=5, trsv=1), path=[("schur_split", 1), ("trsv_old", 1)])


def test_idp_first_form_of_the_step_without_chain():
    _run([_idp(seed=54)], 0, 0, dict(factor=1, nc=0), setup=[("set_chol_step", 1), ("set_chain", 0)])


def test_idp_one_free_keyframe():   # nS < 32: a single tile, mostly pad
    _run([_idp(n_kf=4, n_fixed=3, n_pt=150, n_obs=300, seed=55)], 0, 0, dict(n_free=1, nS=32))


def test_idp_stage_two_with_levels():
    """stage 2: robust kernel off, the outliers of stage 1 at level 1, landmarks whose every edge is excluded (one to three edges
    per landmark, three-pixel noise); capture call = its_stage1: stage 1 runs all its iterations.

    This case was an open finding: the landmark step at 4.8 times its bound (landmark 181: one active edge).  The bound was at fault,
    not k_update: it counted the accumulation error of the back-substitution for exact W, Dinv and b_l, and the float64 REFERENCE
    with its inputs perturbed by one unit roundoff leaves that bound by a factor of 16 to 31 at the same landmarks (14 at landmark
    181) -- J_rho cancels at low parallax, and one or two edges per landmark average nothing out.  stage_ref.landmark_step_tol now
    carries the forward error of J_rho and of the residual through Dinv (tests/test_stage_ref.py::
    test_perturbed_reference_stays_inside_the_landmark_bound); the levels and the state of this capture are those of the CPU
    oracle's stage 1."""
    p = _idp(seed=56, pix_noise=3.0, n_obs=800)
    p.its_stage1 = 2
    _run([p], 0, 2, dict(), stage=1, need_excluded=True)


def test_idp_keyframe_order():   # sparse tracks of consecutive keyframes: the keyframe-by-keyframe order (1) wins
    _run([_idp(n_kf=20, n_pt=600, n_obs=1200, seed=57)], 0, 0, dict(order=1))


def test_idp_one_chain_orders(monkeypatch):
    monkeypatch.setenv("VBA_ONE_CHAIN", "1")   # read per upload: orders 0 and 1 only
    _run([_idp(n_kf=20, n_pt=800, n_obs=4000, seed=57, tracks="random")], 0, 0, dict(order=0, nc=lambda v: v > 0, nc_split=0))
    _run([_idp(n_kf=20, n_pt=600, n_obs=1200, seed=57)], 0, 0, dict(order=1))


def test_idp_more_than_64_keyframes():   # two-word landmark masks; the reference in float64, with the same bounds
    p = _idp(n_kf=70, n_fixed=1, n_pt=2100, n_obs=8400, seed=90)
    _run([p], 0, 0, dict(n_free=69), dtype=np.float64)


def test_idp_rows_32m_plus_1():   # 15 free keyframes: 225 = 7 * 32 + 1 rows of variables
    p = _idp(n_kf=17, n_pt=500, n_obs=2500, seed=91)
    _run([p], 0, 0, dict(n_free=15, pdim=15))


def test_se3_xyz_pad_free():   # 16 free keyframes x 6 = 96 rows: no pad row at all
    _run([_xyz(abi.VARIANT_SE3_XYZ, n_kf=18, n_pt=500, n_obs=2500, seed=92)], 0, 0, dict(nS=96, padn=[0, 0, 0]))


def test_idp_fixed_observer_inside_tracks_caller_order():
    """a keyframe in the middle of the window with its PR vertex fixed (its edges still count for the landmarks, not for S) and its
    velocity fixed on another one; landmarks in the caller's order (grouped by first keyframe, as the reference lists them).

    This case was an open finding (a pivot of -8e10): the PR x PR blocks (a, 4) of the keyframes a that observe a landmark anchored
    in keyframe 4 were 1e14 bounds off, next to the identity block of keyframe 4 -- the reference items of the off-diagonal pairs
    formed Bi^T Br from the observer's edge record whatever the reference keyframe's flag.  Such items are no longer listed
    (csrc/vba_structure.h); every other pattern: tests/test_gpu_kf_fix.py."""
    p = _idp(seed=93, landmark_order="caller")
    fix = np.zeros(p.n_kf, np.uint8)
    fix[4] = 1
    fix[7] = 2
    p.kf_fix = fix
    _run([p], 0, 0, dict())


# ---- batches: k_schur_all / k_schur_off3, k_chol_step4<false> with chain rows, the window under test second in a ragged batch ----
def test_idp_batch_of_eight_ragged():
    probs = [_idp(n_kf=8 + 2 * i, n_pt=300 + 20 * i, n_obs=1500 + 100 * i, seed=60 + i) for i in range(8)]
    for w in (1, 6):
        _run(probs, w, 0, dict(schur=1, factor=4, regime_n=8, trsv=0))


def test_idp_left_looking_packed():
    """left-looking kernels with chain columns (k_chol_chain_diag / k_chol_chain_panel, then k_chol_diag_ll2 / k_chol_panel_ll)"""
    probs = [_idp(seed=70), _idp(n_kf=20, n_pt=700, n_obs=3500, seed=71)]
    _run(probs, 1, 0, dict(l_packed=1, factor=6, trsv=1, nc=lambda v: v > 0), setup=[("set_ll_min", 1)])


def test_idp_full_size_window():   # two-sided order, chain rows side by side; the reference in float64, with the same bounds
    _run([synth.config_c3(seed=7)], 0, 0, dict(schur=0, factor=5, l_packed=0, order=2, nc=lambda v: v > 0, nc_split=lambda v: v > 0),
         dtype=np.float64)


# ---- XYZ landmarks with Levenberg-Marquardt ------------------------------------------------------------------------------------
def test_prv_xyz_lm_one_window():
    _run([_xyz(abi.VARIANT_PRV_XYZ, n_fixed=1)], 0, 0, dict(schur=4, factor=5))


def test_se3_xyz_lm_one_window():
    _run([_xyz(abi.VARIANT_SE3_XYZ)], 0, 0, dict(schur=4, factor=5, pdim=6))


def test_se3_xyz_lm_batch_of_eight():
    probs = [_xyz(abi.VARIANT_SE3_XYZ, n_kf=8 + i, seed=80 + i) for i in range(8)]
    _run(probs, 1, 0, dict(schur=5, factor=4))


# ---- PCG: x_c against the dense solve of the captured S --------------------------------------------------------------------------
@pytest.mark.parametrize("jacobi", [0, 1])
def test_pcg_preconditioners(jacobi):
    p = _idp(seed=90)
    p.solver = abi.SOLVER_PCG
    _run([p], 0, 0, dict(pcg=1, pcg_tri=1 - jacobi, factor=7), path=[("pcg_jacobi", jacobi)])


# ---- the plan of a batch (csrc/vba_host_plan.h): what vba_debug_plan reports, what the launch sites recorded, what came out --------
import plan_cases as pc


def _tiny(i):
    return _idp(n_kf=6, n_fixed=1, n_pt=60, n_obs=300, seed=200 + i)


@pytest.fixture(scope="module")
def tiny_alone():
    """64 tiny windows, each solved in a call of its own on one fresh handle: the reference of every batch below (left unchanged)"""
    ba = backend.LocalBA(0)
    try:
        return [ba.solve(_tiny(i)) for i in range(64)]
    finally:
        ba.close()


def _plan(cap):
    out = np.zeros(len(pc.FIELDS), np.int64)
    cap.lib.vba_debug_plan.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64]
    assert cap.lib.vba_debug_plan(cap.ba.h, out.ctypes.data_as(C.POINTER(C.c_int64)), len(out) - 1) == -1   # bounds
    assert cap.lib.vba_debug_plan(cap.ba.h, out.ctypes.data_as(C.POINTER(C.c_int64)), len(out)) == 0
    return out.tolist()


@pytest.mark.parametrize("n,ll_min", [(1, 0), (7, 0), (8, 0), (64, 0), (8, 8)])
def test_plan_of_a_batch_and_what_it_launched(tiny_alone, n, ll_min):
    probs = [_tiny(i) for i in range(n)]
    cap = Capture(probs, 0, setup=[("set_ll_min", ll_min)] if ll_min else [])
    try:
        want = dict(zip(pc.FIELDS, pc.expected(n, ll_min=ll_min or 256)))
        want["ngroups"] = 1                                     # vba_debug_set_streams(h, 1)
        got = dict(zip(pc.FIELDS, _plan(cap)))
        print("plan of %d windows: %s" % (n, got))
        assert got == want
        lay = cap.layout(n - 1)
        assert (lay["schur"], lay["factor"], lay["trsv"]) == (got["schur"], got["factor"], got["trsv"])   # planned == launched
        assert (lay["regime_n"], lay["l_packed"], lay["pcg_tri"]) == (n, got["left_looking"], got["pcg_tri"])
        qs, rs = cap.ba.download()
    finally:
        cap.close()
    exact = n < 8 and not ll_min                                # the regime of a window solved alone
    for (q0, r0), q, r in zip(tiny_alone, qs, rs):
        dp, dc = np.abs(q.kf_pose - q0.kf_pose).max(), abs(r.chi2_vis - r0.chi2_vis) / r0.chi2_vis
        print("  max |dpose| %.3g  rel dchi2 %.3g" % (dp, dc))
        assert r.status == r0.status == 0 and r.its_done == r0.its_done and (r.obs_outlier == r0.obs_outlier).all()
        if exact:
            assert r.chi2_vis == r0.chi2_vis and (r.obs_chi2 == r0.obs_chi2).all()
            assert (q.kf_pose == q0.kf_pose).all() and (q.pt == q0.pt).all() and (q.kf_vel == q0.kf_vel).all()
        else:                                                   # across a threshold: the bound of tests/test_gpu_parity.py
            assert dc <= 1e-10 and dp < 1e-9


def test_one_chain_flips_two_sided_at_the_next_upload(monkeypatch):
    probs = [_tiny(i) for i in range(8)]
    monkeypatch.delenv("VBA_ONE_CHAIN", raising=False)
    cap = Capture(probs, 0)
    try:
        two_sided, n_up = pc.FIELDS.index("two_sided"), pc.N_UPLOAD
        first = _plan(cap)
        assert first[two_sided] == 1
        monkeypatch.setenv("VBA_ONE_CHAIN", "1")                # read at every upload: the same handle, no new process
        cap.ba.upload(probs)
        second = _plan(cap)
        assert second[two_sided] == 0 and second[n_up:] == [-1] * (len(pc.FIELDS) - n_up)      # no run of this upload yet
        assert [v for i, v in enumerate(second[:n_up]) if i != two_sided] == [v for i, v in enumerate(first[:n_up]) if i != two_sided]
        cap.ba.run()
        assert _plan(cap)[n_up:] == first[n_up:]
        monkeypatch.delenv("VBA_ONE_CHAIN")
        cap.ba.upload(probs)
        assert _plan(cap)[two_sided] == 1
    finally:
        cap.close()
