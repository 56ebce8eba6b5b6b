"""CPU checks of the stage-level reference (tests/stage_ref.py) that tests/test_gpu_stages.py holds the HIP kernels to: the
extended-precision Schur solve is the dense solve of the full system, the error bounds accept a float64 evaluation of the same
stages, and every bound is far tighter than the change one edge makes to S."""
import numpy as np
import pytest

import stage_ref as sr
from mc_slam_amd import abi, synth

CASES = [
    (abi.VARIANT_PRV_IDP, abi.ALGO_GN, dict(n_kf=12, n_fixed=2, n_pt=400, n_obs=2000, seed=41)),
    (abi.VARIANT_PRV_XYZ, abi.ALGO_LM, dict(n_kf=12, n_fixed=1, n_pt=400, n_obs=2000, seed=42)),
    (abi.VARIANT_SE3_XYZ, abi.ALGO_LM, dict(n_kf=12, n_fixed=2, n_pt=400, n_obs=2000, seed=43)),
]
IDS = ["idp", "prv_xyz", "se3_xyz"]


def _window(variant, algo, kw):
    return synth.make_window(variant, algo=algo, **kw)


def _ldlt(A):
    """unpivoted LDL^T in float64, column by column (the reference the bounds of the factor are checked on)"""
    n = A.shape[0]
    L = np.eye(n)
    d = np.zeros(n)
    for j in range(n):
        v = L[j, :j] * d[:j]
        d[j] = A[j, j] - L[j, :j] @ v
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ v) / d[j]
    return L, d


@pytest.mark.parametrize("with_lambda", [False, True])
@pytest.mark.parametrize("variant,algo,kw", CASES, ids=IDS)
def test_schur_solve_equals_dense_solve(oracle, variant, algo, kw, with_lambda):
    p = _window(variant, algo, kw)
    H, b, chi2, lvl = sr.linearize(p)
    pdim, L = sr.dims(p)
    np_ = pdim * p.n_kf_free
    var_act, pt_act = sr.active_sets(p, lvl)
    lam = sr.lambda_init(H, var_act, pt_act, np_, L) if with_lambda else 0.0
    red = sr.reduced(p, H, b, chi2, lvl, lam)
    dx = sr.full_step(red)
    # the full system with the same damping, identity rows for dofs outside the index mapping and for dropped landmarks
    act = np.concatenate([var_act, np.repeat(pt_act, L)])
    Hf = H + lam * np.diag(act.astype(float))
    bf = b.copy()
    out = np.flatnonzero(~act)
    Hf[out, :] = 0
    Hf[:, out] = 0
    Hf[out, out] = 1
    bf[out] = 0
    x = np.linalg.solve(Hf, bf)
    err = np.abs(dx - x).max() / np.abs(x).max()
    print("%s lambda=%.3g: |dx - dense solve| / |dx| = %.2e, cond(H) = %.2e" % ({0: "se3_xyz", 1: "prv_xyz", 2: "idp"}[variant], lam, err,
                                                                                  np.linalg.cond(Hf)))
    assert err <= 1e-12 * np.linalg.cond(Hf)
    assert np.abs(x).max() > 0


@pytest.mark.parametrize("variant,algo,kw", CASES, ids=IDS)
def test_bounds_accept_float64_stages(oracle, variant, algo, kw):
    p = _window(variant, algo, kw)
    H, b, chi2, lvl = sr.linearize(p)
    pdim, L = sr.dims(p)
    var_act, pt_act = sr.active_sets(p, lvl)
    lam = sr.lambda_init(H, var_act, pt_act, pdim * p.n_kf_free, L) if algo == abi.ALGO_LM else 0.0
    ref = sr.reduced(p, H, b, chi2, lvl, lam)
    f64 = sr.reduced(p, H, b, chi2, lvl, lam, dtype=np.float64)
    S, r = ref["S"].astype(np.float64), ref["r"].astype(np.float64)
    tS, tr = sr.tol_S(ref), sr.tol_r(ref)
    rS = sr.ratio(f64["S"] - S, tS)
    rr = sr.ratio(f64["r"] - r, tr)
    # the factor and the two triangular solves of the float64 system
    Lf, d = _ldlt(f64["S"])
    tF = sr.ldlt_tol(Lf, d)
    rF = sr.ratio((Lf * d) @ Lf.T - f64["S"], tF)
    y = np.linalg.solve(Lf, f64["r"])
    x = np.linalg.solve(Lf.T, y / d)
    ty, tx = sr.solve_tols(Lf, d, y, x)
    ry = sr.ratio(f64["r"] - Lf @ y, ty)
    rx = sr.ratio(y - d * (Lf.T @ x), tx)
    bound, ds, lmin = sr.xc_bound(S, tS + tF, tr, x)
    rX = np.linalg.norm(ds * (x - sr.solve_c(ref))) / bound
    rL = sr.ratio(sr.landmark_step(f64, x, dtype=np.float64) - sr.landmark_step(ref, x).astype(np.float64), sr.landmark_step_tol(ref, x))
    print("worst error / bound: S %.3f r %.3f factor %.3f Ly %.3f DL'x %.3f x_c %.3f landmarks %.3f (k %d, kappa %.1f)"
          % (rS, rr, rF, ry, rx, rX, rL, ref["k"], ref["kappa"]))
    for v in (rS, rr, rF, ry, rx, rX, rL):
        assert v <= 1.0


@pytest.mark.parametrize("variant,algo,kw", CASES, ids=IDS)
def test_bounds_are_sensitive_to_one_edge(oracle, variant, algo, kw):
    """the bounds of S, and of S + factor (what L D L^T is held to against the reference), must be at least 1e6 times smaller than
    what dropping one edge, or doubling its weight, does to S"""
    p = _window(variant, algo, kw)
    H, b, chi2, lvl = sr.linearize(p)
    ref = sr.reduced(p, H, b, chi2, lvl)
    tS = sr.tol_S(ref)
    base = ref["S"].astype(np.float64)
    tSF = tS + sr.ldlt_tol(*_ldlt(base))
    fix = np.zeros(p.n_kf, np.uint8) if p.kf_fix is None else p.kf_fix
    free = (np.asarray(p.obs_kf) < p.n_kf_free) & ((fix[p.obs_kf] & 1) == 0)
    rng = np.random.default_rng(7)
    margins = []
    for o in rng.choice(np.flatnonzero(free), 20, replace=False):
        for how in ("drop", "double"):
            q = p.copy()
            lv = lvl.copy()
            if how == "drop":
                lv[o] = 1
            else:
                q.obs_w[o] *= 2
            H2, b2, c2, _ = sr.linearize(q, lvl=lv)
            S2 = sr.reduced(q, H2, b2, c2, lv, dtype=np.float64)["S"]
            margins.append(((np.abs(S2 - base) / tS).max(), (np.abs(S2 - base) / tSF).max()))
    m = np.min(margins, axis=0)
    print("sensitivity: smallest change of S by one edge = %.2e x the S bound, %.2e x the S + factor bound" % tuple(m))
    assert m.min() >= 1e6
