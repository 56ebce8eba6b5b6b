"""CPU checks of the stage-level reference (tests/stage_ref.py) that tests/test_gpu_stages.py holds the HIP kernels to: the
extended-precision Schur solve is the dense solve of the full system, the error bounds accept a float64 evaluation of the same
stages, and every bound is far tighter than the change one edge makes to S."""
import numpy as np
import pytest

import kf_fix_cases as kc
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


# ---- where a stage failure is: the block report of stage_ref.worst_blocks ---------------------------------------------------------
def test_worst_blocks_names_the_perturbed_block(oracle):
    """one entry of a reference S moved by 100 bounds, in a window order that permutes the rows: the report names the keyframe pair
    and the sub-block in the oracle's order, says which of the two vertices is outside the index mapping, and is empty otherwise"""
    p = kc.window("idp", "pr_mid")
    H, b, chi2, lvl = sr.linearize(p)
    ref = sr.reduced(p, H, b, chi2, lvl, dtype=np.float64)
    np_ = 15 * p.n_kf_free
    nS = 160
    vpos = np.random.default_rng(5).permutation(np_)         # rows of the window: any order, the pads behind them
    lay = dict(nS=nS, pdim=15, n_free=p.n_kf_free, vpos=vpos, pad0=[np_, 0, 0], padn=[nS - np_, 0, 0])
    tS = sr.to_window(sr.tol_S(ref), lay, pad_value=0.0)
    low = np.tril(np.ones((nS, nS), bool))
    assert sr.worst_blocks(np.zeros((nS, nS)), tS, lay, ref["var_act"]) == []
    assert sr.format_blocks([]) == "every block within its bound"
    for (a, ra, b_, cb, want) in [(6, 7, 3, 2, (6, 3, "V", "PR", True, True)),        # V of 6 x PR of 3
                                  (7, 4, 4, 1, (7, 4, "PR", "PR", True, False)),      # PR of 7 x the fixed PR of 4
                                  (5, 12, 5, 9, (5, 5, "Bias", "Bias", True, True)),  # inside a diagonal block
                                  (2, 0, 8, 14, (8, 2, "Bias", "PR", True, True))]:   # given as (b, a): reported with a >= b
        i, j = vpos[15 * a + ra], vpos[15 * b_ + cb]
        i, j = max(i, j), min(i, j)                                                  # the lower triangle of the window
        dS = np.zeros((nS, nS))
        dS[i, j] = 100 * tS[i, j]
        dS[vpos[0], vpos[0]] = 0.5 * tS[vpos[0], vpos[0]]                             # within its bound: not reported
        got = sr.worst_blocks(np.where(low, dS, 0), tS, lay, ref["var_act"])
        assert len(got) == 1 and got[0][1:] == want and abs(got[0][0] - 100) < 1e-9, got
        text = sr.format_blocks(got)
        assert ("kf %d %s" % want[:3:2]) in text and ("outside the index mapping" in text) == (not want[5]), text


# ---- fixed vertices inside the free range: the reference is fit for every pattern the GPU tests run ---------------------------------
@pytest.mark.parametrize("pattern", list(kc.PATTERNS))
@pytest.mark.parametrize("variant", list(kc.VARIANTS))
def test_reference_is_fit_for_every_fixed_vertex_pattern(oracle, variant, pattern):
    """for every kf_fix pattern of tests/test_gpu_kf_fix.py: the float64 reduced system is positive definite (identity rows for the
    vertices outside the index mapping: its smallest eigenvalue is 1 or above the rounding of the largest), and the float64 reference
    stays within tol_S and landmark_step_tol of the extended-precision one -- a negative pivot on the GPU is the kernels' doing"""
    p = kc.window(variant, pattern)
    H, b, chi2, lvl = sr.linearize(p)
    pdim, L = sr.dims(p)
    var_act, pt_act = sr.active_sets(p, lvl)
    fix = p.kf_fix
    for kf, bits in kc.PATTERNS[pattern].items():            # the pattern reaches the index mapping
        for part, lo in ((0, 0), (1, 6), (2, 9)):
            if (bits >> part) & 1:
                assert not var_act[pdim * kf + lo]
    lam = sr.lambda_init(H, var_act, pt_act, pdim * p.n_kf_free, L) if p.algo == abi.ALGO_LM else 0.0
    ref = sr.reduced(p, H, b, chi2, lvl, lam)
    f64 = sr.reduced(p, H, b, chi2, lvl, lam, dtype=np.float64)
    ev = np.linalg.eigvalsh(f64["S"])
    act = np.flatnonzero(var_act)
    ev_act = np.linalg.eigvalsh(f64["S"][np.ix_(act, act)])
    x = sr.solve_c(ref)
    rS = sr.ratio(f64["S"] - ref["S"].astype(np.float64), sr.tol_S(ref))
    rL = sr.ratio(sr.landmark_step(f64, x, dtype=np.float64) - sr.landmark_step(ref, x).astype(np.float64), sr.landmark_step_tol(ref, x))
    print("%s %s: eigenvalues of S %.3g .. %.3g (active rows from %.3g), float64 vs long double: S %.2e, landmark step %.2e of the bound"
          % (variant, pattern, ev.min(), ev.max(), ev_act.min(), rS, rL))
    assert ev.min() > 0.5 and ev_act.min() > 1e3 * sr.EPS * ev.max() * len(ev)
    assert rS <= 1.0 and rL <= 1.0


# ---- the landmark bound holds the reference itself: inputs perturbed by one unit roundoff ------------------------------------------
def stage_two_state(oracle):
    """the state and levels test_gpu_stages.py::test_idp_stage_two_with_levels captures: stage 1 (two iterations) on the CPU oracle --
    the same levels, the state to 1e-13, as that GPU run gave"""
    p = synth.make_window(abi.VARIANT_PRV_IDP, n_kf=12, n_fixed=2, n_pt=400, n_obs=800, seed=56, pix_noise=3.0)
    p.its_stage1, p.its_stage2 = 2, 0
    q, r = oracle.solve(p)
    return q, r.obs_outlier.astype(np.uint8)


def test_perturbed_reference_stays_inside_the_landmark_bound(oracle):
    """Stage 2 of the low-parallax case (one or two active edges per landmark, three-pixel noise): every input -- poses, landmark
    parameters, pixel coordinates -- perturbed by independent relative errors of one unit roundoff, the landmark step recomputed in
    float64 over 32 draws at a fixed x_c.  The reference must stay inside its own bound.  The accumulation part of the bound alone
    (exact W, Dinv, b_l) does not hold it: the spread reaches 16 to 31 times that part, at the landmarks where J_rho cancels; with
    the forward-error term of landmark_step_tol it stays below a quarter of the bound.  The bound is still far below what an edge
    does: doubling the weight of one edge of a landmark with two moves its step by more than 1e6 bounds, and the margin of the S
    bounds of this state (what test_gpu_stages._sensitivity measures) is unchanged and at least 1e6."""
    q, lvl = stage_two_state(oracle)
    beg = np.asarray(q.pt_obs_begin)
    n_act = np.add.reduceat((lvl == 0).astype(int), beg[:-1])
    assert (n_act == 0).sum() > 0 and (n_act == 1).sum() > 50
    H, b, chi2, lvl = sr.linearize(q, False, lvl)
    ref = sr.reduced(q, H, b, chi2, lvl)
    xc = sr.solve_c(ref)
    base = sr.landmark_step(ref, xc).astype(np.float64)[:, 0]
    tol = sr.landmark_step_tol(ref, xc, robust_vis=False)[:, 0]
    accum = 8 * sr.EPS * (ref["k"] + ref["kappa"]) * np.abs(ref["Dinv"][:, 0, 0].astype(np.float64)) \
        * (np.abs(ref["bl"][:, 0].astype(np.float64)) + np.einsum("cp,c->p", np.abs(ref["W"][:, :, 0].astype(np.float64)), np.abs(xc)))
    E = sr.idp_edge_terms(q, lvl, False)
    D = np.zeros(base.size)
    np.add.at(D, E["lm"], E["Wt"] * (E["J"] ** 2).sum(axis=1))
    assert np.abs(D * ref["Dinv"][:, 0, 0].astype(np.float64) - 1).max() < 1e-12     # the per-edge terms are those of the oracle's H
    rng = np.random.default_rng(1)
    pert = lambda a: a * (1.0 + sr.EPS * rng.choice([-1.0, 1.0], a.shape))
    spread = np.zeros(base.size)
    for _ in range(32):
        z = q.copy()
        z.kf_pose, z.pt, z.obs_uv = pert(q.kf_pose), pert(q.pt), pert(q.obs_uv)
        H2, b2, c2, _ = sr.linearize(z, False, lvl)
        d = sr.landmark_step(sr.reduced(z, H2, b2, c2, lvl, dtype=np.float64), xc, dtype=np.float64)[:, 0]
        spread = np.maximum(spread, np.abs(d - base))
    i = int((spread / tol).argmax())
    print("perturbed reference: %.3g x the accumulation bound alone, %.3g x the bound (active landmark %d, step %.3g); bound / |step| at most %.2e"
          % ((spread / accum).max(), spread[i] / tol[i], i, base[i], (tol / np.abs(base)).max()))
    assert (spread / accum).max() > 4.0          # the accumulation bound alone does not hold the reference (the recorded finding)
    assert (spread <= tol).all()
    # sensitivity: one edge's weight doubled, on landmarks with two active edges
    act = np.flatnonzero(ref["pt_act"])
    margins = []
    for lm in np.flatnonzero(n_act[act] == 2)[:8]:
        o = next(o for o in range(beg[act[lm]], beg[act[lm] + 1]) if lvl[o] == 0)
        z = q.copy()
        z.obs_w = q.obs_w.copy()
        z.obs_w[o] *= 2
        H2, b2, c2, _ = sr.linearize(z, False, lvl)
        d = sr.landmark_step(sr.reduced(z, H2, b2, c2, lvl, dtype=np.float64), xc, dtype=np.float64)[:, 0]
        margins.append(abs(d[lm] - base[lm]) / tol[lm])
    tS = sr.tol_S(ref)
    S0 = ref["S"].astype(np.float64)
    tSF = tS + sr.ldlt_tol(*_ldlt(S0))
    ms = []
    free = np.flatnonzero((lvl == 0) & (np.asarray(q.obs_kf) < q.n_kf_free))
    for o in np.random.default_rng(3).choice(free, 4, replace=False):
        lv = lvl.copy()
        lv[o] = 1
        H2, b2, c2, _ = sr.linearize(q, False, lv)
        ms.append((np.abs(sr.reduced(q, H2, b2, c2, lv, dtype=np.float64)["S"] - S0) / tSF).max())
    print("one edge: landmark step moves by at least %.2e bounds, S by at least %.2e bounds" % (min(margins), min(ms)))
    assert len(margins) == 8 and min(margins) >= 1e6 and min(ms) >= 1e6
