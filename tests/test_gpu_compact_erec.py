"""The 32-byte inverse-depth edge record (P_c, sqrt(rho' w)) and the pixel copy beside it (obs_uvk): the diagonal Schur walk rebuilds the
weighted residual of b_p = -sum Bi^T r from the two instead of reading it from the record.  S, the reduced right-hand side, b_p and the
H_pp diagonal of one iteration against the extended-precision dense reference of tests/stage_ref.py, with its bounds as they are.

Windows of 2, 3 and 5 free keyframes (410..916 edges), started close to their optimum (one Gauss-Newton iteration per stage).  The walk of the diagonal pair (a, a) takes the items of keyframe a -- its edge
records, the landmark records it anchors, the run records of those -- 64 per trip, one per lane.  The shaped keyframes anchor no landmark,
so their items are exactly their edges, cut to 0, 1, 63, 64, 65, 127, 128 and 129: every boundary of the first three trips.  Every window
also has an unshaped free keyframe, and w5 one that anchors landmarks (reference and run records in its walk).

Among the edges (asserted: on the host where the inputs decide it, else on the captured state):
  * Huber weight below 1 in stage 1 (the generator's 5 % gross outliers);
  * level != 0 in stage 2 (what stage 1 classified out): record scale 0, the walk takes r as 0 by a select;
  * an edge whose landmark lies BEHIND the observing camera at the start (w2: the landmark is moved to a point in front of its
    reference camera and behind that observer): active in stage 1 with P_c.z < 0, classified out for stage 2;
  * observers listed as fixed (two per window), and in w3a a free keyframe whose PR vertex is fixed through kf_fix: scale 0 in its edge
    records although the edges are active -- the case in which the record used to hold a residual that the rebuilt one replaces by 0.

Every window runs alone (k_schur_all_w), inside ragged batches of 8 and of 9 windows (k_schur_all; the ninth window in front moves every
record base), and through the schur_split hook (k_schur_diag with k_schur_off_w / k_schur_off).  Both stages: its = 1 + 1, capture 0
is stage 1 at the initial state, capture 1 stage 2 with the levels of stage 1.  b_p and the H_pp diagonal are read from the device
after the run, so they are compared where the captured iteration is the run's last Schur launch (capture 1; the chi2-only probe is
switched off so that no pass is skipped).  For inverse-depth windows the H_pp diagonal the kernels keep is that of the IMU factors
alone (Gauss-Newton has no lambda init to feed): its reference is the dense H with every vision edge at level 1.

One C3-sized window against the oracle in both landmark orders: tests/test_gpu_parity.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import plan_cases
import stage_ref as sr
from mc_slam_amd import abi, synth
from test_gpu_compact_records import _subset
from test_gpu_stages import CTRL_A, LVL_A, PT_A, POSE_A, VEL_A, BIAS_A, S_B, VARACT_A, VEC_B, Capture, _ctrl

gpu = pytest.mark.gpu

# name -> (make_window arguments, {free keyframe: walk items}, kf_fix)
SPEC = dict(w5=(dict(n_kf=7, n_fixed=2, n_pt=300, n_obs=1200, seed=611), {1: 63, 2: 64, 3: 65, 4: 1}, {}),
            w3a=(dict(n_kf=5, n_fixed=2, n_pt=420, n_obs=1260, seed=612), {1: 127, 2: 128}, {0: 1}),
            w3b=(dict(n_kf=5, n_fixed=2, n_pt=420, n_obs=1260, seed=613), {1: 129, 2: 0}, {}),
            w2=(dict(n_kf=4, n_fixed=2, n_pt=200, n_obs=500, seed=614), {1: 64}, {}))
BEHIND = "w2"


def _shape(p, targets):
    """p with exactly targets[kf] walk items at keyframe kf: it anchors no landmark (no reference record, no run record) and
    observes that many edges"""
    p = _subset(p, np.ones(p.n_obs, bool), ~np.isin(np.asarray(p.pt_ref_kf), list(targets)))
    for kf, n in targets.items():
        idx = np.flatnonzero(p.obs_kf == kf)
        assert idx.size >= n, (kf, n, idx.size)
        keep = np.ones(p.n_obs, bool)
        keep[idx[n:]] = False
        p = _subset(p, keep, np.ones(p.n_pt, bool))   # (a landmark left without an edge goes: it had none elsewhere)
    return p


def _camera(p, k):
    """R_wc and the centre of keyframe k's camera"""
    import oracle_lib
    Tcb = np.asarray(p.T_cb, np.float64)
    Rcb = np.asarray(oracle_lib.quat_to_R(Tcb[3:7])).reshape(3, 3)
    Rwb = np.asarray(oracle_lib.quat_to_R(p.kf_pose[k, 3:7])).reshape(3, 3)
    return Rwb @ Rcb.T, Rwb @ (-Rcb.T @ Tcb[:3]) + p.kf_pose[k, :3]


def _edge_pc(p, q, o):
    import oracle_lib
    return oracle_lib.edge_idp(p.pt[q], p.kf_pose[int(p.pt_ref_kf[q])], p.kf_pose[int(p.obs_kf[o])], p.T_cb, np.asarray(p.K, np.float64),
                               p.obs_uv[o])[1]


def _behind(p):
    """(landmark, edge): the landmark moved to a point at least 5 cm in front of its reference camera and 5 cm behind the camera of
    one of its free observers -- the edge with the widest angle between the two optical axes, the point drawn at random around them"""
    beg = np.asarray(p.pt_obs_begin)
    pid = np.repeat(np.arange(p.n_pt), np.diff(beg))
    cand = [(float(_camera(p, int(p.pt_ref_kf[pid[o]]))[0][:, 2] @ _camera(p, int(p.obs_kf[o]))[0][:, 2]), o)
            for o in range(p.n_obs) if p.obs_kf[o] < p.n_kf_free and beg[pid[o] + 1] - beg[pid[o]] >= 2]
    rng = np.random.default_rng(9)
    for _, o in sorted(cand):
        q = int(pid[o])
        (R0, c0), (Ri, ci) = _camera(p, int(p.pt_ref_kf[q])), _camera(p, int(p.obs_kf[o]))
        X = ci + rng.normal(size=(4000, 3)) * np.exp(rng.uniform(np.log(0.2), np.log(50.0), (4000, 1)))
        P0, Pi = (X - c0) @ R0, (X - ci) @ Ri
        ok = np.flatnonzero((P0[:, 2] > 0.05) & (Pi[:, 2] < -0.05) & (np.abs(P0[:, :2]).max(axis=1) < 50 * P0[:, 2]))
        if ok.size:
            P = P0[ok[0]]
            return q, o, np.array([1.0 / P[2], P[0] / P[2], P[1] / P[2]])
    raise AssertionError("no landmark can be put behind one of its observers")


@functools.lru_cache(maxsize=None)
def windows():
    """name -> (window, info); built once, never changed (every upload copies)"""
    out = {}
    for name, (kw, targets, fix) in SPEC.items():
        p = _shape(synth.make_window(abi.VARIANT_PRV_IDP, landmark_order="caller", init_scale=0.2, **kw), targets)
        info = dict(targets=targets)
        if fix:
            p.kf_fix = np.zeros(p.n_kf, np.uint8)
            for kf, bits in fix.items():
                p.kf_fix[kf] = bits
        if name == BEHIND:
            q, o, pt = _behind(p)
            p.pt[q] = pt
            info.update(behind=(q, o))
        p.its_stage1, p.its_stage2 = 1, 1
        out[name] = (p, info)
    return out


def _filler(i):
    p = synth.make_window(abi.VARIANT_PRV_IDP, n_kf=5 + i % 3, n_fixed=1, n_pt=61 + 10 * i, n_obs=190 + 31 * i, seed=630 + i, init_scale=0.2)
    p.its_stage1, p.its_stage2 = 1, 1
    return p


def _batch(n):
    """(windows, {name: index}): ragged, the windows under test behind and between fillers; nine = eight with one more in front"""
    W = windows()
    order = ["f0", "w5", "w3a", "f1", "w3b", "w2", "f2", "f3"]
    if n == 9:
        order = ["f4"] + order
    probs = [_filler(int(s[1:])) if s[0] == "f" else W[s][0] for s in order]
    return probs, {s: i for i, s in enumerate(order) if s[0] == "w"}


def test_the_windows_are_what_they_claim():
    """(no GPU) free keyframes, walk items of the shaped keyframes, fixed observers, the kf_fix keyframe, the landmark behind a camera"""
    W = windows()
    assert sorted(p.n_kf_free for p, _ in W.values()) == [2, 3, 3, 5]
    seen = []
    for name, (p, info) in W.items():
        ref, okf = np.asarray(p.pt_ref_kf), np.asarray(p.obs_kf)
        for kf, n in info["targets"].items():
            assert kf < p.n_kf_free and (ref == kf).sum() == 0 and (okf == kf).sum() == n, (name, kf, n)
            seen.append(n)
        free_other = [k for k in range(p.n_kf_free) if k not in info["targets"]]
        assert free_other and all((okf == k).sum() > 129 for k in free_other), name   # an unshaped walk of more than two trips
        assert (okf >= p.n_kf_free).sum() >= 100, name                                 # observers listed as fixed
        assert p.its_stage1 == 1 and p.its_stage2 == 1
    assert sorted(set(seen)) == [0, 1, 63, 64, 65, 127, 128, 129]
    p5 = W["w5"][0]
    assert ((np.asarray(p5.pt_ref_kf) == 0).sum() >= 10) and p5.kf_fix is None      # a free keyframe that anchors landmarks
    p3 = W["w3a"][0]
    assert p3.kf_fix[0] == 1 and not p3.kf_fix[1:].any() and (np.asarray(p3.obs_kf) == 0).sum() > 129
    pb, ib = W[BEHIND]
    q, o = ib["behind"]
    assert pb.obs_kf[o] < pb.n_kf_free and _edge_pc(pb, q, o)[2] < -0.05             # behind its observer at the initial state
    sizes = [p.n_obs + p.n_pt for p in _batch(9)[0]]
    assert len(set(sizes)) == 9 and sizes[0] % 2 == 1                                # ragged; the window in front shifts by an odd count


# ---- one captured iteration against the dense reference -------------------------------------------------------------------------
def _bpose(cap, w, lays):
    """(b_p, H_pp diagonal) of window w as the last Schur launch of the run left them (buffer BPOSE: 2 nS doubles per window)"""
    lib = cap.lib
    lib.vba_debug_buf_id.argtypes = [C.c_char_p]
    lib.vba_debug_copy.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_uint64]
    nS = lays[w]["nS"]
    vec0 = sum(l["nS"] for l in lays[:w])
    a = np.zeros(2 * nS)
    assert lib.vba_debug_copy(cap.ba.h, lib.vba_debug_buf_id(b"BPOSE"), 16 * vec0, a.ctypes.data, a.nbytes) == 0
    return a[:nS], a[nS:]


def _check_products(cap, w, name, stage, schur, lays):
    p, info = windows()[name]
    lay = lays[w]
    nS, pdim, nf = lay["nS"], lay["pdim"], p.n_kf_free
    assert lay["schur"] == schur and lay["n_free"] == nf, (lay["schur"], schur)
    ctrl = _ctrl(cap.get(CTRL_A, w, np.uint8, lay["ctrl_bytes"]), lay["ctrl_off"])
    assert ctrl["active"] == 1 and ctrl["stage"] == stage and ctrl["robust_vis"] == (stage == 0), ctrl
    q = p.copy()
    q.kf_pose[...] = cap.get(POSE_A, w, np.float64, 7 * p.n_kf).reshape(-1, 7)
    q.kf_vel = cap.get(VEL_A, w, np.float64, 3 * p.n_kf).reshape(-1, 3)
    q.kf_bias = cap.get(BIAS_A, w, np.float64, 12 * p.n_kf).reshape(-1, 12)
    q.pt[...] = cap.get(PT_A, w, np.float64, 3 * p.n_pt).reshape(-1, 3)
    lvl = cap.get(LVL_A, w, np.uint8, p.n_obs)
    robust = stage == 0
    # what the case claims of its edges
    if stage == 0:
        assert not lvl.any() and np.array_equal(q.pt, p.pt)
        E = sr.idp_edge_terms(q, lvl, True)
        act_w = np.asarray(p.obs_w)[lvl == 0]
        assert (E["Wt"] < act_w * (1 - 1e-9)).sum() >= 3, "no edge with a Huber weight below 1"
    else:
        assert 0 < (lvl != 0).sum() < p.n_obs // 2 and (lvl[np.asarray(p.obs_kf) < p.n_kf_free] != 0).any(), (lvl != 0).sum()
        if "behind" in info:
            assert lvl[info["behind"][1]] != 0, "stage 1 kept the edge behind the camera"
    H, b, chi2, lvl = sr.linearize(q, robust, lvl)
    var_act, _ = sr.active_sets(q, lvl)
    red = sr.reduced(q, H, b, chi2, lvl, 0.0)
    rows, pads = sr.window_rows(lay)
    va = cap.get(VARACT_A, w, np.int32, nS)
    assert np.array_equal(va[rows] != 0, var_act) and not va[pads].any()
    if p.kf_fix is not None:
        assert not var_act[:6].any() and var_act[6:15].all()          # w3a, keyframe 0: PR outside the index mapping, V and Bias inside
    Sref = sr.to_window(red["S"].astype(np.float64), lay)
    rref = sr.to_window(red["r"].astype(np.float64), lay)
    tS = sr.to_window(sr.tol_S(red), lay, pad_value=0.0)
    tr = sr.to_window(sr.tol_r(red), lay)
    S = cap.get(S_B, w, np.float64, nS * nS).reshape(nS, nS)
    r = cap.get(VEC_B, w, np.float64, nS)
    # S: the tiles the factor reads, as tests/test_gpu_stages.py compares it (right-looking factor: a tile it never touches may hold anything)
    F = cap.factor(w, nS)
    nb = lay["nb"]
    tile_on = np.abs(F).reshape(nb, 32, nb, 32).max(axis=(1, 3)) > 0
    read = (np.kron(tile_on | np.eye(nb, dtype=bool), np.ones((32, 32), bool)) if not lay["l_packed"] else np.ones((nS, nS), bool)) & np.tril(np.ones((nS, nS), bool))
    res = dict(S=sr.ratio(np.where(read, S - Sref, 0), tS), r=sr.ratio(r - rref, tr))
    where = sr.format_blocks(sr.worst_blocks(np.where(read, S - Sref, 0), tS, lay, var_act))
    if stage == 1:
        bp, hd = _bpose(cap, w, lays)
        # b_p = J^T W e over the vision and IMU factors of a keyframe: the first term of the bound of r (stage_ref: Cauchy-Schwarz)
        tb = sr.to_window(8.0 * sr.EPS * (red["k"] + red["kappa"]) * np.sqrt(red["h"] * max(chi2, 0.0)), lay)
        bref = sr.to_window(np.where(var_act, b[:pdim * nf], 0.0), lay)
        res["b_p"] = sr.ratio(bp - bref, tb)
        Himu = sr.linearize(q, robust, np.ones(p.n_obs, np.uint8))[0]
        hi = np.where(var_act, np.diag(Himu)[:pdim * nf], 0.0)
        res["H_pp_diag"] = sr.ratio(hd - sr.to_window(hi, lay), sr.to_window(8.0 * sr.EPS * red["k"] * np.abs(hi), lay))
        assert np.abs(bref).max() > 0 and np.abs(hi).max() > 0
    print("  %-4s window %d stage %d (nS %d, k %d, levels %d): error / bound %s; %s"
          % (name, w, stage + 1, nS, red["k"], int((lvl != 0).sum()), " ".join("%s %.3g" % kv for kv in res.items()), where))
    for key, v in res.items():
        assert v <= 1.0, (name, key, v, res, where)


def _run(probs, which, stage, schur, split):
    cap = Capture(probs, stage, path=[("lin_probe", 0)] + ([("schur_split", 1)] if split else []))
    try:
        lays = [cap.layout(w) for w in range(len(probs))]
        for name, w in which.items():
            _check_products(cap, w, name, stage, schur, lays)
    finally:
        cap.close()


@gpu
@pytest.mark.parametrize("stage", [0, 1], ids=["stage1", "stage2"])
@pytest.mark.parametrize("split", [0, 1], ids=["k_schur_all_w", "split"])
@pytest.mark.parametrize("name", list(SPEC))
def test_one_window_alone(name, split, stage):
    _run([windows()[name][0]], {name: 0}, stage, plan_cases.SCHUR_SPLIT_W if split else plan_cases.SCHUR_ALL_W, split)


@gpu
@pytest.mark.parametrize("stage", [0, 1], ids=["stage1", "stage2"])
@pytest.mark.parametrize("n,split", [(8, 0), (9, 0), (9, 1)], ids=["eight", "nine", "nine_split"])
def test_ragged_batch(n, split, stage):
    probs, which = _batch(n)
    _run(probs, which, stage, plan_cases.SCHUR_SPLIT if split else plan_cases.SCHUR_ALL, split)
