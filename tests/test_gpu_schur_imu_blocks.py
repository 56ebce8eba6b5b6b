"""The Schur kernels' block writer and diagonal walk on the smallest windows where they can go wrong, against the dense reference of
tests/stage_ref.py (capture of the first solve iteration, hooks flavour, as in tests/test_gpu_stages.py).

Checked per window, in units of the bounds stage_ref derives (c eps (k + kappa) sqrt(h_i h_j) for S, its rhs twin for vectors):
  * S on every tile the factor reads, and the reduced right-hand side;
  * bpose: the unreduced b_p, and the H_pp diagonal the kernels park behind it.  Inverse-depth windows run Gauss-Newton and park the
    IMU terms of the diagonal only (schur_diag_body: the vision terms feed Levenberg-Marquardt's lambda init, which they never run),
    so their reference is the diagonal of H linearised with every vision edge at level 1; XYZ windows park the whole diagonal.
    Gauss-Newton windows stop at their second terminate() poll (vba_debug_set_stop_after 1), so that the buffer still holds what
    the captured iteration wrote.  Under Levenberg-Marquardt the pass that opens an outer iteration writes b_p and the diagonal
    BEFORE that iteration's poll: the XYZ window is run a second time, stopped at its first poll, and read then.
Windows: 2, 3 and 5 free keyframes behind the fixed predecessor (one IMU factor on the first and last keyframe, two in between; nS 32,
64, 96), a broken IMU chain (two neighbour pairs without a factor, a keyframe with none), a keyframe outside the active set, and
windows thinned until chosen keyframes have exactly 0, 1, 63, 64, 65, 127, 128 and 129 walk items (slot + reference + run records;
the counts are asserted on the host and against the uploaded segment tables).  Each alone (64 lanes per pair), in a batch of 8 and
of 9 ragged windows (16 lanes per pair), with the fused and the split Schur kernels; one PRV-XYZ window under Levenberg-Marquardt."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import stage_ref as sr
from mc_slam_amd import abi, synth, backend

gpu = pytest.mark.gpu

POSE_A, VEL_A, BIAS_A, PT_A, CTRL_A, LVL_A, VARACT_A, S_B, VEC_B = range(9)   # capture items (vba_host_run.h, CAP_*)
WALK_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129)


# ---- windows ---------------------------------------------------------------------------------------------------------------------
def _idp(**kw):
    return synth.make_window(abi.VARIANT_PRV_IDP, n_fixed=1, **kw)


def _subset(p, keep_obs, keep_pt=None):
    """p without the edges that keep_obs drops and without the landmarks keep_pt drops or that are left with no edge (valid CSR)"""
    beg = np.asarray(p.pt_obs_begin, np.int64)
    pid = np.repeat(np.arange(p.n_pt), np.diff(beg))
    keep_obs = np.asarray(keep_obs, bool) & (True if keep_pt is None else np.asarray(keep_pt, bool)[pid])
    cnt = np.bincount(pid[keep_obs], minlength=p.n_pt)
    kp = cnt > 0
    return dataclasses.replace(p, pt=p.pt[kp].copy(), pt_ref_kf=p.pt_ref_kf[kp].copy(),
                               pt_obs_begin=np.concatenate([[0], np.cumsum(cnt[kp])]), obs_kf=p.obs_kf[keep_obs].copy(),
                               obs_uv=p.obs_uv[keep_obs].copy(), obs_w=p.obs_w[keep_obs].copy(), kf_pose=p.kf_pose.copy(),
                               kf_vel=p.kf_vel.copy(), kf_bias=p.kf_bias.copy(), truth={})


def _without_imu_of(p, kf):
    keep = (p.imu_kf_i != kf) & (p.imu_kf_j != kf)
    return dataclasses.replace(p, imu_kf_i=p.imu_kf_i[keep].copy(), imu_kf_j=p.imu_kf_j[keep].copy(),
                               imu_meas=p.imu_meas[keep].copy(), imu_info_prv=p.imu_info_prv[keep].copy(), truth={})


def walk_items(p):
    """walk items of every free keyframe's diagonal pair: its slot records (edges it observes), the landmark records it is the
    reference keyframe of, and its run records -- runs of consecutive landmarks with one reference keyframe inside a work unit of the
    linearisation (at most 64 landmarks and 256 edges, vba_host_structure.h)"""
    k = np.diff(np.asarray(p.pt_obs_begin, np.int64))
    ref = np.asarray(p.pt_ref_kf)
    items = np.bincount(p.obs_kf, minlength=p.n_kf) + np.bincount(ref, minlength=p.n_kf)
    pt = 0
    while pt < p.n_pt:
        first, ne = pt, 0
        while pt < p.n_pt and pt - first < 64 and ne + k[pt] <= 256:
            ne += k[pt]
            pt += 1
        assert pt > first
        for q in range(first, pt):
            if q == first or ref[q] != ref[q - 1]:
                items[ref[q]] += 1
    return items[:p.n_kf_free]


def _thinned(seed, targets):
    """a 9-keyframe window with observations deleted until, for every count of `targets`, some free keyframe has exactly that many
    walk items (0 and 1: the last keyframe, which is nobody's reference).  Returns (window, {count: keyframe})."""
    p = _idp(n_kf=10, n_pt=300, n_obs=900, seed=seed)
    last = p.n_kf_free - 1
    beg = np.asarray(p.pt_obs_begin, np.int64)
    if min(targets) <= 1:   # landmarks seen from the last keyframe alone go first: its edges can then all be deleted
        only_last = (np.diff(beg) == 1) & (p.obs_kf[beg[:-1]] == last)
        p = _subset(p, np.ones(p.n_obs, bool), ~only_last)
        beg = np.asarray(p.pt_obs_begin, np.int64)
    assert not (np.asarray(p.pt_ref_kf) == last).any()
    # work units end at 64 landmarks, never at 256 edges: deleting edges cannot move a run boundary
    assert np.add.reduceat(np.diff(beg), np.arange(0, p.n_pt, 64)).max() <= 256
    pid = np.repeat(np.arange(p.n_pt), np.diff(beg))
    left = np.diff(beg).copy()
    keep = np.ones(p.n_obs, bool)
    have = walk_items(p)
    floor = have - np.bincount(p.obs_kf, minlength=p.n_kf)[:p.n_kf_free]   # what deleting edges cannot take away
    where = {}
    for t in sorted(targets):
        # (the edges a keyframe can lose: those of landmarks that keep another one)
        can = lambda a: int((left[pid[(p.obs_kf == a) & keep]] >= 2).sum())
        cand = [last] if t <= 1 else [a for a in range(last) if a not in where.values()]
        cand = [a for a in cand if 0 <= have[a] - t <= can(a)]
        assert cand, (t, floor.tolist(), have.tolist())
        a = where[t] = cand[0]
        drop = have[a] - t
        for o in np.flatnonzero(p.obs_kf == a):
            if drop and left[pid[o]] >= 2:
                keep[o] = False
                left[pid[o]] -= 1
                drop -= 1
        assert drop == 0, (t, a, drop)
    q = _subset(p, keep)
    assert q.n_pt == p.n_pt
    got = walk_items(q)
    assert all(got[a] == t for t, a in where.items()), (where, got.tolist())
    return q, where


@functools.lru_cache(maxsize=None)
def windows():
    """name -> window (built once, never changed: every upload copies)"""
    out = dict(free2=_idp(n_kf=3, n_pt=80, n_obs=120, seed=301),          # nS 30 -> 32: below one tile
               free3=_idp(n_kf=4, n_pt=100, n_obs=200, seed=302),         # 45 -> 64
               free5=_idp(n_kf=6, n_pt=150, n_obs=450, seed=303))         # 75 -> 96
    # keyframe 2 of five without an IMU factor: pairs (1,2) and (2,3) carry none either, its V / bias dofs leave the active set
    out["broken_chain"] = _without_imu_of(_idp(n_kf=6, n_pt=150, n_obs=450, seed=304), 2)
    # ... and without an edge or a landmark of its own: the whole keyframe is outside the index mapping (identity block)
    p = _without_imu_of(_idp(n_kf=6, n_pt=150, n_obs=450, seed=305), 2)
    out["inactive_keyframe"] = _subset(p, p.obs_kf != 2, np.asarray(p.pt_ref_kf) != 2)
    out["walk_a"], wa = _thinned(311, (0, 63, 127))
    out["walk_b"], wb = _thinned(312, (1, 64, 128))
    out["walk_c"], wc = _thinned(313, (65, 129))
    assert sorted(list(wa) + list(wb) + list(wc)) == sorted(WALK_COUNTS)
    return out, dict(walk_a=wa, walk_b=wb, walk_c=wc)


KINDS = ("free2", "free3", "free5", "broken_chain", "inactive_keyframe", "walk_a", "walk_b", "walk_c")
BATCH8 = ("free2", "free3", "free5", "broken_chain", "inactive_keyframe", "walk_a", "walk_b", "walk_c")
BATCH9 = ("walk_c", "free5", "inactive_keyframe", "free2", "walk_a", "broken_chain", "free3", "walk_b", "free5")


def test_the_windows_are_what_they_claim():
    """(no GPU) IMU factors per keyframe, the keyframe outside every edge, the walk-item counts"""
    W, where = windows()
    per_kf = lambda p: (np.bincount(p.imu_kf_i, minlength=p.n_kf) + np.bincount(p.imu_kf_j, minlength=p.n_kf))[:p.n_kf_free].tolist()
    assert per_kf(W["free2"]) == [2, 1] and per_kf(W["free3"]) == [2, 2, 1] and per_kf(W["free5"]) == [2, 2, 2, 2, 1]
    assert per_kf(W["broken_chain"]) == [2, 1, 0, 1, 1] == per_kf(W["inactive_keyframe"])
    assert (W["broken_chain"].obs_kf == 2).any()
    p = W["inactive_keyframe"]
    assert not (p.obs_kf == 2).any() and not (np.asarray(p.pt_ref_kf) == 2).any() and walk_items(p)[2] == 0
    seen = sorted(int(walk_items(W[name])[a]) for name, m in where.items() for a in m.values())
    assert seen == sorted(WALK_COUNTS)


# ---- capture ---------------------------------------------------------------------------------------------------------------------
class Capture:
    """one vba_batch_run on a fresh handle of the hooks flavour: capture of the first solve iteration (stop_after 1: every window
    stops after it), or no capture at all (stop_after 0: every window stops at its first poll)"""

    def __init__(self, probs, split, stop_after=1):
        self.ba = backend.LocalBA(0, hooks=True)
        lib = self.lib = self.ba.lib
        h = self.ba.h
        lib.vba_debug_set_path.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
        lib.vba_debug_set_stop_after.argtypes = [C.c_void_p, C.c_int32]
        lib.vba_debug_capture_get.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64]
        lib.vba_debug_window_layout.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64]
        lib.vba_debug_factor_dense.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int64]
        lib.vba_debug_copy.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_uint64]
        lib.vba_debug_buf_id.argtypes = [C.c_char_p]
        assert lib.vba_debug_set_streams(h, 1) == 0
        assert lib.vba_debug_set_stop_after(h, stop_after) == 0
        assert lib.vba_debug_set_path(h, b"schur_split", 1 if split else 0) == 0
        self.ba.upload(probs)
        assert stop_after == 0 or lib.vba_debug_capture(h, 0) == 0
        self.ba.run()
        self.probs = probs
        self.lays = [self.layout(w) for w in range(len(probs))]

    def close(self):
        self.ba.close()

    def layout(self, w):
        p = self.probs[w]
        pdim, _ = sr.dims(p)
        n = 20 + pdim * p.n_kf_free + 6
        out = np.zeros(n, np.int64)
        assert self.lib.vba_debug_window_layout(self.ba.h, w, out.ctypes.data_as(C.POINTER(C.c_int64)), n) == 0
        k = 20 + pdim * p.n_kf_free
        return dict(nS=int(out[0]), nb=int(out[1]), pdim=int(out[2]), n_free=int(out[3]), l_packed=int(out[7]), schur=int(out[10]),
                    ctrl_bytes=int(out[13]), ctrl_off=dict(stage=int(out[16]), active=int(out[17]), robust_vis=int(out[18]), lam=int(out[19])),
                    vpos=out[20:k].copy(), pad0=out[k:k + 3].tolist(), padn=out[k + 3:k + 6].tolist())

    def get(self, what, w, dtype, count):
        a = np.zeros(count, dtype)
        assert self.lib.vba_debug_capture_get(self.ba.h, what, w, a.ctypes.data, a.nbytes) == 0, self.lib.vba_last_error(self.ba.h)
        return a

    def buf(self, name, first, count, dtype):
        """`count` elements of a device buffer as the run left it"""
        a = np.zeros(count, dtype)
        bid = self.lib.vba_debug_buf_id(name)
        assert bid >= 0 and self.lib.vba_debug_copy(self.ba.h, bid, first * a.itemsize, a.ctypes.data, a.nbytes) == 0, name
        return a

    def factor(self, w, nS):
        F = np.zeros((nS, nS))
        assert self.lib.vba_debug_factor_dense(self.ba.h, w, F.ctypes.data_as(C.POINTER(C.c_double)), nS * nS) == 0
        return F


_refs = {}


def reference(name, q, robust, lvl):
    """the dense reference of window `name` at the captured state: computed once, shared by every case that captures the same state"""
    key = (name, robust, q.kf_pose.tobytes(), q.kf_vel.tobytes(), q.kf_bias.tobytes(), q.pt.tobytes(), lvl.tobytes())
    if key not in _refs:
        H, b, chi2, lvl = sr.linearize(q, robust, lvl)
        pdim, L = sr.dims(q)
        var_act, pt_act = sr.active_sets(q, lvl)
        lam = sr.lambda_init(H, var_act, pt_act, pdim * q.n_kf_free, L) if q.algo == abi.ALGO_LM else 0.0
        red = sr.reduced(q, H, b, chi2, lvl, lam, dtype=sr.LD)
        n = red["np"]
        if q.variant == abi.VARIANT_PRV_IDP:   # the IMU terms of the diagonal: H with every vision edge at level 1
            hd = np.diag(sr.linearize(q, robust, np.ones(q.n_obs, np.uint8))[0])[:n].copy()
        else:
            hd = np.diag(H)[:n].copy()
        _refs[key] = dict(red=red, var_act=var_act, lam=lam, bp=np.where(var_act, b[:n], 0.0), hd=np.where(var_act, hd, 0.0))
    return _refs[key]


def check_bpose(cap, w, name, ref, va, res):
    """bpose of window w as the run left it: [0, nS) the unreduced b_p, [nS, 2 nS) the parked H_pp diagonal (windows lie in upload
    order)"""
    lay, red = cap.lays[w], ref["red"]
    nS = lay["nS"]
    _, pads = sr.window_rows(lay)
    vec0 = sum(l["nS"] for l in cap.lays[:w])
    assert np.array_equal(cap.buf(b"VARACT", vec0, nS, np.int32), va)
    bpose = cap.buf(b"BPOSE", 2 * vec0, 2 * nS, np.float64)
    assert not bpose[:nS][pads].any() and not bpose[nS:][pads].any()
    res["b_p"] = sr.ratio(bpose[:nS] - sr.to_window(ref["bp"], lay), sr.to_window(sr.tol_r(red), lay))
    th = 8.0 * sr.EPS * (red["k"] + red["kappa"]) * np.abs(ref["hd"])
    res["H_pp_diag"] = sr.ratio(bpose[nS:] - sr.to_window(ref["hd"], lay), sr.to_window(th, lay))


def check_window(cap, w, name, schur, bpose_from=None):
    p, lay = cap.probs[w], cap.lays[w]
    nS = lay["nS"]
    assert lay["schur"] == schur, (lay["schur"], schur)
    raw = cap.get(CTRL_A, w, np.uint8, lay["ctrl_bytes"])
    i32 = lambda o: int(np.frombuffer(raw[o:o + 4].tobytes(), np.int32)[0])
    off = lay["ctrl_off"]
    assert i32(off["active"]) == 1 and i32(off["stage"]) == 0
    q = p.copy()
    q.kf_pose[...] = cap.get(POSE_A, w, np.float64, 7 * p.n_kf).reshape(-1, 7)
    q.kf_vel = cap.get(VEL_A, w, np.float64, 3 * p.n_kf).reshape(-1, 3)
    q.kf_bias = cap.get(BIAS_A, w, np.float64, 12 * p.n_kf).reshape(-1, 12)
    q.pt[...] = cap.get(PT_A, w, np.float64, 3 * p.n_pt).reshape(-1, 3)
    lvl = cap.get(LVL_A, w, np.uint8, p.n_obs)
    ref = reference(name, q, bool(i32(off["robust_vis"])), lvl)
    red, var_act = ref["red"], ref["var_act"]
    if p.algo == abi.ALGO_LM:
        lam = float(np.frombuffer(raw[off["lam"]:off["lam"] + 8].tobytes(), np.float64)[0])
        assert abs(lam - ref["lam"]) <= 1e-12 * ref["lam"], (lam, ref["lam"])
    rows, pads = sr.window_rows(lay)
    va = cap.get(VARACT_A, w, np.int32, nS)
    assert np.array_equal(va[rows] != 0, var_act) and not va[pads].any()
    tS = sr.to_window(sr.tol_S(red), lay, pad_value=0.0)
    tr = sr.to_window(sr.tol_r(red), lay)
    S = cap.get(S_B, w, np.float64, nS * nS).reshape(nS, nS)
    r = cap.get(VEC_B, w, np.float64, nS)
    # tiles the factor reads: everything when S stays pristine (left-looking), else the tiles of the factor's lists
    F = cap.factor(w, nS)
    nb = lay["nb"]
    tile_on = np.abs(F).reshape(nb, 32, nb, 32).max(axis=(1, 3)) > 0
    read = np.kron(tile_on | np.eye(nb, dtype=bool), np.ones((32, 32), bool)) if not lay["l_packed"] else np.ones((nS, nS), bool)
    read &= np.tril(np.ones((nS, nS), bool))
    res = dict(S=sr.ratio(np.where(read, S - sr.to_window(red["S"].astype(np.float64), lay), 0), tS),
               r=sr.ratio(r - sr.to_window(red["r"].astype(np.float64), lay), tr))
    check_bpose(bpose_from or cap, w, name, ref, va, res)
    print("\n  %s (window %d of %d, nS %d, schur path %d): error / bound: %s"
          % (name, w, len(cap.probs), nS, schur, " ".join("%s %.3g" % kv for kv in res.items())))
    for key, v in res.items():
        assert v <= 1.0, (name, key, v, res)


def _check_walk_tables(cap, w, name):
    """the counts this file computes are the ranges the diagonal walk runs over (window 0 of a batch: the tables start at 0)"""
    assert w == 0
    p = cap.probs[w]
    nf = p.n_kf_free
    seg = sum(np.diff(cap.buf(tab, 0, nf + 1, np.int32)) for tab in (b"KFSEG", b"REFSEG", b"PREFBEG"))
    assert np.array_equal(seg, walk_items(p)), (name, seg.tolist(), walk_items(p).tolist())


def _run(names, split, schur):
    W, _ = windows()
    cap = Capture([W[n] for n in names], split)
    try:
        if len(names) == 1:
            _check_walk_tables(cap, 0, names[0])
        for w, n in enumerate(names):
            check_window(cap, w, n, schur)
    finally:
        cap.close()


# ---- cases: schur path ids as vba_debug_window_layout reports them (0 k_schur_all_w, 1 k_schur_all, 2 / 3 the split kernels) ----------
@gpu
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("name", KINDS)
def test_one_window(name, split):
    _run((name,), split, 2 if split else 0)


@gpu
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("names", [BATCH8, BATCH9], ids=["batch8", "batch9"])
def test_ragged_batch(names, split):
    _run(names, split, 3 if split else 1)


@gpu
def test_prv_xyz_levenberg_marquardt():
    """k_schur_diag3 with hd_pass 1 (opens the outer iteration: b_p, H_pp diagonal) and 0 (the trial: S, rhs)"""
    p = synth.make_window(abi.VARIANT_PRV_XYZ, algo=abi.ALGO_LM, n_kf=6, n_fixed=1, n_pt=150, n_obs=600, seed=320)
    cap, first = Capture([p], 0), Capture([p], 0, stop_after=0)   # `first`: only the pass that opens outer iteration 0 has run
    try:
        # (the same upload of the same window: the state the captured iteration started from; var_act is compared in check_bpose)
        assert first.lays[0]["vpos"].tolist() == cap.lays[0]["vpos"].tolist()
        check_window(cap, 0, "prv_xyz_lm", 4, bpose_from=first)
    finally:
        cap.close()
        first.close()
