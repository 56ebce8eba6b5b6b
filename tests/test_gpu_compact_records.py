"""The 48-byte inverse-depth slot and edge records and the per-landmark (sqrt(Dinv), beta) array, on the smallest windows where their
addressing can go wrong: whole solves against the CPU oracle (the bars of tests/test_gpu_parity.py) and against each other.

Windows: 3 and 5 free keyframes, 50..60 landmarks, 150..241 edges.  The first windows of the ragged batch of nine have an odd
n_obs + n_pt, so the slot records of every later window start at an odd record index: at 48 bytes per record no longer a multiple of
64 bytes (nor of 32).  Among them (asserted on the host, the first against the oracle's outlier bitmap):
  * a landmark whose edges are all outliers in stage 2: D = 0, sqrt(Dinv) = 0 -- the update skips it on the 16 bytes of lm_sd;
  * landmarks with a fixed reference keyframe (their reference record holds U = 0);
  * a keyframe outside the active set (no edge, no landmark, no IMU factor);
  * a keyframe that is nobody's reference (its diagonal walk has slot records only), and in every window keyframes that are.

Four runs of the nine windows: the batch through k_schur_all and through the split k_schur_diag + k_schur_off (16 lanes per pair),
and the same windows in two ragged sub-batches of five and four through the few-window k_schur_all_w and its split twin
k_schur_diag + k_schur_off_w (64 lanes per pair).  Fused and split kernels of one regime walk the same items in the same order: equal
bit for bit.  The two regimes deal the items of an off-diagonal pair to 16 or to 64 lanes and so add them in another (fixed) order:
they agree to rounding, with the bars tests/test_gpu_parity.py sets between chunkings that change the kernels (chi2 1e-10 relative,
states 1e-9; measured on MI355X, with these records and with the 64-byte ones before them: chi2 <= 7e-15, states <= 4e-14, none of
the nine windows equal bit for bit).  Every run meets the oracle's bars.

Position in the batch: a window's results must not depend on where its records start.  The last window of the nine (records at an odd
index) equals, bit for bit, the same window as the first of another batch of nine (records at 0); alone it equals, bit for bit, the
last window of a ragged sub-batch of four; and across the regimes it agrees to rounding as above."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import plan_cases
from mc_slam_amd import abi, synth, backend
from test_gpu_parity import _check

gpu = pytest.mark.gpu


def _idp(**kw):
    return synth.make_window(abi.VARIANT_PRV_IDP, **kw)


def _subset(p, keep_obs, keep_pt):
    """p without the edges keep_obs drops and without the landmarks keep_pt drops or that are left with no edge (valid CSR)"""
    beg = np.asarray(p.pt_obs_begin, np.int64)
    pid = np.repeat(np.arange(p.n_pt), np.diff(beg))
    keep_obs = np.asarray(keep_obs, bool) & np.asarray(keep_pt, bool)[pid]
    cnt = np.bincount(pid[keep_obs], minlength=p.n_pt)
    kp = cnt > 0
    return dataclasses.replace(p, pt=p.pt[kp].copy(), pt_ref_kf=p.pt_ref_kf[kp].copy(),
                               pt_obs_begin=np.concatenate([[0], np.cumsum(cnt[kp])]), obs_kf=p.obs_kf[keep_obs].copy(),
                               obs_uv=p.obs_uv[keep_obs].copy(), obs_w=p.obs_w[keep_obs].copy(), kf_pose=p.kf_pose.copy(),
                               kf_vel=p.kf_vel.copy(), kf_bias=p.kf_bias.copy(), truth={})


INACTIVE_KF = 4   # of window "inactive": the newest keyframe, so that the IMU chain of the others stays whole (a gap in the middle
                  # leaves the velocities and biases behind it to one factor: numerically singular, no comparison with the oracle)


def _inactive_keyframe(p, kf):
    """keyframe kf without an IMU factor, an edge or a landmark of its own: outside the active set"""
    keep = (p.imu_kf_i != kf) & (p.imu_kf_j != kf)
    p = dataclasses.replace(p, imu_kf_i=p.imu_kf_i[keep].copy(), imu_kf_j=p.imu_kf_j[keep].copy(),
                            imu_meas=p.imu_meas[keep].copy(), imu_info_prv=p.imu_info_prv[keep].copy(), truth={})
    return _subset(p, p.obs_kf != kf, np.asarray(p.pt_ref_kf) != kf)


DEAD_LM = 7   # the landmark of window "dead" whose edges all become outliers


def _dead_landmark(p, lm):
    """every edge of landmark lm moved 60..90 pixels off, each in its own direction: no inverse depth along the bearing fits two
    of them, so the outlier pass between the stages removes them all"""
    q = p.copy()
    q.obs_uv = p.obs_uv.copy()
    o0, o1 = int(p.pt_obs_begin[lm]), int(p.pt_obs_begin[lm + 1])
    assert o1 - o0 >= 3
    rng = np.random.default_rng(5)
    ang = rng.uniform(0, 2 * np.pi) + 2 * np.pi * np.arange(o1 - o0) / (o1 - o0)
    q.obs_uv[o0:o1] += (rng.uniform(60, 90, o1 - o0) * np.array([np.cos(ang), np.sin(ang)])).T
    return q


@functools.lru_cache(maxsize=None)
def windows():
    """name -> window (built once, never changed: every upload copies)"""
    return dict(odd3=_idp(n_kf=6, n_fixed=3, n_pt=59, n_obs=150, seed=501),     # 3 free keyframes, n_obs + n_pt = 209
                odd5=_idp(n_kf=6, n_fixed=1, n_pt=53, n_obs=192, seed=502),     # 5 free, 245
                dead=_dead_landmark(_idp(n_kf=6, n_fixed=1, n_pt=60, n_obs=241, seed=503), DEAD_LM),   # 5 free, 301
                inactive=_inactive_keyframe(_idp(n_kf=6, n_fixed=1, n_pt=60, n_obs=230, seed=504), INACTIVE_KF),
                free3=_idp(n_kf=5, n_fixed=2, n_pt=60, n_obs=151, seed=505),
                free5=_idp(n_kf=7, n_fixed=2, n_pt=60, n_obs=240, seed=506),
                last=_idp(n_kf=6, n_fixed=1, n_pt=50, n_obs=175, seed=507))


BATCH9 = ("odd3", "odd5", "dead", "inactive", "free3", "odd5", "free5", "odd3", "last")
SUB = (slice(0, 5), slice(5, 9))   # the few-window regime: ragged sub-batches of five and four windows


@functools.lru_cache(maxsize=None)
def oracle_solution(name):
    import oracle_lib
    return oracle_lib.solve(windows()[name])


def test_the_windows_are_what_they_claim():
    """(no GPU) sizes, the odd record bases, and the special landmarks and keyframes -- the dead landmark against the oracle"""
    W = windows()
    for name, p in W.items():
        assert p.n_kf_free in (3, 5) and 30 <= p.n_pt <= 60 and 150 <= p.n_obs <= 400, (name, p.n_kf_free, p.n_pt, p.n_obs)
    base = np.cumsum([0] + [W[n].n_obs + W[n].n_pt for n in BATCH9])   # first slot record of every window of the batch
    assert all((W[n].n_obs + W[n].n_pt) % 2 == 1 for n in BATCH9[:3]), base.tolist()
    assert (base[1:9] * 48 % 64 != 0).all() and base[8] % 2 == 1, base.tolist()   # (the last window is also solved alone)
    for sl in SUB:                                                     # and inside the sub-batches
        b = np.cumsum([0] + [W[n].n_obs + W[n].n_pt for n in BATCH9[sl]])
        assert (b[1:-1] * 48 % 64 != 0).any()
    for name, p in W.items():
        ref = np.asarray(p.pt_ref_kf)
        assert (ref >= p.n_kf_free).any(), name                       # landmarks with a fixed reference keyframe
        used = np.bincount(ref, minlength=p.n_kf)[:p.n_kf_free]
        seen = np.bincount(p.obs_kf, minlength=p.n_kf)[:p.n_kf_free]
        assert ((used == 0) & (seen > 0)).any() and (used > 0).any(), (name, used.tolist())   # nobody's reference / somebody's
    p = W["inactive"]
    assert not (p.obs_kf == INACTIVE_KF).any() and not (np.asarray(p.pt_ref_kf) == INACTIVE_KF).any()
    assert not ((p.imu_kf_i == INACTIVE_KF) | (p.imu_kf_j == INACTIVE_KF)).any() and p.n_imu == 4
    p = W["dead"]
    qo, ro = oracle_solution("dead")
    o0, o1 = int(p.pt_obs_begin[DEAD_LM]), int(p.pt_obs_begin[DEAD_LM + 1])
    assert ro.status == 0 and ro.its_done[1] >= 1 and ro.obs_outlier[o0:o1].all()   # all outliers when stage 2 runs: D = 0 there
    assert ro.obs_outlier.sum() < p.n_obs // 4


# ---- runs ------------------------------------------------------------------------------------------------------------------------
def _solve(probs, split):
    """upload + run + download on a fresh handle of the hooks flavour; returns [(problem, result)] and the Schur path of the run"""
    ba = backend.LocalBA(0, hooks=True)
    try:
        lib = ba.lib
        lib.vba_debug_set_path.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
        lib.vba_debug_plan.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64]
        assert lib.vba_debug_set_path(ba.h, b"schur_split", 1 if split else 0) == 0
        ba.upload(list(probs)); ba.run()
        qs, rs = ba.download()
        plan = np.zeros(len(plan_cases.FIELDS), np.int64)
        assert lib.vba_debug_plan(ba.h, plan.ctypes.data_as(C.POINTER(C.c_int64)), len(plan)) == 0
        return [(q.copy(), r) for q, r in zip(qs, rs)], int(plan[plan_cases.FIELDS.index("schur")])
    finally:
        ba.close()


@functools.lru_cache(maxsize=None)
def runs():
    """the nine windows through the four Schur paths (computed once, shared by the tests)"""
    W = windows()
    ps = [W[n] for n in BATCH9]
    out = {}
    for split in (0, 1):
        out["batch", split], path = _solve(ps, split)
        assert path == (plan_cases.SCHUR_SPLIT if split else plan_cases.SCHUR_ALL), path
        few = []
        for sl in SUB:
            got, path = _solve(ps[sl], split)
            assert path == (plan_cases.SCHUR_SPLIT_W if split else plan_cases.SCHUR_ALL_W), path
            few += got
        out["few", split] = few
    return out


def _same_bits(a, b):
    (qa, ra), (qb, rb) = a, b
    assert ra.status == rb.status == 0 and ra.its_done == rb.its_done
    assert np.array_equal(ra.obs_outlier, rb.obs_outlier) and np.array_equal(ra.obs_chi2, rb.obs_chi2)
    assert ra.chi2_vis == rb.chi2_vis and ra.chi2_prv == rb.chi2_prv and ra.chi2_bias == rb.chi2_bias
    assert np.array_equal(np.asarray(ra.chi2_trace), np.asarray(rb.chi2_trace))
    for f in ("kf_pose", "kf_vel", "kf_bias", "pt"):
        assert np.array_equal(getattr(qa, f), getattr(qb, f)), f


def _same_to_rounding(a, b):
    """two regimes of kernels (another fixed order of the sums): the bars of test_batch_solve_streams_fresh_windows_like_upload_run_download"""
    (qa, ra), (qb, rb) = a, b
    assert ra.status == rb.status == 0 and ra.its_done == rb.its_done and np.array_equal(ra.obs_outlier, rb.obs_outlier)
    d = dict(chi2=abs(ra.chi2_vis - rb.chi2_vis) / ra.chi2_vis, pose=np.abs(qa.kf_pose - qb.kf_pose).max(), pt=np.abs(qa.pt - qb.pt).max())
    print("  across the regimes: chi2 %.3g relative, poses %.3g, landmarks %.3g" % (d["chi2"], d["pose"], d["pt"]))
    assert d["chi2"] <= 1e-10 and d["pose"] < 1e-9 and d["pt"] < 1e-9, d


@gpu
@pytest.mark.parametrize("regime", ["batch", "few"])
def test_fused_and_split_schur_kernels_agree_bit_for_bit(regime):
    R = runs()
    for w in range(len(BATCH9)):
        _same_bits(R[regime, 0][w], R[regime, 1][w])


@gpu
def test_many_window_and_few_window_kernels_agree():
    R = runs()
    bitwise = 0
    for w in range(len(BATCH9)):
        _same_to_rounding(R["batch", 0][w], R["few", 0][w])
        bitwise += all(np.array_equal(getattr(R["batch", 0][w][0], f), getattr(R["few", 0][w][0], f)) for f in ("kf_pose", "pt"))
    print("  windows equal bit for bit across the regimes: %d of %d" % (bitwise, len(BATCH9)))


@gpu
@pytest.mark.parametrize("key", [("batch", 0), ("few", 0), ("batch", 1)], ids=["k_schur_all", "k_schur_all_w", "split"])
def test_every_path_matches_the_oracle(key):
    R, W = runs(), windows()
    for w, name in enumerate(BATCH9):
        q, r = R[key][w]
        qo, ro = oracle_solution(name)
        _check(W[name], q, r, qo, ro)
    # the dead landmark was not moved by stage 2 (sqrt(Dinv) = 0: the update leaves it alone); the oracle agrees (_check)
    w = BATCH9.index("dead")
    o0, o1 = int(W["dead"].pt_obs_begin[DEAD_LM]), int(W["dead"].pt_obs_begin[DEAD_LM + 1])
    assert R[key][w][1].obs_outlier[o0:o1].all()


@gpu
def test_a_window_does_not_depend_on_where_its_records_start():
    R, W = runs(), windows()
    last = W["last"]
    # many-window kernels: records at an odd index (last of the nine) / at 0 (first of another nine)
    first_of_nine, path = _solve([last] + [W[n] for n in BATCH9[:8]], 0)
    assert path == plan_cases.SCHUR_ALL
    _same_bits(R["batch", 0][8], first_of_nine[0])
    # few-window kernels: alone / last of the ragged sub-batch of four
    alone, path = _solve([last], 0)
    assert path == plan_cases.SCHUR_ALL_W
    _same_bits(alone[0], R["few", 0][8])
    # and across the regimes
    _same_to_rounding(alone[0], R["batch", 0][8])
    qo, ro = oracle_solution("last")
    _check(last, alone[0][0], alone[0][1], qo, ro)
