"""The host halves of vba_sim3_optimize and vba_pose_optimize (mc_slam_amd/csrc/vba_host_sim3.h, vba_host_pose.h, vba_host_arena.h:
refusals, arena offsets, packing, write-back, inverse_host) under AddressSanitizer + UBSan (CPU only).  The harness
(tests/host_small_check.cpp) packs into heap blocks of exactly the arena's sizes; every expected offset below is restated from the
sizes alone, and the packed regions are compared with the interleaving done in NumPy through an order-sensitive checksum."""
import numpy as np
import pytest

from mc_slam_amd import abi, synth
import host_check_lib as hc
from host_check_lib import checksum, up

SIM3_DESC = np.dtype([("i", "<i4", 6), ("pair0", "<i8"), ("S", "<f8", 8), ("K1", "<f8", 4), ("K2", "<f8", 4), ("th2", "<f8"), ("huber", "<f8")])
SIM3_OUT, FRAME_DESC, FRAME_OUT = 112, 32 + 8 * (3 * 22 + 19 + 61 + 81 + 225 + 6), 32 + 8 * (4 + 22 + 225)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return hc.build(tmp_path_factory, "host_small_check", pthread=True)


# ---------------------------------------------------------------------------------------------------------------- sim3
def _write_sim3(path, items):
    """items: (problem, dict of n_pairs / nulls / want_chi2 overrides)"""
    with open(path, "wb") as f:
        f.write(np.array([len(items)], dtype="<i4").tobytes())
        for p, o in items:
            f.write(np.array([o.get("n_pairs", p.n_pairs), p.n_pairs, p.fix_scale, p.its_stage1, p.its_stage2_bad, p.its_stage2_clean, p.min_inliers,
                              o.get("nulls", 0), o.get("want_chi2", 1)], dtype="<i4").tobytes())
            f.write(np.concatenate([p.S12, p.K1, p.K2, [p.th2, p.huber]]).astype("<f8").tobytes())
            for a in (p.p1c, p.p2c, p.uv1, p.uv2, p.w1, p.w2):
                f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())


def _sim3_batch(counts, seed0):
    return [synth.make_sim3_pair(seed0 + k, n, fix_scale=bool(k % 2)) for k, n in enumerate(counts)]


SIM3_SHAPES = [[0], [1], [7, 0, 33], [64, 65], [3 + k % 5 for k in range(300)]]     # 300 items: beyond the threaded-packing threshold (256)


@pytest.mark.parametrize("want_chi2", [1, 0])
def test_sim3_offsets_packing_and_write_back(checker, tmp_path, want_chi2):
    batches = [_sim3_batch(c, 100 * k) for k, c in enumerate(SIM3_SHAPES)]
    files = []
    for k, ps in enumerate(batches):
        files.append(str(tmp_path / ("b%d.s3" % k)))
        _write_sim3(files[-1], [(p, dict(want_chi2=want_chi2)) for p in ps])
    for ps, line in zip(batches, hc.run(checker, ["sim3"] + files, len(files))):
        f = hc.fields(line)
        n, n_tot = len(ps), sum(p.n_pairs for p in ps)
        # today's formulas: [desc | p | uv | w] up, [out | flag | c] back, no device-only region
        sizes = [up(SIM3_DESC.itemsize * n), up((6 * n_tot + 6) * 8), up((4 * n_tot + 4) * 8), up((2 * n_tot + 2) * 8),
                 up(SIM3_OUT * n), up(n_tot + 1), up((2 * n_tot + 2) * 8)]
        offs = np.concatenate([[0], np.cumsum(sizes)])
        assert [f[k] for k in ("desc", "p", "uv", "w", "out", "flag", "c")] == offs[:7].tolist()
        hc.assert_bound(f, [(k, k) for k in ("desc", "out", "p", "uv", "w", "c", "flag")])                 # Sim3Batch reads every region where it is
        assert (f["n_tot"], f["want_chi2"], f["upload"], f["back"], f["total"]) == (n_tot, want_chi2, offs[4], offs[7] - offs[4], offs[7])
        assert f["download"] == (offs[7] if want_chi2 else offs[6]) - offs[4]         # chi2 comes back only when a caller asked for it
        d = np.zeros(n, dtype=SIM3_DESC)
        pair0 = np.concatenate([[0], np.cumsum([p.n_pairs for p in ps])])
        for k, p in enumerate(ps):
            d[k] = ((p.n_pairs, p.fix_scale, p.its_stage1, p.its_stage2_bad, p.its_stage2_clean, p.min_inliers), pair0[k], p.S12, p.K1, p.K2, p.th2, p.huber)
        assert f["sum_desc"] == checksum(d)
        assert f["sum_p"] == checksum(*[np.hstack([p.p1c, p.p2c]) for p in ps])
        assert f["sum_uv"] == checksum(*[np.hstack([p.uv1, p.uv2]) for p in ps])
        assert f["sum_w"] == checksum(*[np.stack([p.w1, p.w2], axis=1) for p in ps])
        # the write-back of a synthetic result: record k says k, pair i of the call is flagged when i is odd, chi2 = (2 i, 2 i + 1)
        i = np.arange(n_tot)
        assert f["got_inliers"] == n * (n - 1) // 2 and f["got_S7"] == sum(k + 7 for k in range(n))
        assert f["got_flag"] == int((i & 1).sum())
        assert (f["got_chi12"], f["got_chi21"]) == ((int((2 * i).sum()), int((2 * i + 1).sum())) if want_chi2 else (0, 0))


def test_sim3_refusals_carry_todays_messages(checker, tmp_path):
    p = synth.make_sim3_pair(6, 20)
    good = (p, {})
    cases = [((p, dict(n_pairs=-1)), "negative n_pairs"),
             ((p, dict(nulls=1)), "NULL array with n_pairs > 0"),
             ((p, dict(nulls=2)), "NULL array with n_pairs > 0"),
             ((p, dict(nulls=4)), "NULL problem or result"),
             ((p.copy(S12=np.r_[np.nan, p.S12[1:]]), {}), "S12 is not finite"),
             ((p.copy(S12=np.r_[p.S12[:7], np.inf]), {}), "S12 is not finite"),
             ((p.copy(S12=np.r_[p.S12[:3], 0, 0, 0, 0, 1.0]), {}), "zero quaternion in S12"),
             ((p.copy(S12=np.r_[p.S12[:7], 0.0]), {}), "scale of S12 is not positive"),
             ((p.copy(S12=np.r_[p.S12[:7], -1.0]), {}), "scale of S12 is not positive"),
             ((p.copy(its_stage1=0), {}), "iteration budgets must be at least 1"),
             ((p.copy(its_stage2_bad=0), {}), "iteration budgets must be at least 1"),
             ((p.copy(its_stage2_clean=-3), {}), "iteration budgets must be at least 1"),
             ((p.copy(min_inliers=-1), {}), "negative min_inliers"),
             ((p.copy(th2=np.nan), {}), "th2 / huber are not usable"),
             ((p.copy(huber=0.0), {}), "th2 / huber are not usable"),
             ((p.copy(huber=np.inf), {}), "th2 / huber are not usable")]
    files = []
    for k, (bad, _) in enumerate(cases):
        files.append(str(tmp_path / ("r%d.s3" % k)))
        _write_sim3(files[-1], [good, bad])
    for (_, msg), line in zip(cases, hc.run(checker, ["sim3"] + files, len(files))):
        assert line == "error problem 1: " + msg
    # a NULL array is no refusal while n_pairs is 0; scale before quaternion, as the entry point orders them
    q = synth.make_sim3_pair(7, 0)
    _write_sim3(files[0], [(q, dict(nulls=1)), (p.copy(S12=np.r_[p.S12[:3], 0, 0, 0, 0, 0.0]), {})])
    assert hc.run(checker, ["sim3"] + files[:1], 1) == ["error problem 1: scale of S12 is not positive"]
    raw = open(files[1], "rb").read()
    open(files[1], "wb").write(raw[:len(raw) // 2])                                   # a truncated file: refused by the reader
    assert hc.run(checker, ["sim3"] + files[1:2], 1) == ["error load"]


# ---------------------------------------------------------------------------------------------------------------- pose
def _write_pose(path, items):
    """items: (frame, dict of kind / n_obs / n_obs_last / nulls overrides)"""
    with open(path, "wb") as f:
        f.write(np.array([len(items)], dtype="<i4").tobytes())
        for p, o in items:
            f.write(np.array([o.get("kind", p.last_is_frame), p.compute_marg, o.get("n_obs", p.n_obs), o.get("n_obs_last", p.n_obs_last), p.n_obs,
                              p.n_obs_last, o.get("nulls", 0)], dtype="<i4").tobytes())
            s = p.as_struct()
            for a in (p.nav, p.nav_last, p.K, p.T_cb, p.g_w, p.imu_meas, p.imu_cov_pvphi, p.prior_nav, p.prior_info, [s.inv_bg_rw2, s.inv_ba_rw2],
                      p.obs_pw, p.obs_uv, p.obs_w, p.last_pw, p.last_uv, p.last_w):
                f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())


@pytest.fixture(scope="module")
def frames():
    """the frame generator of tests/test_gpu_pose.py, one frame of each kind"""
    return {abi_kind: f for abi_kind, f in ((0, synth.make_frame(seed=51, n_obs=40)), (1, synth.make_frame(seed=52, n_obs=40, last_is_frame=True)),
                                            (2, synth.make_frame_vision(seed=53, n_obs=40)))}


def _cut(f, n_obs, n_last=0):
    """the frame with its first n_obs observations (and n_last of the last frame)"""
    import copy
    assert f.n_obs >= n_obs and f.n_obs_last >= n_last
    g = copy.copy(f)
    g.obs_pw, g.obs_uv, g.obs_w = f.obs_pw[:n_obs].copy(), f.obs_uv[:n_obs].copy(), f.obs_w[:n_obs].copy()
    g.last_pw, g.last_uv, g.last_w = f.last_pw[:n_last].copy(), f.last_uv[:n_last].copy(), f.last_w[:n_last].copy()
    return g


def _pose_batches(frames):
    every = [_cut(frames[kind], n, n_last if kind == 1 else 0) for n in (0, 1, 31) for kind in (0, 1, 2) for n_last in ((0, 5) if kind == 1 else (0,))]
    return [every, [_cut(frames[1], 31, 5)], [_cut(frames[1], 0, 0)], [_cut(frames[k % 3], k % 4, (k % 3) if k % 3 == 1 else 0) for k in range(300)]]


def test_pose_offsets_packing_and_write_back(checker, tmp_path, frames):
    batches = _pose_batches(frames)
    files = []
    for k, fs in enumerate(batches):
        files.append(str(tmp_path / ("b%d.fr" % k)))
        _write_pose(files[-1], [(f, {}) for f in fs])
    hub = [float(np.float32(np.sqrt(x))) for x in (30.5779, 21.666, 16.812, 5.991)]
    for fs, line in zip(batches, hc.run(checker, ["pose"] + files, len(files))):
        f = hc.fields(line, floats=("info_err",))
        n = len(fs)
        n_last = [g.n_obs_last if g.last_is_frame == 1 else 0 for g in fs]
        n_tot = sum(g.n_obs for g in fs) + sum(n_last)
        # today's formulas: [desc | pw | uv | w] up, [out | lvl] back, err stays on the device
        sizes = [up(FRAME_DESC * n), up((3 * n_tot + 3) * 8), up((2 * n_tot + 2) * 8), up((n_tot + 1) * 8), up(FRAME_OUT * n), up(n_tot + 1), up((2 * n_tot + 2) * 8)]
        offs = np.concatenate([[0], np.cumsum(sizes)])
        assert [f[k] for k in ("desc", "pw", "uv", "w", "out", "lvl", "err")] == offs[:7].tolist()
        hc.assert_bound(f, [(k, k) for k in ("desc", "out", "pw", "uv", "w", "err", "lvl")])             # PoseBatch reads every region where it is
        assert f["n_frames"] == n
        assert (f["n_tot"], f["upload"], f["back"], f["total"]) == (n_tot, offs[4], offs[6] - offs[4], offs[7])
        # a frame's observations, then its last frame's
        assert f["sum_pw"] == checksum(*[a for g, nl in zip(fs, n_last) for a in (g.obs_pw, g.last_pw[:nl])])
        assert f["sum_uv"] == checksum(*[a for g, nl in zip(fs, n_last) for a in (g.obs_uv, g.last_uv[:nl])])
        assert f["sum_w"] == checksum(*[a for g, nl in zip(fs, n_last) for a in (g.obs_w, g.last_w[:nl])])
        s_int, s_val, o = 0, 0, 0
        for k, (g, nl) in enumerate(zip(fs, n_last)):
            iv = [g.last_is_frame, 1 if g.compute_marg else 0, g.n_obs, nl, o, o + g.n_obs, 0, 0]
            o += g.n_obs + nl
            s_int += sum((8 * k + q + 1) * v for q, v in enumerate(iv))
            s = g.as_struct()
            s_val += (k + 1) * checksum(g.nav, g.nav_last, g.prior_nav, g.K, g.T_cb[:3], g.g_w, g.imu_meas, g.prior_info,
                                        np.array([s.inv_bg_rw2, s.inv_ba_rw2] + hub))
        assert f["sum_int"] == s_int % 2 ** 64 and f["sum_val"] == s_val % 2 ** 64
        # info_pvr * cov = I: 1e-12 relative for the inverse (test_inverse_host) times the condition of these covariances
        cond = max(np.linalg.cond(g.imu_cov_pvphi) for g in fs)
        print("info_err %.3g cond %.3g" % (f["info_err"], cond))
        assert f["info_err"] <= 1e-12 * cond
        i = np.arange(n_tot)
        assert f["got_inliers"] == n * (n - 1) // 2 and f["got_nav21"] == sum(k + 21 for k in range(n))
        lvl, o, got_o, got_l = (i & 1), 0, 0, 0
        for g, nl in zip(fs, n_last):
            got_o += int(lvl[o:o + g.n_obs].sum()); o += g.n_obs
            got_l += int(lvl[o:o + nl].sum()); o += nl
        assert (f["got_outlier"], f["got_outlier_last"]) == (got_o, got_l)


def test_pose_refusals_carry_todays_messages(checker, tmp_path, frames):
    kf, fr = _cut(frames[0], 31), _cut(frames[1], 31, 5)
    zero, nan = _cut(frames[0], 31), _cut(frames[1], 31, 5)
    zero.imu_cov_pvphi = np.zeros((9, 9))
    nan.imu_cov_pvphi = frames[1].imu_cov_pvphi.copy()
    nan.imu_cov_pvphi[4, 4] = np.nan
    cases = [((kf, dict(n_obs=-1)), "bad frame"), ((kf, dict(nulls=1)), "bad frame"), ((kf, dict(nulls=4)), "bad frame"), ((kf, dict(nulls=8)), "bad frame"),
             ((kf, dict(kind=3)), "unknown frame kind"), ((kf, dict(kind=-1)), "unknown frame kind"),
             ((fr, dict(n_obs_last=-5)), "negative n_obs_last"), ((fr, dict(nulls=2)), "bad last frame"),
             ((zero, {}), "imu_cov_pvphi is singular or not finite"), ((nan, {}), "imu_cov_pvphi is singular or not finite")]
    files = []
    for k, (bad, _) in enumerate(cases):
        files.append(str(tmp_path / ("r%d.fr" % k)))
        _write_pose(files[-1], [(fr, {}), bad])
    for (_, msg), line in zip(cases, hc.run(checker, ["pose"] + files, len(files))):
        assert line == "error " + msg
    # what is no refusal: a negative n_obs_last and NULL last arrays where no last frame is read, a singular covariance in a vision-only frame
    vis = _cut(frames[2], 31)
    vis.imu_cov_pvphi = np.zeros((9, 9))
    _write_pose(files[0], [(kf, dict(n_obs_last=-5, nulls=2)), (vis, {}), (_cut(frames[1], 0, 0), dict(nulls=1 | 2))])
    assert hc.fields(hc.run(checker, ["pose"] + files[:1], 1)[0], floats=("info_err",))["n_tot"] == 62


# ------------------------------------------------------------------------------------------------------------- inverse
def test_inverse_host(checker, tmp_path):
    r = np.random.default_rng(9)
    Q, _ = np.linalg.qr(r.normal(size=(9, 9)))
    A = Q @ np.diag(np.linspace(1.0, 50.0, 9)) @ Q.T                    # SPD, condition 50
    A = (A + A.T) / 2
    sing = A.copy(); sing[:, 3] = 0; sing[3, :] = 0
    nan = A.copy(); nan[2, 5] = np.nan
    inf = A.copy(); inf[0, 0] = np.inf
    mats = [A, np.zeros((9, 9)), sing, nan, inf, np.eye(15)]
    files = []
    for k, M in enumerate(mats):
        files.append(str(tmp_path / ("m%d.bin" % k)))
        open(files[-1], "wb").write(np.array([len(M)], dtype="<i4").tobytes() + M.astype("<f8").tobytes())
    lines = hc.run(checker, ["inverse"] + files, len(files))
    got = np.array(lines[0].split()[1:], dtype=float).reshape(9, 9)
    want = np.linalg.inv(A)
    err = np.abs(got - want).max() / np.abs(want).max()
    print("inverse_host vs numpy.linalg.inv: %.2e relative" % err)
    assert lines[0].startswith("ok ") and err <= 1e-12
    assert lines[1:5] == ["singular"] * 4
    assert np.array_equal(np.array(lines[5].split()[1:], dtype=float).reshape(15, 15), np.eye(15))
