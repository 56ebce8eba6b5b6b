"""Synthetic EuRoC-calibrated local-BA windows.

No EuRoC data exists in the build environment, so "EuRoC-derived" means: EuRoC camera intrinsics and
camera-IMU extrinsic (config/euroc.yaml:40-44,54-57), 200 Hz IMU / 4 Hz keyframes, the reference's IMU
noise constants (src/IMU/imudata.cpp:25-31), ORB scale-pyramid weights (1/1.2^(2*octave)) and the
reference's own preintegration recursion (src/IMU/IMUPreintegrator.cpp:63-112, restated here in numpy so
that input synthesis never touches oracle/).

The ground-truth trajectory is DEFINED as the discrete integration of the noise-free IMU signal with the
reference's update rule, so noise-free preintegrated factors have exactly zero residual at ground truth.
"""
import numpy as np

from . import abi

EUROC_K = np.array([458.654, 457.296, 367.215, 248.375])
EUROC_WH = (752.0, 480.0)
EUROC_TBC = np.array([
    [0.0148655429818, -0.999880929698, 0.00414029679422, -0.0216401454975],
    [0.999557249008, 0.0149672133247, 0.025715529948, -0.064676986768],
    [-0.0257744366974, 0.00375618835797, 0.999660727178, 0.00981073058949],
    [0.0, 0.0, 0.0, 1.0]])
GRAVITY = 9.810  # src/IMU/configparam.cpp:6


# ---------------------------------------------------------------- small Lie helpers (batched numpy)
def hat(v):
    v = np.asarray(v, dtype=np.float64)
    M = np.zeros(v.shape[:-1] + (3, 3))
    M[..., 0, 1], M[..., 0, 2] = -v[..., 2], v[..., 1]
    M[..., 1, 0], M[..., 1, 2] = v[..., 2], -v[..., 0]
    M[..., 2, 0], M[..., 2, 1] = -v[..., 1], v[..., 0]
    return M


def so3_exp(w):
    """Rodrigues, batched: (...,3) -> (...,3,3)."""
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    W = hat(w)
    W2 = W @ W
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th * th / 6.0, np.sin(ths) / ths)
    b = np.where(small, 0.5 - th * th / 24.0, (1 - np.cos(ths)) / (ths * ths))
    return np.eye(3) + a * W + b * W2


def so3_jr(w):
    """Right Jacobian, the reference's formula (src/IMU/so3.cpp:33-50), batched."""
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    small = th < 0.00001
    ths = np.where(small, 1.0, th)
    K = hat(w) / ths
    J = np.eye(3) - (1 - np.cos(ths)) / ths * K + (1 - np.sin(ths) / ths) * (K @ K)
    return np.where(small, np.eye(3), J)


def rot_to_quat(R):
    """3x3 -> (x,y,z,w), w >= 0, unit."""
    R = np.asarray(R, dtype=np.float64)
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = np.zeros(4)
        q[i] = 0.25 * s
        q[3] = (R[k, j] - R[j, k]) / s
        q[j] = (R[j, i] + R[i, j]) / s
        q[k] = (R[k, i] + R[i, k]) / s
    if q[3] < 0:
        q = -q
    return q / np.linalg.norm(q)


def quat_to_rot(q):
    x, y, z, w = q
    return np.array([
        [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _orthonormalise(R):
    return quat_to_rot(rot_to_quat(R))  # as configparam.cpp:55-56


def extrinsics():
    """(R_bc, p_bc, T_cb[7]) from config/euroc.yaml, rotation re-normalised through a quaternion."""
    R_bc = _orthonormalise(EUROC_TBC[:3, :3])
    p_bc = EUROC_TBC[:3, 3].copy()
    R_cb = R_bc.T
    t_cb = -R_cb @ p_bc
    return R_bc, p_bc, np.concatenate([t_cb, rot_to_quat(R_cb)])


# ---------------------------------------------------------------- preintegration (numpy restatement of A15)
def preintegrate(omega, acc, dts):
    """IMUPreintegrator::update applied over samples, batched over E edges.

    omega, acc: [E,S,3] bias-corrected samples, dts: [E,S].  Returns (meas [E,61], cov_PVphi [E,9,9]).
    Follows src/IMU/IMUPreintegrator.cpp:63-112 line by line.
    """
    E, S, _ = omega.shape
    dP = np.zeros((E, 3)); dV = np.zeros((E, 3)); dR = np.tile(np.eye(3), (E, 1, 1))
    JPg = np.zeros((E, 3, 3)); JPa = np.zeros((E, 3, 3)); JVg = np.zeros((E, 3, 3)); JVa = np.zeros((E, 3, 3))
    JRg = np.zeros((E, 3, 3))
    cov = np.zeros((E, 9, 9)); T = np.zeros(E)
    I3 = np.eye(3)
    for s in range(S):
        dt = dts[:, s][:, None, None]
        dt2 = dt * dt
        w, a = omega[:, s], acc[:, s]
        dRk = so3_exp(w * dts[:, s][:, None])
        Jr = so3_jr(w * dts[:, s][:, None])
        RS = dR @ hat(a)
        A = np.tile(np.eye(9), (E, 1, 1))
        A[:, 6:9, 6:9] = np.swapaxes(dRk, 1, 2)
        A[:, 3:6, 6:9] = -RS * dt
        A[:, 0:3, 6:9] = -0.5 * RS * dt2
        A[:, 0:3, 3:6] = I3 * dt
        Bg = np.zeros((E, 9, 3)); Bg[:, 6:9] = Jr * dt
        Ca = np.zeros((E, 9, 3)); Ca[:, 3:6] = dR * dt; Ca[:, 0:3] = 0.5 * dR * dt2
        cov = A @ cov @ np.swapaxes(A, 1, 2) + abi.GYR_MEAS_COV * (Bg @ np.swapaxes(Bg, 1, 2)) \
            + abi.ACC_MEAS_COV * (Ca @ np.swapaxes(Ca, 1, 2))
        RSJ = RS @ JRg
        JPa = JPa + JVa * dt - 0.5 * dR * dt2
        JPg = JPg + JVg * dt - 0.5 * RSJ * dt2
        JVa = JVa - dR * dt
        JVg = JVg - RSJ * dt
        JRg = np.swapaxes(dRk, 1, 2) @ JRg - Jr * dt
        Ra = np.einsum("eij,ej->ei", dR, a)
        dP = dP + dV * dts[:, s][:, None] + 0.5 * Ra * (dts[:, s] ** 2)[:, None]
        dV = dV + Ra * dts[:, s][:, None]
        dR = dR @ dRk
        dR = np.stack([_orthonormalise(dR[e]) for e in range(E)])  # normalizeRotationM, IMUPreintegrator.h:163-174
        T = T + dts[:, s]
    meas = np.concatenate([T[:, None], dP, dV, dR.reshape(E, 9), JPg.reshape(E, 9), JPa.reshape(E, 9),
                           JVg.reshape(E, 9), JVa.reshape(E, 9), JRg.reshape(E, 9)], axis=1)
    return meas, cov


def prv_information(cov_pvphi):
    """inverse of the V/phi-swapped covariance (src/Optimizer.cpp:273-280)."""
    perm = [0, 1, 2, 6, 7, 8, 3, 4, 5]
    c = cov_pvphi[..., perm, :][..., :, perm]
    return np.linalg.inv(c)


# ---------------------------------------------------------------- the generator
def make_window(variant=abi.VARIANT_PRV_IDP, n_kf=50, n_fixed=1, n_pt=5000, n_obs=30000, seed=3,
                kf_dt=0.25, imu_dt=0.005, outlier_frac=0.05, algo=None, noise=True, init_scale=1.0, pix_noise=1.0,
                tracks="nearest", landmark_order="random"):
    """Build one synthetic local-BA window.

    n_kf keyframes in time order t0..; the FIRST n_fixed in time are fixed (the window's predecessor and,
    if n_fixed > 1, older co-observers).  In the returned Problem free keyframes come first (time order),
    fixed ones after.  n_obs counts reprojection EDGES (variant 2: the reference keyframe's own
    observation is not an edge, src/Optimizer.cpp:395-398).  init_scale multiplies the perturbation of the initial
    guess (poses, velocities, depths / points): < 1 = a window that starts close to its optimum.  pix_noise multiplies the
    keypoint noise (1 = one pixel at octave 0, ORB-SLAM's model); the information matrices are not changed, so chi2 scales with
    pix_noise^2 and the absolute |dchi2| < 1e-3 stop of Gauss-Newton is reached after fewer iterations for sharp features.
    tracks: which of the keyframes that see a landmark observe it -- "nearest" = the ones closest in time to the keyframe it was
    created from (tracks are runs of consecutive keyframes: a sliding window), "random" = a random subset of them (tracks with
    gaps, co-visibility scattered over the whole span in which the point is in view: a co-visibility window).
    """
    rng = np.random.default_rng(seed)
    R_bc, p_bc, T_cb = extrinsics()
    R_cb = R_bc.T
    S = int(round(kf_dt / imu_dt))
    n_steps = (n_kf - 1) * S
    t = np.arange(n_steps) * imu_dt

    # gravity: (0,0,-g) rotated by a fixed seed rotation
    g_w = so3_exp(rng.normal(0, 0.3, 3)) @ np.array([0.0, 0.0, -GRAVITY])
    # smooth body-rate and world-acceleration signals (MAV-like: ~1 m/s, ~0.3 rad/s)
    fw = rng.uniform(0.15, 0.6, 3); pw = rng.uniform(0, 2 * np.pi, 3); aw = rng.uniform(0.1, 0.3, 3)
    fa = rng.uniform(0.1, 0.4, 3); pa = rng.uniform(0, 2 * np.pi, 3); aa = np.array([1.0, 1.0, 0.3]) * rng.uniform(0.5, 1.2, 3)
    omega_true = aw * np.sin(2 * np.pi * fw * t[:, None] + pw)
    acc_world = aa * np.sin(2 * np.pi * fa * t[:, None] + pa)
    # discrete ground truth with the reference's integration rule
    R = np.eye(3); V = np.array([1.0, 0.3, 0.0]) * rng.uniform(0.6, 1.2); P = np.zeros(3)
    Rs, Vs, Ps = [R.copy()], [V.copy()], [P.copy()]
    acc_true = np.zeros((n_steps, 3))
    for k in range(n_steps):
        a_b = R.T @ (acc_world[k] - g_w)
        acc_true[k] = a_b
        P = P + V * imu_dt + 0.5 * g_w * imu_dt ** 2 + 0.5 * (R @ a_b) * imu_dt ** 2
        V = V + g_w * imu_dt + (R @ a_b) * imu_dt
        R = _orthonormalise(R @ so3_exp(omega_true[k] * imu_dt))
        if (k + 1) % S == 0:
            Rs.append(R.copy()); Vs.append(V.copy()); Ps.append(P.copy())
    Rs, Vs, Ps = np.array(Rs), np.array(Vs), np.array(Ps)   # time order, n_kf entries

    bg_true = rng.normal(0, 1e-3, 3) if noise else np.zeros(3)
    ba_true = rng.normal(0, 2e-2, 3) if noise else np.zeros(3)
    bg_est = bg_true + (rng.normal(0, 2e-4, 3) if noise else 0)
    ba_est = ba_true + (rng.normal(0, 5e-3, 3) if noise else 0)
    sg = 1.7e-4 / np.sqrt(imu_dt) if noise else 0.0
    sa = 2.0e-3 / np.sqrt(imu_dt) if noise else 0.0
    gyr_meas = omega_true + bg_true + rng.normal(0, 1, omega_true.shape) * sg
    acc_meas = acc_true + ba_true + rng.normal(0, 1, acc_true.shape) * sa

    # camera poses (ground truth): R_cw = (R_wb R_bc)^T, p_wc = R_wb p_bc + p_wb  (src/KeyFrame.cpp:101-106)
    R_wc = Rs @ R_bc
    p_wc = np.einsum("kij,j->ki", Rs, p_bc) + Ps
    fx, fy, cx, cy = EUROC_K
    Wd, Hd = EUROC_WH

    def project(Pw, k):
        Pc = R_wc[k].T @ (Pw - p_wc[k])
        return np.array([fx * Pc[0] / Pc[2] + cx, fy * Pc[1] / Pc[2] + cy]), Pc[2]

    # how many edges each point gets (sum exactly n_obs, each >= 1 for IDP / >= 2 otherwise)
    extra = 1 if variant == abi.VARIANT_PRV_IDP else 0   # the reference KF's own observation
    kmin = 1 if variant == abi.VARIANT_PRV_IDP else 2
    base = n_obs // n_pt
    ks = np.full(n_pt, base, dtype=np.int64)
    ks[: n_obs - base * n_pt] += 1
    jmax = max(0, min(2, base - kmin, n_kf - extra - base - 1))
    if base + (1 if n_obs % n_pt else 0) + extra > n_kf:
        raise ValueError("n_obs/n_pt too large for n_kf keyframes")
    jit = rng.integers(-jmax, jmax + 1, n_pt // 2)
    ks[: 2 * (n_pt // 2): 2] += jit
    ks[1: 2 * (n_pt // 2): 2] -= jit
    rng.shuffle(ks)
    assert ks.sum() == n_obs and ks.min() >= kmin

    R_cw_all = np.swapaxes(R_wc, 1, 2)

    def project_all(Pw):
        """pixel and depth of world point Pw in every keyframe."""
        Pc = np.einsum("kij,kj->ki", R_cw_all, Pw[None, :] - p_wc)
        z = Pc[:, 2]
        zs = np.where(np.abs(z) < 1e-9, 1e-9, z)
        return np.stack([fx * Pc[:, 0] / zs + cx, fy * Pc[:, 1] / zs + cy], axis=1), z

    pts_w = np.zeros((n_pt, 3)); obs_lists = []
    kf_ids = np.arange(n_kf)
    for p in range(n_pt):
        need = int(ks[p]) + extra
        for _try in range(500):
            c = int(rng.integers(0, n_kf))
            u, v = rng.uniform(20, Wd - 20), rng.uniform(20, Hd - 20)
            d = rng.uniform(2.0, 10.0)
            Pw = R_wc[c] @ (np.array([(u - cx) / fx, (v - cy) / fy, 1.0]) * d) + p_wc[c]
            uv, z = project_all(Pw)
            ok = (z > 0.5) & (uv[:, 0] > 5) & (uv[:, 0] < Wd - 5) & (uv[:, 1] > 5) & (uv[:, 1] < Hd - 5)
            cand = kf_ids[ok]
            if cand.size < need:
                continue
            if tracks == "random":
                vis = rng.choice(cand, need, replace=False)
            else:
                vis = cand[np.argsort(np.abs(cand - c), kind="stable")[:need]]
            if (vis >= n_fixed).any():
                break
        else:
            raise RuntimeError("could not place point")
        pts_w[p] = Pw
        obs_lists.append(np.sort(vis))

    # index map: time index -> problem index (free first)
    n_free = n_kf - n_fixed
    tidx = list(range(n_fixed, n_kf)) + list(range(n_fixed))
    pidx = np.zeros(n_kf, dtype=np.int64)
    pidx[tidx] = np.arange(n_kf)

    if landmark_order == "caller":
        # the order the reference's caller hands landmarks over in: lLocalMapPoints is filled keyframe by keyframe over
        # lLocalKeyFrames (oldest first, the current keyframe last), every keyframe appending the map points no earlier one has
        # listed (src/Optimizer.cpp:59-78) -- landmarks come grouped by the FIRST local keyframe that observes them; inside a
        # group the order is the keyframe's feature order (arbitrary: the generation order here)
        key = np.array([min(int(pidx[k]) for k in l if pidx[k] < n_free) for l in obs_lists])
        perm = np.argsort(key, kind="stable")
        pts_w = pts_w[perm]
        obs_lists = [obs_lists[i] for i in perm]
    elif landmark_order != "random":
        raise ValueError("landmark_order: 'random' or 'caller'")

    # observations (vectorised): edge list in point order, ascending keyframe time inside a point
    first = 1 if variant == abi.VARIANT_PRV_IDP else 0
    e_pt = np.concatenate([np.full(len(l) - first, p) for p, l in enumerate(obs_lists)])
    e_tk = np.concatenate([l[first:] for l in obs_lists])
    pt_obs_begin = np.concatenate([[0], np.cumsum([len(l) - first for l in obs_lists])])

    def measure(pt_idx, tk_idx):
        Pc = np.einsum("eij,ej->ei", R_cw_all[tk_idx], pts_w[pt_idx] - p_wc[tk_idx])
        uv = np.stack([fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy], axis=1)
        n = len(pt_idx)
        octave = np.minimum(rng.geometric(0.45, n) - 1, 7)
        w = np.float32(1.0 / (1.2 ** (2 * octave))).astype(np.float64)
        out = np.zeros(n, dtype=bool)
        if noise:
            uv = uv + rng.normal(0, 1, (n, 2)) * (1.2 ** octave)[:, None] * pix_noise
            out = rng.uniform(size=n) < outlier_frac
            uv = uv + out[:, None] * rng.choice([-1.0, 1.0], (n, 2)) * rng.uniform(15, 25, (n, 2))
        return np.float32(uv).astype(np.float64), w, out, Pc[:, 2]

    obs_uv, obs_w, is_outlier, _ = measure(e_pt, e_tk)
    obs_kf = pidx[e_tk]
    if variant == abi.VARIANT_PRV_IDP:
        ref_tk = np.array([l[0] for l in obs_lists])
        _of = outlier_frac
        outlier_frac = 0.0   # the reference observation defines the bearing: noisy but never a gross outlier
        uvr, _w, _o, depth = measure(np.arange(n_pt), ref_tk)
        outlier_frac = _of
        depth0 = depth * (1 + (init_scale * rng.normal(0, 0.03, n_pt) if noise else 0.0))
        pt_arr = np.stack([1.0 / depth0, (uvr[:, 0] - cx) / fx, (uvr[:, 1] - cy) / fy], axis=1)
        pt_ref = pidx[ref_tk]
    else:
        pt_arr = pts_w + (init_scale * rng.normal(0, 0.05, (n_pt, 3)) if noise else 0)
        if variant == abi.VARIANT_SE3_XYZ:
            pt_arr = np.float32(pt_arr).astype(np.float64)
        pt_ref = np.zeros(n_pt, dtype=np.int64)

    # keyframe states: ground truth + initial-guess perturbation (free ones only)
    pose = np.zeros((n_kf, 7)); vel = np.zeros((n_kf, 3)); bias = np.zeros((n_kf, 12))
    pose_gt = np.zeros((n_kf, 7))
    for tk in range(n_kf):
        i = pidx[tk]
        Rk, Pk, Vk = Rs[tk], Ps[tk], Vs[tk]
        if variant == abi.VARIANT_SE3_XYZ:
            Rcw = R_wc[tk].T
            pose_gt[i] = np.concatenate([-Rcw @ p_wc[tk], rot_to_quat(Rcw)])
        else:
            pose_gt[i] = np.concatenate([Pk, rot_to_quat(Rk)])
        if i < n_free and noise:
            Rn = Rk @ so3_exp(init_scale * rng.normal(0, np.deg2rad(0.5), 3))
            Pn = Pk + init_scale * rng.normal(0, 0.02, 3)
            Vn = Vk + init_scale * rng.normal(0, 0.05, 3)
        else:
            Rn, Pn, Vn = Rk, Pk, Vk
        if variant == abi.VARIANT_SE3_XYZ:
            Rcw = (Rn @ R_bc).T
            tcw = -Rcw @ (Rn @ p_bc + Pn)
            # the vision path stores poses as float32 cv::Mat (include/Converter.h:56-60)
            T = np.eye(4); T[:3, :3] = Rcw; T[:3, 3] = tcw
            T = np.float32(T).astype(np.float64)
            pose[i] = np.concatenate([T[:3, 3], rot_to_quat(T[:3, :3])])
        else:
            pose[i] = np.concatenate([Pn, rot_to_quat(Rn)])
        vel[i] = Vn
        bias[i, 0:3] = bg_est; bias[i, 3:6] = ba_est

    prob_kw = dict(variant=variant, n_kf_free=n_free, kf_pose=pose, pt=np.array(pt_arr),
                   pt_obs_begin=pt_obs_begin, obs_kf=obs_kf, obs_uv=np.array(obs_uv), obs_w=obs_w, K=EUROC_K)
    if variant != abi.VARIANT_SE3_XYZ:
        # one PRV + one bias edge per consecutive keyframe pair whose later KF is free
        ei, ej = [], []
        om, ac, dts = [], [], []
        for tk in range(1, n_kf):
            if pidx[tk] >= n_free:
                continue   # edges between two fixed keyframes are never built (src/Optimizer.cpp:251-312)
            ei.append(pidx[tk - 1]); ej.append(pidx[tk])
            sl = slice((tk - 1) * S, tk * S)
            g = gyr_meas[sl] - bg_est
            a = acc_meas[sl] - ba_est
            # KeyFrame::ComputePreInt (src/KeyFrame.cpp:195-252): first sample integrated over t_imu0 - t_prevKF
            # (= 0 here) and then again inside the loop
            om.append(np.concatenate([g[:1], g])); ac.append(np.concatenate([a[:1], a]))
            dts.append(np.concatenate([[0.0], np.full(S, imu_dt)]))
        meas, cov = preintegrate(np.array(om), np.array(ac), np.array(dts))
        prob_kw.update(kf_vel=vel, kf_bias=bias, T_cb=T_cb, g_w=g_w, imu_kf_i=ei, imu_kf_j=ej, imu_meas=meas,
                       imu_info_prv=prv_information(cov).reshape(-1, 81))
    if variant == abi.VARIANT_PRV_IDP:
        prob_kw.update(pt_ref_kf=pt_ref, depth_min=0.01, algo=abi.ALGO_GN)
    else:
        prob_kw.update(depth_min=0.0, algo=abi.ALGO_LM)
    if algo is not None:
        prob_kw["algo"] = algo
    prob = abi.Problem(**prob_kw)
    prob.truth = dict(pose=pose_gt, vel=np.array([Vs[tk] for tk in tidx]), pts_w=pts_w, bg=bg_true, ba=ba_true,
                      bg_est=bg_est, ba_est=ba_est, is_outlier=np.array(is_outlier, dtype=bool), time_index=tidx,
                      R_bc=R_bc, p_bc=p_bc)
    return prob


# the BASELINE.json configurations
def config_c2(seed=2, landmark_order="random"):
    """Vision-only LocalBundleAdjustment: 20 KF / 2k MapPoints / ~12k EdgeSE3ProjectXYZ, LM."""
    return make_window(abi.VARIANT_SE3_XYZ, n_kf=20, n_fixed=2, n_pt=2000, n_obs=12000, seed=seed, landmark_order=landmark_order)


def config_c3(seed=3, n_kf=50, n_pt=5000, n_obs=30000, landmark_order="random"):
    """LocalBAPRVIDP: 50 KF (49 free + fixed predecessor) / 5k pts / 30k EdgePRIDP + 49 PRV + 49 bias, GN."""
    return make_window(abi.VARIANT_PRV_IDP, n_kf=n_kf, n_fixed=1, n_pt=n_pt, n_obs=n_obs, seed=seed, landmark_order=landmark_order)


def config_c3_ragged(seed=3, landmark_order="random", kinds=True):
    """A LocalBAPRVIDP window whose size is drawn around BASELINE configs[2]: 40..60 keyframes (mean 50), 100 landmarks per
    keyframe, 6 edges per landmark (mean 5 000 / 30 000) -- so that the windows of a batch differ in size, co-visibility and
    ITERATION COUNTS the way the windows of a real session do (everything depends on the seed only).  Three kinds of window:
    60 %: one-pixel keypoint noise and 2..8 % gross outliers (the window still holds the mismatches of its newest keyframes):
          Gauss-Newton runs 5 + 3 iterations;
    20 %: no gross outliers left (earlier passes erased them), keypoint noise 0.3 px: 4..5 + 2;
    20 %: no gross outliers, 0.1 px: 3..4 + 1 (the |dchi2| < 1e-3 stop is absolute, so it comes earlier where chi2 is small).
    kinds=False: the iteration mix of round 2 -- every window of the first kind (the same sizes, all 5 + 3), so that a rate can be
    compared like for like across rounds (bench.py --iteration-mix r2)."""
    r = np.random.default_rng(1000003 * seed + 17)
    n_kf = int(r.integers(40, 61))
    outlier_frac = float(r.uniform(0.02, 0.08))
    kind = float(r.uniform())
    pix = 1.0
    if kinds and kind >= 0.8:
        outlier_frac, pix = 0.0, 0.1
    elif kinds and kind >= 0.6:
        outlier_frac, pix = 0.0, 0.3
    return make_window(abi.VARIANT_PRV_IDP, n_kf=n_kf, n_fixed=1, n_pt=100 * n_kf, n_obs=600 * n_kf, seed=seed,
                       outlier_frac=outlier_frac, pix_noise=pix, landmark_order=landmark_order)


def config_c3s(seed=3, landmark_order="random"):
    """The LocalBAPRVIDP window of configs[2] with SCATTERED co-visibility: 50 free keyframes + 8 fixed older
    co-observers (src/Optimizer.cpp:199-232: every keyframe outside the window that sees a window landmark is added as a fixed
    vertex), 5 000 landmarks / 30 000 edges whose tracks are random subsets of the keyframes that see them (gaps instead of runs of
    consecutive keyframes), 10-20 % of the landmarks anchored in a fixed reference keyframe."""
    return make_window(abi.VARIANT_PRV_IDP, n_kf=58, n_fixed=8, n_pt=5000, n_obs=30000, seed=seed, tracks="random", landmark_order=landmark_order)


def config_c2s(seed=2, landmark_order="random"):
    """configs[1] with scattered co-visibility: the vision-only LocalBundleAdjustment(KeyFrame*, bool*, Map*, LocalMapping*) takes the
    co-visibility set of the current keyframe as its window (src/Optimizer.cpp:3861-3875), not a run of consecutive keyframes"""
    return make_window(abi.VARIANT_SE3_XYZ, n_kf=20, n_fixed=2, n_pt=2000, n_obs=12000, seed=seed, tracks="random", landmark_order=landmark_order)


def config_c4(seed=4, landmark_order="random"):
    """Synthetic VI graph: 200 KF / 50k pts / 500k obs + IMU chain."""
    return make_window(abi.VARIANT_PRV_IDP, n_kf=200, n_fixed=1, n_pt=50000, n_obs=500000, seed=seed, landmark_order=landmark_order)


def config_gba(seed=6, n_kf=300, n_pt=30000, n_obs=180000, its=10, robust=1):
    """GlobalBundleAdjustmentNavStatePRV at map scale: every keyframe free except PR/Bias of keyframe 0,
    XYZ landmarks, one optimize(its) with Levenberg-Marquardt."""
    p = make_window(abi.VARIANT_PRV_XYZ, algo=abi.ALGO_LM, n_kf=n_kf, n_fixed=0, n_pt=n_pt, n_obs=n_obs, seed=seed, outlier_frac=0.02)
    p.protocol, p.robust, p.its_stage1, p.its_stage2 = abi.PROTO_SINGLE, robust, its, 0
    p.huber_vis = float(np.float32(np.sqrt(5.99)))
    p.kf_fix = np.zeros(p.n_kf, np.uint8); p.kf_fix[0] = 0b101
    return p


def make_frame(seed=5, n_obs=300, last_is_frame=False, compute_marg=True, noise=True, outlier_frac=0.1, pt_noise=0.01):
    """One tracked frame for the IMU-aided PoseOptimization (src/Optimizer.cpp:1671-2317): the last keyframe / frame,
    the preintegration up to the current frame, n_obs map points seen by both, a perturbed initial state."""
    w = make_window(abi.VARIANT_PRV_XYZ, n_kf=3, n_fixed=1, n_pt=n_obs, n_obs=3 * n_obs, seed=seed, noise=noise,
                    outlier_frac=outlier_frac)
    rng = np.random.default_rng(seed + 7919)
    LAST, CUR = 0, 1                     # problem rows of time 1 and time 2
    k = [i for i in range(w.n_imu) if w.imu_kf_i[i] == LAST and w.imu_kf_j[i] == CUR][0]
    perm = [0, 1, 2, 6, 7, 8, 3, 4, 5]
    cov = np.linalg.inv(w.imu_info_prv[k].reshape(9, 9))[np.ix_(perm, perm)]
    pts = w.truth["pts_w"] + (rng.normal(0, pt_noise, (n_obs, 3)) if noise else 0.0)
    e_pt = np.repeat(np.arange(w.n_pt), np.diff(w.pt_obs_begin))
    sel_c, sel_l = w.obs_kf == CUR, w.obs_kf == LAST
    nav = lambda i: np.concatenate([w.kf_pose[i], w.kf_vel[i], w.kf_bias[i]])
    gt = w.truth
    nav_last = nav(LAST)
    if not last_is_frame:   # the last keyframe is trusted: ground truth pose
        nav_last[:7] = gt["pose"][LAST]; nav_last[7:10] = gt["vel"][LAST]
    kw = dict(nav=nav(CUR), nav_last=nav_last, obs_pw=pts[e_pt[sel_c]], obs_uv=w.obs_uv[sel_c], obs_w=w.obs_w[sel_c],
              K=w.K, T_cb=w.T_cb, g_w=w.g_w, imu_meas=w.imu_meas[k], imu_cov_pvphi=cov,
              last_is_frame=int(last_is_frame), compute_marg=int(compute_marg))
    if last_is_frame:
        sig = np.array([0.02] * 3 + [0.05] * 3 + [0.01] * 3 + [1e-3] * 3 + [1e-2] * 3)
        L = np.diag(1.0 / sig) + np.tril(rng.normal(0, 0.05, (15, 15)), -1) / sig[None, :]
        prior = nav_last.copy()
        prior[:3] = gt["pose"][LAST][:3] + rng.normal(0, 0.01, 3)
        kw.update(last_pw=pts[e_pt[sel_l]], last_uv=w.obs_uv[sel_l], last_w=w.obs_w[sel_l], prior_nav=prior, prior_info=L.T @ L)
    f = abi.FrameProblem(**kw)
    f.truth = dict(nav=np.concatenate([gt["pose"][CUR], gt["vel"][CUR]]), is_outlier=gt["is_outlier"][sel_c],
                   is_outlier_last=gt["is_outlier"][sel_l])
    return f


def make_frame_vision(seed=1, n_obs=200, noise=True, outlier_frac=0.1, pt_noise=0.01):
    """BASELINE configs[0] (C1): one frame, ~200 monocular correspondences, vision-only Optimizer::PoseOptimization(Frame*)
    (src/Optimizer.cpp:3610-3835).  nav[0..6] = T_cw as SE3Quat, float32-narrowed like pFrame->mTcw; points float32."""
    f = make_frame(seed=seed, n_obs=n_obs, noise=noise, outlier_frac=outlier_frac, pt_noise=pt_noise)
    R_bc, p_bc, _ = extrinsics()

    def tcw(nav):
        Rwb = quat_to_rot(nav[3:7])
        Rcw = (Rwb @ R_bc).T
        t = -Rcw @ (Rwb @ p_bc + nav[:3])
        T = np.float32(np.concatenate([Rcw.reshape(-1), t])).astype(np.float64)
        return np.concatenate([T[9:], rot_to_quat(_orthonormalise(T[:9].reshape(3, 3)))])
    nav = np.zeros(abi.NAV_STRIDE); nav[:7] = tcw(f.nav)
    g = abi.FrameProblem(nav=nav, nav_last=np.zeros(abi.NAV_STRIDE), obs_pw=np.float32(f.obs_pw).astype(np.float64), obs_uv=f.obs_uv,
                         obs_w=f.obs_w, K=f.K, T_cb=f.T_cb, g_w=f.g_w, imu_meas=f.imu_meas, imu_cov_pvphi=f.imu_cov_pvphi,
                         last_is_frame=2, compute_marg=0)
    gt = np.concatenate([f.truth["nav"][:7], np.zeros(3)])
    g.truth = dict(T_cw=tcw(gt), is_outlier=f.truth["is_outlier"])
    return g


# ---------------------------------------------------------------- loop-closure Sim3 candidates (vba_sim3_optimize)
def _sim3_exp(u):
    """exp of a sim(3) tangent (omega, upsilon, sigma) as (R, t, s), through the series of the 4x4 generator
    [[sigma I + [omega]x, upsilon], [0, 0]] (input synthesis only: not the closed form under test)"""
    G = np.zeros((4, 4))
    G[:3, :3] = hat(u[:3]) + u[6] * np.eye(3)
    G[:3, 3] = u[3:6]
    E, T = np.eye(4), np.eye(4)
    for k in range(1, 40):
        T = T @ G / k
        E = E + T
    s = float(np.exp(u[6]))
    return _orthonormalise(E[:3, :3] / s), E[:3, 3].copy(), s


def make_sim3_pair(seed, n_pairs, fix_scale=False, outlier_frac=0.1, noise=True, same_K=False):
    """One loop candidate as Optimizer::OptimizeSim3 sees it (src/Optimizer.cpp:4579-4720): a true S12 (rotation ~0.2 rad,
    translation ~0.3 m, log-scale sigma 0.15 unless fixed), points 3-10 m in front of KF2 mapped into KF1, pixel noise of one sigma
    per octave (octaves 0-3, w = 1.2^(-2 octave)), gross errors of 8-40 px on outlier_frac of the pairs, K2 != K1 unless same_K,
    and an initial S12 perturbed from the truth by (0.03 rad, 0.1 m, 0.05) as a RANSAC seed would be."""
    r = np.random.default_rng(seed)
    n = int(n_pairs)
    K1 = EUROC_K.copy()
    K2 = K1.copy() if same_K else K1 * np.array([1.02, 0.99, 1.01, 0.97])
    R, _, _ = _sim3_exp(np.concatenate([r.normal(size=3) * 0.2, np.zeros(4)]))
    t = r.normal(size=3) * 0.3
    s = 1.0 if fix_scale else float(np.exp(r.normal() * 0.15))
    p2 = np.stack([r.uniform(-2, 2, n), r.uniform(-1.5, 1.5, n), r.uniform(3, 10, n)], axis=1)
    p1 = s * p2 @ R.T + t
    lv1, lv2 = r.integers(0, 4, n), r.integers(0, 4, n)
    w1, w2 = 1.2 ** (-2.0 * lv1), 1.2 ** (-2.0 * lv2)
    uv1 = p1[:, :2] / p1[:, 2:3] * K1[:2] + K1[2:]
    uv2 = p2[:, :2] / p2[:, 2:3] * K2[:2] + K2[2:]
    if noise:
        uv1 = uv1 + r.normal(size=(n, 2)) * (1.2 ** lv1)[:, None]
        uv2 = uv2 + r.normal(size=(n, 2)) * (1.2 ** lv2)[:, None]
    m = r.random(n) < outlier_frac
    uv1[m] += r.uniform(8, 40, (int(m.sum()), 2)) * r.choice([-1.0, 1.0], (int(m.sum()), 2))
    u0 = np.concatenate([r.normal(size=3) * 0.03, r.normal(size=3) * 0.1, [0.0 if fix_scale else r.normal() * 0.05]])
    dR, dt, ds = _sim3_exp(u0)
    R0, t0, s0 = dR @ R, ds * (dR @ t) + dt, (s if fix_scale else ds * s)
    S12 = np.concatenate([t0, rot_to_quat(R0), [s0]])
    return abi.Sim3Problem(S12=S12, p1c=p1, p2c=p2, uv1=uv1, uv2=uv2, w1=w1, w2=w2, K1=K1, K2=K2, fix_scale=int(bool(fix_scale)),
                           truth=dict(S12=np.concatenate([t, rot_to_quat(R), [s]]), is_outlier=m))


def make_sim3_ransac(seed, n_pairs, fix_scale, outlier_frac, noise3d=0.01, same_K=False):
    """One loop candidate as Sim3Solver sees it after its constructor (src/Sim3Solver.cpp:29-95): the geometry of make_sim3_pair
    (a true S12, points 3-10 m in front of KF2 mapped into KF1), but with the noise ON THE 3D POINTS of both sides, proportional
    to the depth: noise3d (1 %) of z along z and a tenth of that across, as triangulated map points err.  Exact 3D correspondences
    would make every clean hypothesis perfect and the first one a hit.  The p1c of outlier_frac of the pairs are replaced by
    unrelated points; the gates are 9.210 sigma2 of octaves 0-3 (:78-79).  No triples: draw_triples; truth: S12, is_outlier."""
    r = np.random.default_rng(seed)
    n = int(n_pairs)
    K1 = EUROC_K.copy()
    K2 = K1.copy() if same_K else K1 * np.array([1.02, 0.99, 1.01, 0.97])
    R, _, _ = _sim3_exp(np.concatenate([r.normal(size=3) * 0.2, np.zeros(4)]))
    t = r.normal(size=3) * 0.3
    s = 1.0 if fix_scale else float(np.exp(r.normal() * 0.15))
    p2 = np.stack([r.uniform(-2, 2, n), r.uniform(-1.5, 1.5, n), r.uniform(3, 10, n)], axis=1)
    p1 = s * p2 @ R.T + t
    sig = np.array([0.1 * noise3d, 0.1 * noise3d, noise3d])
    p1 = p1 + r.normal(size=(n, 3)) * sig * p1[:, 2:3]
    p2 = p2 + r.normal(size=(n, 3)) * sig * p2[:, 2:3]
    m = r.random(n) < outlier_frac
    k = int(m.sum())
    p1[m] = np.stack([r.uniform(-2, 2, k), r.uniform(-1.5, 1.5, k), r.uniform(3, 10, k)], axis=1)
    lv1, lv2 = r.integers(0, 4, n), r.integers(0, 4, n)
    return abi.Sim3RansacProblem(p1c=p1, p2c=p2, max_err1=9.210 * 1.2 ** (2.0 * lv1), max_err2=9.210 * 1.2 ** (2.0 * lv2), K1=K1, K2=K2,
                                 sample=np.zeros((0, 3), dtype=np.int32), fix_scale=int(bool(fix_scale)),
                                 truth=dict(S12=np.concatenate([t, rot_to_quat(R), [s]]), is_outlier=m))


def draw_triples(seed, n_pairs, n_hyp):
    """[n_hyp, 3] int32: three distinct pair indices per hypothesis (the library takes any indices; the facade draws as the
    reference does)"""
    r = np.random.default_rng(seed)
    return np.stack([r.choice(int(n_pairs), 3, replace=False) for _ in range(int(n_hyp))]).astype(np.int32).reshape(-1, 3)


# ---------------------------------------------------------------- new map points (vba_triangulate)
TRI_KINDS = ("good", "far", "gross", "octave", "behind2", "chi2_2")


def level_tables(n_levels=8, scale_factor=1.2):
    """mvScaleFactors and mvLevelSigma2 as ORBextractor builds them in float32, widened"""
    s = np.ones(n_levels, dtype=np.float32)
    for i in range(1, n_levels):
        s[i] = s[i - 1] * np.float32(scale_factor)
    return s.astype(np.float64), (s * s).astype(np.float64)


def make_triangulate(seed, n_matches, kind="std", n_levels=8, scale_factor=1.2, same_K=True):
    """One keyframe pair of LocalMapping::CreateNewMapPoints with its matches, every input rounded through float32 as the reference
    holds it.  EuRoC intrinsics, a baseline of 0.1-0.5 m, a relative rotation of a few degrees.  kind:
      std      a sideways baseline near the origin; matches: 68 % true points 1.5-12 m deep, 15 % 60-400 m deep (these fail the
               parallax gate), 10 % gross mismatches (a random pixel in keyframe 2), 7 % with octaves that disagree by five levels
      far      the pair about 50 m from the origin, every depth chosen so that the parallax lies just inside the gate (1.03-1.6
               times the gate's angle)
      forward  a baseline along the optical axis; beside the std mix, a tenth of the matches is a point between the two cameras
               (in front of keyframe 1, behind keyframe 2) and a tenth a close point seen at octave 7 in keyframe 1 and octave 0 in
               keyframe 2 with a few pixels of error in keyframe 2 (passes keyframe 1's chi-square test, fails keyframe 2's)
    Pixel noise: 0.7 pixels times the scale of the octave.  truth: kind [n] (index into TRI_KINDS), Xw [n,3]."""
    r = np.random.default_rng(seed)
    n = int(n_matches)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    K1 = f32(EUROC_K).astype(np.float64)
    K2 = K1.copy() if same_K else f32(K1 * np.array([1.02, 0.99, 1.01, 0.97])).astype(np.float64)
    scale, sigma2 = level_tables(n_levels, scale_factor)
    R1 = so3_exp(r.normal(size=3) * 0.5)
    C1 = r.uniform(-2, 2, 3)
    if kind == "far":
        u = r.normal(size=3)
        C1 = 50.0 * u / np.linalg.norm(u)
    b = r.uniform(0.1, 0.5)
    a = r.uniform(0, 2 * np.pi)
    d = np.array([0.2 * np.cos(a), 0.1 * np.sin(a), 1.0]) if kind == "forward" else np.array([np.cos(a), 0.3 * np.sin(a), r.uniform(-0.1, 0.1)])
    d /= np.linalg.norm(d)
    C2 = C1 + R1.T @ (b * d)
    R2 = so3_exp(r.normal(size=3) * 0.03) @ R1

    def pose(R, Cw):   # the float32 pose of a keyframe and the centre it derives from it (KeyFrame::SetPose)
        R32 = f32(R)
        t32 = f32(-(R32.astype(np.float64) @ Cw))
        return R32.astype(np.float64), t32.astype(np.float64), (-(R32.T @ t32)).astype(np.float64)

    Rcw1, tcw1, Ow1 = pose(R1, C1)
    Rcw2, tcw2, Ow2 = pose(R2, C2)
    probs = dict(std=[0.68, 0.15, 0.10, 0.07, 0, 0], far=[1, 0, 0, 0, 0, 0], forward=[0.50, 0.13, 0.10, 0.07, 0.10, 0.10])[kind]
    kinds = r.choice(len(TRI_KINDS), size=n, p=probs)
    oct1 = r.choice(n_levels, size=n, p=np.array([35, 25, 15, 10, 6, 4, 3, 2])[:n_levels] / np.array([35, 25, 15, 10, 6, 4, 3, 2])[:n_levels].sum())
    oct2 = np.clip(oct1 + r.choice([-1, 0, 0, 0, 1], size=n), 0, n_levels - 1)
    uv1 = np.stack([r.uniform(20, 732, n), r.uniform(20, 460, n)], axis=1)
    depth = r.uniform(1.5, 12, n)
    depth = np.where(kinds == 1, r.uniform(60, 400, n), depth)
    if kind == "far":
        depth = b * np.sqrt(1 - d[2] ** 2) / (np.arccos(0.9998) * r.uniform(1.03, 1.6, n))
    m = kinds == 5
    depth = np.where(m, r.uniform(1.2, 2.5, n), depth)
    oct1 = np.where(m, n_levels - 1, oct1)
    oct2 = np.where(m, 0, oct2)
    m = kinds == 3
    flip = r.random(n) < 0.5
    oct1 = np.where(m, np.where(flip, r.integers(0, 2, n), n_levels - 1 - r.integers(0, 2, n)), oct1)
    oct2 = np.where(m, np.where(flip, n_levels - 1 - r.integers(0, 2, n), r.integers(0, 2, n)), oct2)
    oct1, oct2 = np.clip(oct1, 0, n_levels - 1), np.clip(oct2, 0, n_levels - 1)
    Xc1 = depth[:, None] * np.stack([(uv1[:, 0] - K1[2]) / K1[0], (uv1[:, 1] - K1[3]) / K1[1], np.ones(n)], axis=1)
    m = kinds == 4     # between the cameras, a third of the baseline off the axis
    ph = r.uniform(0, 2 * np.pi, n)
    Xc1 = np.where(m[:, None], b * np.stack([0.3 * np.cos(ph), 0.3 * np.sin(ph), r.uniform(0.35, 0.65, n)], axis=1), Xc1)
    Xw = Xc1 @ R1 + C1
    proj = lambda K, R, C, X: (lambda Y: np.stack([K[0] * Y[:, 0] / Y[:, 2] + K[2], K[1] * Y[:, 1] / Y[:, 2] + K[3]], axis=1))((X - C) @ R.T)
    uv1 = proj(K1, R1, C1, Xw)
    uv2 = proj(K2, R2, C2, Xw)
    noise = np.where((kinds == 4)[:, None], 0.05, 0.7)
    uv1 = uv1 + r.normal(size=(n, 2)) * noise * scale[oct1][:, None]
    uv2 = uv2 + r.normal(size=(n, 2)) * noise * scale[oct2][:, None]
    m = kinds == 5
    ph = r.uniform(0, 2 * np.pi, n)
    uv2 = np.where(m[:, None], uv2 + r.uniform(4, 7, n)[:, None] * np.stack([np.cos(ph), np.sin(ph)], axis=1), uv2)
    m = kinds == 2
    uv2 = np.where(m[:, None], np.stack([r.uniform(20, 732, n), r.uniform(20, 460, n)], axis=1), uv2)
    return abi.TriangulateProblem(Rcw1=Rcw1, tcw1=tcw1, Ow1=Ow1, K1=K1, Rcw2=Rcw2, tcw2=tcw2, Ow2=Ow2, K2=K2, level_sigma2_1=sigma2, scale_1=scale,
                                  level_sigma2_2=sigma2, scale_2=scale, uv1=f32(uv1).astype(np.float64), uv2=f32(uv2).astype(np.float64),
                                  oct1=oct1, oct2=oct2, ratio_factor=float(np.float32(1.5) * np.float32(scale_factor)), cos_max=0.9998, chi2_th=5.991,
                                  truth=dict(kind=kinds, Xw=Xw))


# ---------------------------------------------------------------- essential graphs (vba_posegraph_optimize)
TWO_VIEW_KINDS = ("general", "plane", "rotation")


def draw_sets(seed, n_matches, n_hyp):
    """n_hyp sets of eight distinct match indices (mvSets, src/Initializer.cpp:78-101, drawn with NumPy's generator); where
    n_matches allows it no two sets hold the same eight matches, so that no two hypotheses fit the same data"""
    rng = np.random.default_rng(seed)
    sets, seen = [], set()
    for _ in range(n_hyp):
        for attempt in range(50):
            s = rng.choice(n_matches, 8, replace=False)
            key = tuple(sorted(s.tolist()))
            if key not in seen:
                break
        seen.add(key)
        sets.append(s)
    return np.array(sets, dtype=np.int32).reshape(-1, 8)


def make_two_view(seed, n_matches, n_hyp, kind="general", baseline=0.5, noise=0.3, outlier_frac=0.0, far_frac=0.0, extra_keys=(37, 53),
                  min_triangulated=50, min_parallax=1.0, rot_deg=3.0, float32=True):
    """One frame pair of Initializer::Initialize: n_matches points of a scene seen from frame 1 (the origin) and frame 2 (R21, t21),
    pixel noise of `noise` pixels, a share of wrong matches, a share of points some hundred metres away (parallax below the
    0.99998 cosine), unmatched keypoints in both frames, everything through float32 (float32=False: exact doubles, for known-answer checks).  kind: 'general' (a box 4-10 m deep),
    'plane' (a tilted plane 6 m away), 'rotation' (the general scene, t = 0).  truth: R21, t21 (unit), the wrong matches."""
    rng = np.random.default_rng(seed)
    K = np.array([500.0, 480.0, 320.0, 240.0])
    n = n_matches
    z = rng.uniform(4.0, 10.0, n)
    if kind == "plane":
        a, b = rng.uniform(-0.3, 0.3, 2)
    xy = rng.uniform(-0.45, 0.45, (n, 2))
    if kind == "plane":
        z = 6.0 / (1.0 - a * xy[:, 0] - b * xy[:, 1])                  # z = 6 + a x + b y with x = xy z
    far = rng.random(n) < far_frac
    z = np.where(far, rng.uniform(300.0, 600.0, n), z)
    X = np.column_stack([xy[:, 0] * z, xy[:, 1] * z, z])
    R = so3_exp(np.deg2rad(rot_deg) * rng.normal(size=3) / np.sqrt(3.0))
    d = rng.normal(size=3) * np.array([1.0, 0.6, 0.25])
    d /= np.linalg.norm(d)
    t = np.zeros(3) if kind == "rotation" else baseline * d
    Y = X @ R.T + t
    proj = lambda P: np.column_stack([K[0] * P[:, 0] / P[:, 2] + K[2], K[1] * P[:, 1] / P[:, 2] + K[3]])
    p1 = proj(X) + noise * rng.normal(size=(n, 2))
    p2 = proj(Y) + noise * rng.normal(size=(n, 2))
    wrong = rng.random(n) < outlier_frac
    p2[wrong] = np.column_stack([rng.uniform(0, 640, wrong.sum()), rng.uniform(0, 480, wrong.sum())])
    nk1, nk2 = n + extra_keys[0], n + extra_keys[1]
    i1, i2 = np.sort(rng.permutation(nk1)[:n]), rng.permutation(nk2)[:n]   # mvMatches12 ascends in the first index (:51-62)
    uv1 = np.column_stack([rng.uniform(0, 640, nk1), rng.uniform(0, 480, nk1)])
    uv2 = np.column_stack([rng.uniform(0, 640, nk2), rng.uniform(0, 480, nk2)])
    uv1[i1], uv2[i2] = p1, p2
    f32 = (lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)) if float32 else (lambda a: np.asarray(a, dtype=np.float64))
    return abi.TwoViewProblem(f32(uv1), f32(uv2), np.column_stack([i1, i2]), draw_sets(seed + 7919, n, n_hyp), f32(K), 1.0, min_parallax,
                              min_triangulated, truth=dict(R21=R, t21=d if kind != "rotation" else t, wrong=wrong, far=far))


def _s3_mul(a, b):
    return a[0] @ b[0], a[2] * (a[0] @ b[1]) + a[1], a[2] * b[2]


def _s3_inv(a):
    return a[0].T, -(a[0].T @ a[1]) / a[2], 1.0 / a[2]


def _s3_pack(a):
    return np.concatenate([a[1], rot_to_quat(a[0]), [a[2]]])


def make_posegraph(seed, n_kf, span=3, loops=None, fix_scale=False, fixed_at=0, rot_drift=2e-3, trans_drift=2e-2, scale_drift=2e-3,
                   n_corrected=None, dup_edge=None, isolated=False, n_pt=0, loop_rot_err=0.0, noise=True, radius=5.0):
    """One essential graph as Optimizer::OptimizeEssentialGraph sees it (src/Optimizer.cpp:4243-4478).
    A closed trajectory of n_kf keyframes on a circle (Siw = camera-from-world, scale 1); odometry composes the true relative
    motions with a drift in rotation, translation and (unless fix_scale) scale per step, starting from the truth at keyframe 0.
    Edges (vertex 0 = i, vertex 1 = j, measurement Sji = Sjw Swi):
      * from every keyframe i to its `span` predecessors, measured from the DRIFTED poses (what the reference does with
        NonCorrectedSim3: spanning-tree and covisibility edges);
      * `loops`: a list of (i, j) pairs that carry the TRUE relative pose (default: one loop, (n_kf - 1, 0)), turned by
        loop_rot_err radians about a fixed axis when that is not 0 (a wrong loop measurement).
    Initial estimates are the drifted poses, except for the last n_corrected keyframes (default span + 1), to which the loop
    correction of the last keyframe is propagated (CorrectedSim3, src/LoopClosing.cpp:452-474): the input has the discontinuity
    the real one has.  fixed_at: the fixed vertex (None: none).  dup_edge: index of an edge that is listed twice; isolated: one
    more vertex without edges; n_pt: map points around the trajectory with random reference vertices.  noise=False: no drift at all
    (the input is the truth).  truth['S']: the true Siw."""
    r = np.random.default_rng(seed)
    n = int(n_kf)
    ang = 2 * np.pi * np.arange(n) / n
    true = []
    for k in range(n):
        Rwc = so3_exp(np.array([0.0, 0.0, ang[k]])) @ so3_exp(0.05 * np.array([np.sin(3 * ang[k]), np.cos(2 * ang[k]), 0.0]))
        c = np.array([radius * np.cos(ang[k]), radius * np.sin(ang[k]), 0.2 * np.sin(3 * ang[k])])
        true.append((Rwc.T, -Rwc.T @ c, 1.0))
    drift = [true[0]]
    for k in range(1, n):
        rel = _s3_mul(true[k], _s3_inv(true[k - 1]))
        if noise:
            u = np.concatenate([r.normal(size=3) * rot_drift, r.normal(size=3) * trans_drift,
                                [0.0 if fix_scale else r.normal() * scale_drift]])
            rel = _s3_mul(_sim3_exp(u), rel)
        drift.append(_s3_mul(rel, drift[k - 1]))
    ei, ej, meas = [], [], []
    for i in range(1, n):
        for j in range(max(0, i - span), i):
            ei.append(i); ej.append(j); meas.append(_s3_mul(drift[j], _s3_inv(drift[i])))
    if loops is None:
        loops = [(n - 1, 0)]
    wrong = (so3_exp(loop_rot_err * np.array([0.6, 0.0, 0.8])), np.zeros(3), 1.0)
    for i, j in loops:
        ei.append(int(i)); ej.append(int(j))
        m = _s3_mul(true[j], _s3_inv(true[i]))
        meas.append(_s3_mul(wrong, m) if loop_rot_err else m)
    if dup_edge is not None:
        ei.append(ei[dup_edge]); ej.append(ej[dup_edge]); meas.append(meas[dup_edge])
    # CorrectedSim3: g2oCorrectedSiw = g2oSic * g2oCorrectedScw, Sic from the uncorrected poses
    init = list(drift)
    nc = span + 1 if n_corrected is None else int(n_corrected)
    if noise and loops:
        cur = n - 1
        for i in range(max(1, n - nc), n):
            init[i] = _s3_mul(_s3_mul(drift[i], _s3_inv(drift[cur])), true[cur])
    S = np.stack([_s3_pack(a) for a in init])
    St = np.stack([_s3_pack(a) for a in true])
    fixed = np.zeros(n, dtype=np.uint8)
    if fixed_at is not None:
        fixed[fixed_at] = 1
    if isolated:
        extra = _s3_pack((so3_exp(r.normal(size=3) * 0.3), r.normal(size=3), 1.0 if fix_scale else 1.1))
        S, St, fixed = np.vstack([S, extra]), np.vstack([St, extra]), np.append(fixed, np.uint8(0))
    pt = pt_ref = None
    if n_pt:
        a = r.uniform(0, 2 * np.pi, n_pt)
        pt = np.stack([(radius + r.uniform(1, 4, n_pt)) * np.cos(a), (radius + r.uniform(1, 4, n_pt)) * np.sin(a), r.uniform(-1, 1, n_pt)], axis=1)
        pt_ref = r.integers(0, n, n_pt)
    return abi.PoseGraphProblem(S=S, fixed=fixed, edge_i=ei, edge_j=ej, edge_S=np.stack([_s3_pack(m) for m in meas]),
                                fix_scale=int(bool(fix_scale)), pt=pt, pt_ref=pt_ref, truth=dict(S=St))


# ---------------------------------------------------------------- matching for triangulation (vba_search_triangulation)
def compute_f12(Rcw1, tcw1, K1, Rcw2, tcw2, K2):
    """LocalMapping::ComputeF12 (src/LocalMapping.cpp:1659-1680) in float64 on the inputs as given: K1^-T [t12]x R12 K2^-1"""
    R12 = Rcw1 @ Rcw2.T
    t12 = -R12 @ tcw2 + tcw1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    Kinv = lambda K: np.array([[1 / K[0], 0, -K[2] / K[0]], [0, 1 / K[1], -K[3] / K[1]], [0, 0, 1]])
    return Kinv(K1).T @ tx @ R12 @ Kinv(K2)


def synth_match_pair(seed, n_true=60, n_distract1=20, n_distract2=20, n_nodes=12, flip_bits=12, unshared=0.1, mp1=0.1, mp2=0.1,
                     n_levels=8, scale_factor=1.2, angle_noise=3.0, rot_outliers=0.1, noise=0.3, check_orientation=True, th_low=50, big_node=0):
    """One keyframe pair of ORBmatcher::SearchForTriangulation, every input rounded through float32 as the reference holds it.  A
    two-view scene with known poses (EuRoC intrinsics, a sideways baseline of 0.2-0.5 m, a relative rotation of a few degrees, an
    in-plane roll of about 40 degrees so that rot = angle1 - angle2 is of either sign); n_true world features 2-10 m deep with
    random 256-bit descriptors, seen by both keyframes as copies with flip_bits flipped bits each; n_distract1 / n_distract2
    keypoints per keyframe that exist only there (random descriptor, random pixel).  Every true feature sits in one of n_nodes
    vocabulary nodes in both keyframes, except the share `unshared`, whose copy in keyframe 2 sits in another node; distractors
    sit in random nodes, and node ids exist that only one keyframe uses.  Shares mp1 / mp2 of the keypoints already have a map
    point.  big_node: the first big_node true features sit in node 0 in both keyframes.  Angles: that of keyframe 2 is that of keyframe 1 minus the roll plus angle_noise degrees of noise; the share
    rot_outliers of the true features gets a random angle in keyframe 2.  Keypoints are shuffled, so node_feat is not ascending.
    truth: pair [n_true,2] (idx1, idx2), shared [n_true] bool."""
    r = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    K = f32(EUROC_K).astype(np.float64)
    scale, sigma2 = level_tables(n_levels, scale_factor)
    roll = np.deg2rad(r.uniform(30, 50))
    R1 = so3_exp(r.normal(size=3) * 0.3)
    C1 = r.uniform(-1, 1, 3)
    a = r.uniform(0, 2 * np.pi)
    d = np.array([np.cos(a), 0.4 * np.sin(a), r.uniform(-0.1, 0.1)])
    C2 = C1 + R1.T @ (r.uniform(0.2, 0.5) * d / np.linalg.norm(d))
    R2 = so3_exp(np.array([0.0, 0.0, roll])) @ so3_exp(r.normal(size=3) * 0.03) @ R1

    def pose(R, Cw):
        R32 = f32(R)
        return R32.astype(np.float64), f32(-(R32.astype(np.float64) @ Cw)).astype(np.float64)

    Rcw1, tcw1 = pose(R1, C1)
    Rcw2, tcw2 = pose(R2, C2)
    n1, n2 = n_true + n_distract1, n_true + n_distract2
    oct_p = np.array([35, 25, 15, 10, 6, 4, 3, 2] + [1] * 56)[:n_levels].astype(float)
    oct_t = r.choice(n_levels, size=n_true, p=oct_p / oct_p.sum())
    # true features: a pixel in keyframe 1, a depth, the world point, its pixel in keyframe 2
    uv1t = np.stack([r.uniform(60, 690, n_true), r.uniform(60, 420, n_true)], axis=1)
    depth = r.uniform(2, 10, n_true)
    Xc1 = depth[:, None] * np.stack([(uv1t[:, 0] - K[2]) / K[0], (uv1t[:, 1] - K[3]) / K[1], np.ones(n_true)], axis=1)
    Xw = Xc1 @ R1 + C1
    Y = (Xw - C2) @ R2.T
    uv2t = np.stack([K[0] * Y[:, 0] / Y[:, 2] + K[2], K[1] * Y[:, 1] / Y[:, 2] + K[3]], axis=1)
    uv1t = uv1t + r.normal(size=(n_true, 2)) * noise * scale[oct_t][:, None]
    uv2t = uv2t + r.normal(size=(n_true, 2)) * noise * scale[oct_t][:, None]
    base = r.integers(0, 256, (n_true, 32), dtype=np.uint8)

    def flipped(dsc):
        out = np.unpackbits(dsc, axis=1)
        which = np.argsort(r.random(out.shape), axis=1)[:, :flip_bits]     # flip_bits distinct positions per row
        np.put_along_axis(out, which, 1 - np.take_along_axis(out, which, axis=1), axis=1)
        return np.packbits(out, axis=1)

    d1 = np.vstack([flipped(base), r.integers(0, 256, (n_distract1, 32), dtype=np.uint8)])
    d2 = np.vstack([flipped(base), r.integers(0, 256, (n_distract2, 32), dtype=np.uint8)])
    rnd_uv = lambda n: np.stack([r.uniform(20, 732, n), r.uniform(20, 460, n)], axis=1)
    uv1 = np.vstack([uv1t, rnd_uv(n_distract1)])
    uv2 = np.vstack([uv2t, rnd_uv(n_distract2)])
    ang1 = r.uniform(0, 360, n1)
    ang2t = ang1[:n_true] - np.rad2deg(roll) + r.normal(size=n_true) * angle_noise
    out = r.random(n_true) < rot_outliers
    ang2t = np.where(out, r.uniform(0, 360, n_true), ang2t)
    ang2 = np.mod(np.concatenate([ang2t, r.uniform(0, 360, n_distract2)]), 360.0)
    ang1 = f32(ang1); ang2 = f32(ang2)
    ang1[ang1 >= 360] = 0; ang2[ang2 >= 360] = 0
    oct2 = np.concatenate([np.clip(oct_t + r.choice([-1, 0, 0, 0, 1], size=n_true), 0, n_levels - 1), r.choice(n_levels, size=n_distract2, p=oct_p / oct_p.sum())])
    # nodes: ids 10 * k + 5 are shared candidates, 10 * k + 1 exist in keyframe 1 only, 10 * k + 8 in keyframe 2 only
    node_t = r.integers(0, n_nodes, n_true)
    shared = r.random(n_true) >= unshared
    node_t[:big_node] = 0                                  # the first big_node true features share node 0 in both keyframes
    shared[:big_node] = True
    node1 = np.concatenate([10 * node_t + 5, np.where(r.random(n_distract1) < 0.3, 10 * r.integers(0, n_nodes, n_distract1) + 1, 10 * r.integers(0, n_nodes, n_distract1) + 5)])
    node2t = np.where(shared, 10 * node_t + 5, 10 * ((node_t + 1 + r.integers(0, max(n_nodes - 1, 1), n_true)) % n_nodes) + 5)
    if n_nodes == 1:
        shared[:] = True
        node2t = 10 * node_t + 5
    node2 = np.concatenate([node2t, np.where(r.random(n_distract2) < 0.3, 10 * r.integers(0, n_nodes, n_distract2) + 8, 10 * r.integers(0, n_nodes, n_distract2) + 5)])
    has1 = (r.random(n1) < mp1).astype(np.uint8)
    has2 = (r.random(n2) < mp2).astype(np.uint8)
    # shuffle the keypoints of both keyframes
    p1, p2 = r.permutation(n1), r.permutation(n2)          # new index -> old index
    inv1, inv2 = np.argsort(p1), np.argsort(p2)

    def fv(node, perm):
        m = {}
        for new in r.permutation(len(perm)):               # the order inside a node is not ascending
            m.setdefault(int(node[perm[new]]), []).append(int(new))
        return abi.feat_vec_csr(m)

    id1, b1, ft1 = fv(node1, p1)
    id2, b2, ft2 = fv(node2, p2)
    F12 = f32(compute_f12(Rcw1, tcw1, K, Rcw2, tcw2, K)).astype(np.float64)
    Cw1 = -(f32(Rcw1).T @ f32(tcw1))                       # GetCameraCenter in float32
    C2c = f32(Rcw2) @ Cw1 + f32(tcw2)
    invz = np.float32(1.0) / C2c[2]
    K32 = f32(K)
    ex, ey = K32[0] * C2c[0] * invz + K32[2], K32[1] * C2c[1] * invz + K32[3]
    return abi.SearchTriProblem(desc1=d1[p1], desc2=d2[p2], has_mp1=has1[p1], has_mp2=has2[p2], node_id1=id1, node_begin1=b1, node_feat1=ft1,
                                node_id2=id2, node_begin2=b2, node_feat2=ft2, uv1=f32(uv1[p1]).astype(np.float64), uv2=f32(uv2[p2]).astype(np.float64),
                                angle1=ang1[p1], angle2=ang2[p2], oct2=oct2[p2], level_sigma2_2=sigma2, scale_2=scale, F12=F12,
                                epipole=np.array([float(ex), float(ey)]), th_low=th_low, check_orientation=check_orientation,
                                truth=dict(pair=np.stack([inv1[:n_true], inv2[:n_true]], axis=1), shared=shared,
                                           pose=(Rcw1, tcw1, Rcw2, tcw2, K)))


# ---------------------------------------------------------------- projection search for map-point fusion (vba_fuse)
FUSE_KINDS = ("match", "far_desc", "random", "behind", "outside", "distance", "angle", "level_high", "skip")


def fuse_scene(seed, n_keys=1000, n_pt=600, n_levels=8, scale_factor=1.2, flip_bits=12, width=640, height=480, cols=64, rows=48,
               mix=(0.62, 0.06, 0.1, 0.04, 0.04, 0.04, 0.04, 0.03, 0.03), noise=0.4, th=3.0, th_low=50, check_reproj=True):
    """One ORBmatcher::Fuse call, every input rounded through float32 as the reference holds it.  A keyframe with a random pose, a
    pinhole camera of width x height pixels, n_keys keypoints at random pixels with random 256-bit descriptors and octaves, the
    cols x rows grid assigned as Frame::AssignFeaturesToGrid does (abi.grid_csr).  n_pt map points, each of one kind, with the
    shares of `mix` (FUSE_KINDS):
      match       the back-projection of one keypoint (every keypoint once before any is taken twice) 2-10 m deep, noise pixels of noise
                  times its level's scale, the keypoint's descriptor with flip_bits flipped bits
      far_desc    the same with 90 flipped bits
      random      a random pixel, depth and descriptor (no keypoint in the area, or none similar)
      behind      behind the camera;  outside  in front of it but out of the image
      distance    a distance range that does not hold the point;  angle  a normal that looks away
      level_high  a distance between 0.84 and 0.99 of mfMinDistance: the predicted level is n_levels
      skip        a match that the caller marks as skipped
    Normal and distances come from a reference view 0.1-0.5 m from the keyframe's centre, which saw the point at the keypoint's
    octave: normal = the unit vector from it, mfMaxDistance = its distance times that level's scale, mfMinDistance = mfMaxDistance
    over the last level's scale, dist_min / dist_max = 0.8f / 1.2f times those (MapPoint.cpp).  truth: kind [n_pt] (index into
    FUSE_KINDS), key [n_pt] (the keypoint of a match, far_desc or skip, else -1)."""
    r = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    scale, sigma2 = level_tables(n_levels, scale_factor)
    inv_sigma2 = (np.float32(1.0) / f32(sigma2)).astype(np.float64)
    log_sf = float(np.float32(np.log(np.float32(scale_factor))))
    K = f32([0.72 * width, 0.72 * width, 0.5 * width - 0.5, 0.5 * height - 0.5]).astype(np.float64)
    Rm = so3_exp(r.normal(size=3) * 0.4)
    Cw = r.uniform(-2, 2, 3)
    Rcw = f32(Rm).astype(np.float64)
    tcw = f32(-(Rcw @ Cw)).astype(np.float64)
    Ow = (-(f32(Rcw).T @ f32(tcw))).astype(np.float64)                      # GetCameraCenter in float32
    bounds = np.array([0.0, float(width), 0.0, float(height)])
    inv_w = float(np.float32(cols) / np.float32(bounds[1] - bounds[0]))
    inv_h = float(np.float32(rows) / np.float32(bounds[3] - bounds[2]))
    uv = f32(np.stack([r.uniform(0, width - 1, n_keys), r.uniform(0, height - 1, n_keys)], axis=1)).astype(np.float64)
    oct_p = np.array([35, 25, 15, 10, 6, 4, 3, 2] + [1] * 56)[:n_levels].astype(float)
    octv = r.choice(n_levels, size=n_keys, p=oct_p / oct_p.sum()).astype(np.uint8)
    desc = r.integers(0, 256, (n_keys, 32), dtype=np.uint8)
    cell_begin, cell_feat = abi.grid_csr(uv, bounds, cols, rows, inv_w, inv_h)

    kind = r.choice(len(FUSE_KINDS), size=n_pt, p=np.asarray(mix, dtype=float) / np.sum(mix))
    free = list(r.permutation(n_keys))
    key = np.full(n_pt, -1)
    pos, normal = np.zeros((n_pt, 3)), np.zeros((n_pt, 3))
    dmin, dmax, pmax = np.zeros(n_pt), np.zeros(n_pt), np.zeros(n_pt)
    pdesc = r.integers(0, 256, (n_pt, 32), dtype=np.uint8)
    skip = np.zeros(n_pt, dtype=np.uint8)
    top = np.float32(scale[n_levels - 1])
    for i in range(n_pt):
        kd = FUSE_KINDS[kind[i]]
        depth = r.uniform(2, 10)
        lev = int(r.choice(n_levels, p=oct_p / oct_p.sum()))
        px = np.array([r.uniform(0, width - 1), r.uniform(0, height - 1)])
        if kd in ("match", "far_desc", "skip") and n_keys > 0:
            if not free:
                free = list(r.permutation(n_keys))                            # a second round: two points of the call share a keypoint
            k = int(free.pop())
            key[i] = k
            lev = int(octv[k])
            px = uv[k] + r.normal(size=2) * noise * scale[lev]
            bits = np.unpackbits(desc[k])
            which = r.permutation(256)[:90 if kd == "far_desc" else flip_bits]
            bits[which] ^= 1
            pdesc[i] = np.packbits(bits)
        if kd == "behind":
            depth = -depth
        if kd == "outside":
            px = np.array([width + r.uniform(5, 200), r.uniform(0, height - 1)]) if r.random() < 0.5 else np.array([r.uniform(0, width - 1), -r.uniform(5, 200)])
        Xc = depth * np.array([(px[0] - K[2]) / K[0], (px[1] - K[3]) / K[1], 1.0])
        Xw = f32(Rm.T @ Xc + Cw).astype(np.float64)
        off = r.normal(size=3)
        Cref = Cw + off / np.linalg.norm(off) * r.uniform(0.1, 0.5)
        if kd == "angle":
            Cref = Xw + (Xw - Cw) * r.uniform(1.0, 1.2)                       # the reference view looks at it from the other side
        dref = np.linalg.norm(Xw - Cref)
        mx = np.float32(dref) * np.float32(scale[lev])                         # UpdateNormalAndDepth
        if kd == "distance":
            mx = np.float32(dref) * np.float32(r.choice([0.3, 3.0 * float(top)]))   # the range ends below or starts above the point
        if kd == "level_high":
            mx = np.float32(np.linalg.norm(Xw - Ow) / r.uniform(0.84, 0.99)) * top   # dist3D = 0.84 .. 0.99 of mfMinDistance
        mn = mx / top
        pos[i], normal[i] = Xw, f32((Xw - Cref) / dref)
        pmax[i], dmax[i], dmin[i] = mx, np.float32(1.2) * mx, np.float32(0.8) * mn
        skip[i] = kd == "skip"
    return abi.FuseProblem(Rcw=Rcw, tcw=tcw, Ow=Ow, K=K, bounds=bounds, desc=desc, uv=uv, oct=octv, scale=scale, inv_level_sigma2=inv_sigma2,
                           log_scale_factor=log_sf, grid_cols=cols, grid_rows=rows, grid_inv_w=inv_w, grid_inv_h=inv_h, cell_begin=cell_begin,
                           cell_feat=cell_feat, pos=pos, normal=normal, dist_min=dmin, dist_max=dmax, pred_max=pmax, pt_desc=pdesc, skip=skip,
                           th=th, th_low=th_low, check_reproj=check_reproj, truth=dict(kind=kind, key=key))


# ---------------------------------------------------------------- Sim3 projection matching (vba_search_by_sim3)
SIM3_SEARCH_KINDS = ("match", "matched", "no_pt1", "no_pt2", "far_desc", "behind", "outside", "distance", "level_high")


def sim3_search_scene(seed, n_keys1=1000, n_keys2=1000, n_common=400, n_levels=(8, 8), scale_factor=1.2, flip_bits=12, size=((640, 480), (640, 480)),
                      grid=((64, 48), (64, 48)), mix=(0.6, 0.08, 0.04, 0.04, 0.05, 0.04, 0.05, 0.05, 0.05), noise=0.4, s12=1.1, th=7.5, th_high=100,
                      extra_points=0.15):
    """One ORBmatcher::SearchBySim3 call, every input rounded through float32 as the reference holds it.  Two keyframes with
    different poses, images of size[k] pixels with grids of grid[k] cells and n_levels[k] levels, one pinhole camera (that of
    keyframe 1, used in both directions as the reference does), and a Sim3 with s12 != 1 (p_c1 = s12 R12 p_c2 + t12; log(s12) must
    not be a multiple of log(scale_factor)).  n_common physical features are each present as ONE MAP POINT PER KEYFRAME: the point
    of keyframe 2 lies at a random pixel of image 2, 2-10 deep, and the point of keyframe 1 is that point pushed through the Sim3,
    so the two map copies disagree in world space as they do before a loop is closed.  Each keyframe has a keypoint at the
    projection of its own point plus noise pixels times its level's scale; the two keypoint descriptors are flip_bits apart and
    each point's descriptor is that of its own keypoint.  Octaves: oct2 = oct1 + ceil(log(s12) / log(scale_factor)) - 1 and
    mfMaxDistance = distance * scale[oct] * factor^e with e drawn so that both predicted levels accept the other keypoint.
    Every feature is of one kind, with the shares of `mix` (SIM3_SEARCH_KINDS):
      match       as above;  matched  the same, already matched (vbAlreadyMatched set on both sides)
      no_pt1      keyframe 1 has no usable point on its keypoint;  no_pt2  keyframe 2 has none
      far_desc    the two keypoint descriptors are 120 bits apart
      behind      behind both cameras;  outside  in front but 80-200 pixels out of both images
      distance    distance ranges that do not hold the points
      level_high  mfMaxDistance = distance in the target * factor^(n_levels of the target - 0.5): the predicted level is the
                  target's n_levels (state 6 when the source has at least as many levels; otherwise the range gate catches it)
    The other keypoints of both keyframes are distractors at random pixels with random descriptors; a share extra_points of them
    carries a random map point.  truth: kind [n_common] (index into SIM3_SEARCH_KINDS), key1 / key2 [n_common] (the feature's
    keypoint in each keyframe)."""
    r = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    f64 = lambda a: f32(a).astype(np.float64)
    n_keys = (n_keys1, n_keys2)
    n_common = min(n_common, n_keys1, n_keys2)
    logsf = float(np.log(scale_factor))
    log_sf = float(np.float32(np.log(np.float32(scale_factor))))
    (w1, h1) = size[0]
    K = f64([0.72 * w1, 0.72 * w1, 0.5 * w1 - 0.5, 0.5 * h1 - 0.5])
    scales = [level_tables(n_levels[k], scale_factor)[0] for k in range(2)]
    Rm = [so3_exp(r.normal(size=3) * 0.4) for _ in range(2)]
    Cw = [r.uniform(-2, 2, 3) for _ in range(2)]
    Rcw = [f64(Rm[k]) for k in range(2)]
    tcw = [f64(-(Rcw[k] @ Cw[k])) for k in range(2)]
    s12 = float(np.float32(s12))
    R12 = f64(so3_exp(r.normal(size=3) * 0.02))
    t12 = f64(r.normal(size=3) * 0.05)
    delta = np.log(s12) / logsf
    kshift = int(np.ceil(delta)) - 1
    frac = delta - kshift

    kind = r.choice(len(SIM3_SEARCH_KINDS), size=n_common, p=np.asarray(mix, dtype=float) / np.sum(mix))
    perm = [r.permutation(n_keys[k]) for k in range(2)]
    key = [perm[k][:n_common] for k in range(2)]
    uv = [np.stack([r.uniform(0, size[k][0] - 1, n_keys[k]), r.uniform(0, size[k][1] - 1, n_keys[k])], axis=1) for k in range(2)]
    desc = [r.integers(0, 256, (n_keys[k], 32), dtype=np.uint8) for k in range(2)]
    octv = []
    for k in range(2):
        oct_p = np.array([35, 25, 15, 10, 6, 4, 3, 2] + [1] * 56)[:n_levels[k]].astype(float)
        octv.append(r.choice(n_levels[k], size=n_keys[k], p=oct_p / oct_p.sum()).astype(np.uint8))
    has = [(r.random(n_keys[k]) < extra_points).astype(np.uint8) for k in range(2)]
    matched = [np.zeros(n_keys[k], dtype=np.uint8) for k in range(2)]
    pos = [np.zeros((n_keys[k], 3)) for k in range(2)]
    dmin, dmax, pmax = ([np.zeros(n_keys[k]) for k in range(2)] for _ in range(3))
    pdesc = [r.integers(0, 256, (n_keys[k], 32), dtype=np.uint8) for k in range(2)]
    tops = [np.float32(scales[k][-1]) for k in range(2)]

    def ray(px):
        return np.array([(px[0] - K[2]) / K[0], (px[1] - K[3]) / K[1], 1.0])

    def project(c):
        return np.array([K[0] * c[0] / c[2] + K[2], K[1] * c[1] / c[2] + K[3]])

    def set_point(k, i, c, mx):
        """the map point of keypoint i of keyframe k at c in its camera, with mfMaxDistance mx"""
        pos[k][i] = f64(Rm[k].T @ c + Cw[k])
        mx = np.float32(mx)
        pmax[k][i], dmax[k][i], dmin[k][i] = mx, np.float32(1.2) * mx, np.float32(0.8) * (mx / tops[k])

    # the distractors' points: a random pixel and depth in their own camera, seen at their keypoint's octave
    for k in range(2):
        for i in np.nonzero(has[k])[0]:
            c = r.uniform(2, 10) * ray(uv[k][i] + r.normal(size=2) * 3)
            set_point(k, i, c, np.linalg.norm(c) * scales[k][octv[k][i]])

    lo, hi = max(0, -kshift), min(n_levels[0] - 2, n_levels[1] - 2 - kshift)
    for f in range(n_common):
        kd = SIM3_SEARCH_KINDS[kind[f]]
        i1, i2 = int(key[0][f]), int(key[1][f])
        o1 = int(r.integers(lo, max(lo, min(hi, 3)) + 1))
        o2 = min(max(o1 + kshift, 0), n_levels[1] - 1)
        octv[0][i1], octv[1][i2] = o1, o2
        depth = r.uniform(2, 10)
        px2 = np.array([r.uniform(30, size[1][0] - 31), r.uniform(30, size[1][1] - 31)])
        if kd == "outside":
            off = r.uniform(80, 200)
            px2 = np.array([max(size[0][0], size[1][0]) + off, px2[1]]) if r.random() < 0.5 else np.array([px2[0], -off])
        if kd == "behind":
            depth = -depth
        c2 = depth * ray(px2)
        c1 = s12 * (R12 @ c2) + t12
        d1, d2 = np.linalg.norm(c1), np.linalg.norm(c2)
        mx1 = d1 * scales[0][o1] * scale_factor ** (-frac + r.uniform(-0.35, 0.35))
        mx2 = d2 * scales[1][o2] * scale_factor ** (frac + r.uniform(-0.35, 0.35))
        if kd == "distance":
            far = r.random() < 0.5
            mx1 = d2 * (3.0 * float(tops[0]) if far else 0.3)                # the range ends below or starts above the point
            mx2 = d1 * (3.0 * float(tops[1]) if far else 0.3)
        if kd == "level_high":
            mx1 = d2 * scale_factor ** (n_levels[1] - 0.5)
            mx2 = d1 * scale_factor ** (n_levels[0] - 0.5)
        set_point(0, i1, c1, mx1)
        set_point(1, i2, c2, mx2)
        has[0][i1], has[1][i2] = kd != "no_pt1", kd != "no_pt2"
        if kd == "matched":
            matched[0][i1] = matched[1][i2] = 1
        if kd not in ("behind", "outside"):
            uv[0][i1] = project(c1) + r.normal(size=2) * noise * scales[0][o1]
            uv[1][i2] = project(c2) + r.normal(size=2) * noise * scales[1][o2]
        bits = np.unpackbits(desc[0][i1])
        bits[r.permutation(256)[:120 if kd == "far_desc" else flip_bits]] ^= 1
        desc[1][i2] = np.packbits(bits)
        pdesc[0][i1], pdesc[1][i2] = desc[0][i1], desc[1][i2]

    kfs = []
    for k in range(2):
        w, h = size[k]
        cols, rows = grid[k]
        bounds = np.array([0.0, float(w), 0.0, float(h)])
        inv_w, inv_h = float(np.float32(cols) / np.float32(w)), float(np.float32(rows) / np.float32(h))
        uvk = f64(uv[k])
        cb, cf = abi.grid_csr(uvk, bounds, cols, rows, inv_w, inv_h)
        kfs.append(abi.SearchSim3KF(Rcw=Rcw[k], tcw=tcw[k], bounds=bounds, desc=desc[k], uv=uvk, oct=octv[k], scale=scales[k], log_scale_factor=log_sf,
                                    grid_cols=cols, grid_rows=rows, grid_inv_w=inv_w, grid_inv_h=inv_h, cell_begin=cb, cell_feat=cf, has_pt=has[k],
                                    matched=matched[k], pos=pos[k], dist_min=dmin[k], dist_max=dmax[k], pred_max=pmax[k], pt_desc=pdesc[k]))
    return abi.SearchSim3Problem(kf1=kfs[0], kf2=kfs[1], K=K, s12=s12, R12=R12, t12=t12, th=th, th_high=th_high,
                                 truth=dict(kind=kind, key1=key[0].copy(), key2=key[1].copy()))


# ---------------------------------------------------------------- projection matching for tracking (vba_search_by_projection)
def search_proj_scene(seed, mode, n_keys=1000, n_q=600, twins=0.3, occupied=0.1, non_blocking=0.1, th=None, th_high=100, nn_ratio=0.8,
                      check_orientation=True, rotation=20.0, angle_noise=3.0, angle_outliers=0.1, **kw):
    """One call of a tracking matcher (abi.SearchProjProblem of `mode`), every input rounded through float32 as the reference holds
    it.  The frame and the queries are those of fuse_scene(seed, n_keys, n_q, **kw) -- a query of kind match projects near a keypoint
    whose descriptor it nearly has, and with more matching queries than keypoints several queries want the same keypoint --, with what
    the two matchers add:
      twins         the last share `twins` of the keypoints are moved beside keypoint 0, 1, ...: up to 1.5 pixels away, the same
                    octave, the descriptor 2-10 bits off.  A query that finds its keypoint taken then has a second candidate under
                    th_high, and best and second best of the local-map mode lie close (the ratio test decides)
      occupied      a random share of the keypoints held a point with observations before the call
      non_blocking  a random share of the queries has Observations() == 0: its claim does not block
      last frame    q_oct is the keypoint's octave for a match (one level off for a fifth of them), random otherwise; keypoint angles
                    are uniform in [0, 360), a match's q_angle is its keypoint's plus `rotation` plus angle_noise degrees of noise, a
                    share angle_outliers of them and every other query has a random one.  th defaults to 15 (Tracking.cpp:1754)
      local map     th defaults to 1 (Tracking.cpp:2163)
    truth: that of fuse_scene."""
    f = fuse_scene(seed, n_keys=n_keys, n_pt=n_q, **kw)
    r = np.random.default_rng(seed + 7919)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    desc, uv, octv = f.desc.copy(), f.uv.copy(), f.oct.copy()
    m = min(int(n_keys * twins), n_keys // 2)
    w, h = f.bounds[1], f.bounds[3]
    for j in range(m):
        k = n_keys - m + j
        uv[k] = f32(np.clip(uv[j] + r.uniform(-1.5, 1.5, 2), 0.0, [w - 1.0, h - 1.0])).astype(np.float64)
        octv[k] = octv[j]
        bits = np.unpackbits(desc[j])
        bits[r.permutation(256)[:int(r.integers(2, 11))]] ^= 1
        desc[k] = np.packbits(bits)
    cell_begin, cell_feat = abi.grid_csr(uv, f.bounds, f.grid_cols, f.grid_rows, f.grid_inv_w, f.grid_inv_h)
    occ = (r.random(n_keys) < occupied).astype(np.uint8)
    blocks = (r.random(n_q) >= non_blocking).astype(np.uint8)
    common = dict(Rcw=f.Rcw, tcw=f.tcw, K=f.K, bounds=f.bounds, desc=desc, uv=uv, oct=octv, scale=f.scale, grid_cols=f.grid_cols, grid_rows=f.grid_rows,
                  grid_inv_w=f.grid_inv_w, grid_inv_h=f.grid_inv_h, cell_begin=cell_begin, cell_feat=cell_feat, occupied=occ, q_pos=f.pos, q_desc=f.pt_desc,
                  q_skip=f.skip, q_blocks=blocks, th_high=th_high, truth=f.truth)
    if mode == abi.SEARCH_PROJ_LOCAL_MAP:
        return abi.SearchProjProblem(mode=mode, Ow=f.Ow, log_scale_factor=f.log_scale_factor, q_normal=f.normal, q_dist_min=f.dist_min, q_dist_max=f.dist_max,
                                     q_pred_max=f.pred_max, th=1.0 if th is None else th, nn_ratio=nn_ratio, cos_view=0.5, **common)
    key = f.truth["key"]
    angle = f32(r.uniform(0.0, 360.0, n_keys))
    angle[angle >= 360.0] = 0.0
    q_oct = r.integers(0, f.n_levels, n_q).astype(np.uint8)
    q_angle = f32(r.uniform(0.0, 360.0, n_q))
    for i in range(n_q):
        if key[i] >= 0:
            o = int(f.oct[key[i]]) + (int(r.choice([-1, 1])) if r.random() < 0.2 else 0)
            q_oct[i] = min(max(o, 0), f.n_levels - 1)
            if r.random() >= angle_outliers:
                q_angle[i] = np.float32(np.mod(float(angle[key[i]]) + rotation + r.normal() * angle_noise, 360.0))
    q_angle[q_angle >= 360.0] = 0.0
    return abi.SearchProjProblem(mode=mode, angle=angle, q_oct=q_oct, q_angle=q_angle, th=15.0 if th is None else th,
                                 check_orientation=check_orientation, **common)


# ---------------------------------------------------------------- loop-closure / relocalisation projection matching (vba_search_by_projection_kf)
def search_proj_kf_scene(seed, mode, n_keys=1000, n_q=600, twins=0.3, occupied=0.1, th=10.0, th_dist=None, behind=0.1, check_orientation=True,
                         rotation=20.0, angle_noise=3.0, angle_outliers=0.1, **kw):
    """One call of the loop-closure or the relocalisation matcher (abi.SearchProjKfProblem of `mode`), every input rounded through
    float32 as the reference holds it.  The target, the queries, the twins (contention) and the occupied share are those of
    search_proj_scene(seed, SEARCH_PROJ_LOCAL_MAP, ...), which is built on fuse_scene; every query blocks.  th_dist defaults to TH_LOW = 50
    in loop mode and to ORBdist = 100 in reloc mode.  Reloc mode adds
      behind        a share of the queries of kind match is mirrored through the camera centre: the point lies behind the camera at
                    the same distance and projects to the same pixel, so it passes every gate of the mode and can match
      angles        keypoint angles are uniform in [0, 360), a match's q_angle is its keypoint's plus `rotation` plus angle_noise
                    degrees of noise, a share angle_outliers of them and every other query has a random one
    truth: that of fuse_scene, and behind [n_q] in reloc mode."""
    reloc = mode == abi.SEARCH_PROJ_KF_RELOC
    g = search_proj_scene(seed, abi.SEARCH_PROJ_LOCAL_MAP, n_keys=n_keys, n_q=n_q, twins=twins, occupied=occupied, non_blocking=0.0, **kw)
    r = np.random.default_rng(seed + 104729)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    common = dict(mode=mode, Rcw=g.Rcw, tcw=g.tcw, Ow=g.Ow, K=g.K, bounds=g.bounds, desc=g.desc, uv=g.uv, oct=g.oct, scale=g.scale,
                  log_scale_factor=g.log_scale_factor, grid_cols=g.grid_cols, grid_rows=g.grid_rows, grid_inv_w=g.grid_inv_w, grid_inv_h=g.grid_inv_h,
                  cell_begin=g.cell_begin, cell_feat=g.cell_feat, occupied=g.occupied, q_desc=g.q_desc, q_skip=g.q_skip, q_dist_min=g.q_dist_min,
                  q_dist_max=g.q_dist_max, q_pred_max=g.q_pred_max, th=th)
    if not reloc:
        return abi.SearchProjKfProblem(q_pos=g.q_pos, q_normal=g.q_normal, th_dist=50 if th_dist is None else th_dist, cos_view=0.5, truth=g.truth, **common)
    key, kind = g.truth["key"], g.truth["kind"]
    pos = g.q_pos.copy()
    is_behind = np.zeros(n_q, dtype=bool)
    for i in range(n_q):
        if FUSE_KINDS[kind[i]] == "match" and r.random() < behind:
            xc = g.Rcw @ pos[i] + g.tcw
            pos[i] = f32(g.Rcw.T @ (-xc - g.tcw)).astype(np.float64)
            is_behind[i] = True
    angle = f32(r.uniform(0.0, 360.0, n_keys))
    angle[angle >= 360.0] = 0.0
    q_angle = f32(r.uniform(0.0, 360.0, n_q))
    for i in range(n_q):
        if key[i] >= 0 and r.random() >= angle_outliers:
            q_angle[i] = np.float32(np.mod(float(angle[key[i]]) + rotation + r.normal() * angle_noise, 360.0))
    q_angle[q_angle >= 360.0] = 0.0
    return abi.SearchProjKfProblem(q_pos=pos, angle=angle, q_angle=q_angle, th_dist=100 if th_dist is None else th_dist,
                                   check_orientation=check_orientation, truth=dict(g.truth, behind=is_behind), **common)


# ---------------------------------------------------------------- bag-of-words matching (vba_search_by_bow)
def search_bow_scene(seed, mode, n_keys1=1500, n_keys2=1500, n_nodes=100, twins=0.6, flip_bits=12, near_dup=0.15, unshared=0.1, mp1=0.7, mp2=0.8,
                     th_low=50, nn_ratio=0.75, check_orientation=True, rotation=25.0, angle_noise=3.0, angle_outliers=0.1):
    """One ORBmatcher::SearchByBoW call (abi.SearchBowProblem of `mode`).
      twins         the first share `twins` of min(n_keys1, n_keys2) keypoints exist on both sides: the descriptor of side 2 is the one
                    of side 1 with up to flip_bits bits flipped, and both lie in the same vocabulary node (a share `unshared` of them
                    is moved to another node on side 2).  The rest are strangers with random descriptors and random nodes
      near_dup      a share of the keypoints of side 1 is overwritten with the descriptor of an EARLIER keypoint of its node, 0-4 bits
                    off, so that several queries of a node want the same keypoint of side 2 (contention, ratio-test flips)
      nodes         ids 10 k + 5 on both sides, 10 k + 1 on side 1 only, 10 k + 8 on side 2 only; the order inside a node is shuffled
      mp1, mp2      shares of keypoints with a good map point (side 2: read in KF_KF mode only)
      angles        uniform on side 1; a twin's angle on side 2 is that of side 1 minus `rotation` plus noise, random for outliers
    Keypoint indices are shuffled on both sides.  truth: pair [n_twins, 2], the indices of every twin on both sides."""
    r = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    nt = int(min(n_keys1, n_keys2) * twins)

    def flipped(dsc, lo, hi):
        out = np.unpackbits(dsc, axis=1)
        for row in out:
            row[r.permutation(256)[:int(r.integers(lo, hi + 1))]] ^= 1
        return np.packbits(out, axis=1).reshape(-1, 32)

    d1 = r.integers(0, 256, (n_keys1, 32), dtype=np.uint8)
    node1 = 10 * r.integers(0, max(n_nodes, 1), n_keys1) + np.where(r.random(n_keys1) < 0.1, 1, 5)
    node1[:nt] = node1[:nt] // 10 * 10 + 5
    for i in range(n_keys1):
        if r.random() < near_dup:
            same = np.nonzero(node1[:i] == node1[i])[0]
            if len(same):
                d1[i] = flipped(d1[same[int(r.integers(len(same)))]][None], 0, 4)[0]
    d2 = r.integers(0, 256, (n_keys2, 32), dtype=np.uint8)
    node2 = 10 * r.integers(0, max(n_nodes, 1), n_keys2) + np.where(r.random(n_keys2) < 0.1, 8, 5)
    if nt:
        d2[:nt] = flipped(d1[:nt], 0, flip_bits)
        moved = r.random(nt) < unshared
        node2[:nt] = np.where(moved, 10 * ((node1[:nt] // 10 + 1) % max(n_nodes, 1)) + 5, node1[:nt])
    ang1 = r.uniform(0, 360, n_keys1)
    ang2 = r.uniform(0, 360, n_keys2)
    keep = r.random(nt) >= angle_outliers
    ang2[:nt] = np.where(keep, np.mod(ang1[:nt] - rotation + r.normal(size=nt) * angle_noise, 360.0), ang2[:nt])
    ang1, ang2 = f32(ang1), f32(ang2)
    ang1[ang1 >= 360] = 0; ang2[ang2 >= 360] = 0
    good1 = (r.random(n_keys1) < mp1).astype(np.uint8)
    good2 = (r.random(n_keys2) < mp2).astype(np.uint8)
    p1, p2 = r.permutation(n_keys1), r.permutation(n_keys2)          # new index -> old index
    inv1, inv2 = np.argsort(p1), np.argsort(p2)

    def fv(node, perm):
        m = {}
        for new in r.permutation(len(perm)):                       # the order inside a node is not ascending
            m.setdefault(int(node[perm[new]]), []).append(int(new))
        return abi.feat_vec_csr(m)

    id1, b1, ft1 = fv(node1, p1)
    id2, b2, ft2 = fv(node2, p2)
    return abi.SearchBowProblem(mode=mode, desc1=d1[p1], desc2=d2[p2], good_mp1=good1[p1], good_mp2=good2[p2] if mode == abi.SEARCH_BOW_KF_KF else None,
                                node_id1=id1, node_begin1=b1, node_feat1=ft1, node_id2=id2, node_begin2=b2, node_feat2=ft2,
                                angle1=ang1[p1] if check_orientation else None, angle2=ang2[p2] if check_orientation else None, th_low=th_low,
                                nn_ratio=nn_ratio, check_orientation=check_orientation, truth=dict(pair=np.stack([inv1[:nt], inv2[:nt]], axis=1)))


# ---------------------------------------------------------------- matching for the monocular initialisation (vba_search_for_initialization)
def search_init_scene(seed, n_keys1=1500, n_keys2=1500, size=(640, 480), cols=64, rows=48, window_size=100.0, level0=0.6, matched=0.7, twins=0.2,
                      crowd=0.3, flip_bits=24, spread=0.6, th_low=50, nn_ratio=0.9, check_orientation=True, rotation=20.0, angle_noise=3.0,
                      angle_outliers=0.1):
    """One ORBmatcher::SearchForInitialization call (abi.SearchInitProblem), every input as the reference holds it (float32 pixels).
      pixels      off the integer lattice: a keypoint of frame 2 lies on (integer + an odd multiple of 1/8), a vbPrevMatched entry on
                  (integer + an odd multiple of 1/4), so with an integer window no |dx| sits on r and no floor or ceil argument on an integer
      level0      the share of the keypoints of either frame at octave 0; the others are spread over the octaves 1 .. 7
      matched     the first share `matched` of min(n_keys1, n_keys2) keypoints of frame 1 are views of keypoint i of frame 2: the
                  descriptor 0 .. flip_bits bits off, vbPrevMatched within spread * window_size of it, the same octave
      twins       the last share of the keypoints of frame 2 are moved beside keypoint 0, 1, ...: up to 3 pixels away, the same octave,
                  the descriptor 2 .. 10 bits off: best and second best lie close, and the ratio test decides
      crowd       the last share of the keypoints of frame 1 are second views of the keypoints 0, 1, ... of frame 1 (the descriptor up
                  to 6 bits off theirs, vbPrevMatched drawn anew around the same keypoint of frame 2): queries compete for a keypoint, and
                  the later one steals it when it is strictly nearer
      angles      uniform in frame 2; a view's angle1 is its keypoint's plus `rotation` plus angle_noise degrees of noise, a share
                  angle_outliers of the views and every other keypoint has a random one
    Both frames are shuffled at the end.  truth: key1 [n_keys1], the keypoint of frame 2 a keypoint of frame 1 is a view of, -1 for none."""
    r = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    w, h = size
    bounds = np.array([0.0, float(w), 0.0, float(h)])

    def octaves(n):
        return np.where(r.random(n) < level0, 0, r.integers(1, 8, n)).astype(np.uint8)

    def flipped(d, lo, hi):
        bits = np.unpackbits(d)
        bits[r.permutation(256)[:int(r.integers(lo, hi + 1))]] ^= 1
        return np.packbits(bits)

    lat8 = lambda n, top: r.integers(0, max(int(top) - 1, 1), n) + (2 * r.integers(0, 4, n) + 1) / 8.0
    uv2 = np.stack([lat8(n_keys2, w), lat8(n_keys2, h)], axis=1).reshape(-1, 2)
    oct2 = octaves(n_keys2)
    d2 = r.integers(0, 256, (n_keys2, 32), dtype=np.uint8)
    m2 = min(int(n_keys2 * twins), n_keys2 // 2)
    for j in range(m2):
        k = n_keys2 - m2 + j
        uv2[k] = np.clip(uv2[j] + r.integers(-3, 4, 2), 0.125, [w - 0.125, h - 0.125])
        oct2[k] = oct2[j]
        d2[k] = flipped(d2[j], 2, 10)
    ang2 = r.uniform(0.0, 360.0, n_keys2)

    def around(k):
        reach = max(int(abs(window_size) * spread), 1)
        c = np.floor(uv2[k]) + r.integers(-reach, reach + 1, 2) + (2 * r.integers(0, 2, 2) + 1) / 4.0
        return np.clip(c, 0.25, [w - 0.25, h - 0.25])

    key1 = np.full(n_keys1, -1, dtype=np.int64)
    oct1 = octaves(n_keys1)
    d1 = r.integers(0, 256, (n_keys1, 32), dtype=np.uint8)
    prev = np.stack([r.integers(0, max(w - 1, 1), n_keys1), r.integers(0, max(h - 1, 1), n_keys1)], axis=1).reshape(-1, 2) + (2 * r.integers(0, 2, (n_keys1, 2)) + 1) / 4.0
    ang1 = r.uniform(0.0, 360.0, n_keys1)
    nm = int(min(n_keys1, n_keys2 - m2) * matched)
    for i in range(nm):
        key1[i], oct1[i], d1[i], prev[i] = i, oct2[i], flipped(d2[i], 0, flip_bits), around(i)
    mc = min(int(n_keys1 * crowd), n_keys1 - nm, nm)
    for j in range(mc):
        i, src = n_keys1 - mc + j, j % max(nm, 1)
        key1[i], oct1[i], d1[i], prev[i] = key1[src], oct1[src], flipped(d1[src], 0, 6), around(key1[src])
    for i in np.nonzero(key1 >= 0)[0]:
        if r.random() >= angle_outliers:
            ang1[i] = np.mod(ang2[key1[i]] + rotation + r.normal() * angle_noise, 360.0)
    ang1, ang2 = f32(ang1), f32(ang2)
    ang1[ang1 >= 360] = 0; ang2[ang2 >= 360] = 0
    p1, p2 = r.permutation(n_keys1), r.permutation(n_keys2)          # new index -> old index
    inv2 = np.argsort(p2)
    uv2 = f32(uv2[p2]).astype(np.float64).reshape(-1, 2)
    inv_w, inv_h = float(np.float32(cols) / np.float32(w)), float(np.float32(rows) / np.float32(h))
    cell_begin, cell_feat = abi.grid_csr(uv2, bounds, cols, rows, inv_w, inv_h)
    k1 = key1[p1]
    return abi.SearchInitProblem(desc1=d1[p1], oct1=oct1[p1], prev_matched=f32(prev[p1]), desc2=d2[p2], uv2=uv2, oct2=oct2[p2], bounds=bounds, grid_cols=cols,
                                 grid_rows=rows, grid_inv_w=inv_w, grid_inv_h=inv_h, cell_begin=cell_begin, cell_feat=cell_feat,
                                 angle1=ang1[p1] if check_orientation else None, angle2=ang2[p2] if check_orientation else None,
                                 window_size=window_size, th_low=th_low, nn_ratio=nn_ratio, check_orientation=check_orientation,
                                 truth=dict(key1=np.where(k1 >= 0, inv2[np.maximum(k1, 0)], -1) if n_keys2 else k1))
