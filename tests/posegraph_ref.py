"""NumPy restatement of the reference's essential-graph optimisation -- TEST INFRASTRUCTURE, the yardstick of the pose-graph tests.

The reference (Optimizer::OptimizeEssentialGraph, src/Optimizer.cpp:4243-4552, with g2o's VertexSim3Expmap / EdgeSim3,
types_seven_dof_expmap.h:48-124, Sim3 of sim3.h:41-292, the numeric Jacobians of base_binary_edge.hpp:131-205, the assembly of
:68-90 and the Levenberg-Marquardt loop of optimization_algorithm_levenberg.cpp:61-164) cannot be compiled here (no Eigen, no
OpenCV), so this file restates it the way tests/sim3_ref.py restates OptimizeSim3.  Nothing of the library is imported: the GPU
kernel k_posegraph_opt (mc_slam_amd/csrc/vba_posegraph.h) is compared WITH this file, never built from it.

    optimize(problem, dtype=np.float64, trace=True) -> result

`problem` is anything with the attributes of mc_slam_amd.abi.PoseGraphProblem (S [n,8] = t(3) q(4, xyzw) s, fixed, edge_i, edge_j,
edge_S, fix_scale, its, lambda_init).  Everything is vectorised over edges / vertices.  `dtype` is the number format of the Sim3
arithmetic, the error function, the central differences and the assembly; the dense solve of H + lambda I is always float64
(LAPACK has no other).  result.trace lists (cost before, cost after, accepted) of every LM trial.

As in sim3_ref.py the quaternion of an update is normalised (Sim3(update) builds Quaterniond(R) and leaves it as it is).
"""
from types import SimpleNamespace

import numpy as np

EPS = 1e-5
DBL_MAX = np.finfo(np.float64).max
DELTA = 1e-9


# ---- Sim3 arithmetic, batched over the leading axis; a Sim3 is the tuple (q [n,4] xyzw, t [n,3], s [n]) ----
def unpack(S, dtype=np.float64):
    S = np.asarray(S, dtype=dtype).reshape(-1, 8)
    return S[:, 3:7].copy(), S[:, :3].copy(), S[:, 7].copy()


def pack(S):
    q, t, s = S
    return np.concatenate([t, q, s[:, None]], axis=1)


def skew(v):
    M = np.zeros(v.shape[:-1] + (3, 3), dtype=v.dtype)
    M[..., 0, 1], M[..., 0, 2] = -v[..., 2], v[..., 1]
    M[..., 1, 0], M[..., 1, 2] = v[..., 2], -v[..., 0]
    M[..., 2, 0], M[..., 2, 1] = -v[..., 1], v[..., 0]
    return M


def q2R(q):
    """Eigen::Quaterniond::toRotationMatrix"""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.empty(q.shape[:-1] + (3, 3), dtype=q.dtype)
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - (tyy + tzz), txy - twz, txz + twy
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = txy + twz, 1 - (txx + tzz), tyz - twx
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = txz - twy, tyz + twx, 1 - (txx + tyy)
    return R


def R2q(m):
    """Eigen's quaternion from a rotation matrix (x y z w), then normalised; one matrix at a time is branchy, so every case is
    computed and the right one selected"""
    n = m.shape[0]
    q = np.zeros((n, 4), dtype=m.dtype)
    tr = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
    i = np.zeros(n, dtype=int)
    i[m[:, 1, 1] > m[:, 0, 0]] = 1
    i[m[:, 2, 2] > m[np.arange(n), i, i]] = 2
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.sqrt(tr + 1.0)
        h = 0.5 / t
        q0 = np.stack([(m[:, 2, 1] - m[:, 1, 2]) * h, (m[:, 0, 2] - m[:, 2, 0]) * h, (m[:, 1, 0] - m[:, 0, 1]) * h, 0.5 * t], axis=1)
        q[:] = q0
        for c in range(3):
            sel = (tr <= 0) & (i == c)
            if not sel.any():
                continue
            a, b, k = c, (c + 1) % 3, (c + 2) % 3
            mm = m[sel]
            t2 = np.sqrt(mm[:, a, a] - mm[:, b, b] - mm[:, k, k] + 1.0)
            h2 = 0.5 / t2
            qq = np.zeros((mm.shape[0], 4), dtype=m.dtype)
            qq[:, a] = 0.5 * t2
            qq[:, 3] = (mm[:, k, b] - mm[:, b, k]) * h2
            qq[:, b] = (mm[:, b, a] + mm[:, a, b]) * h2
            qq[:, k] = (mm[:, k, a] + mm[:, a, k]) * h2
            q[sel] = qq
    return q / np.sqrt((q * q).sum(axis=1))[:, None]


def qmul(a, b):
    return np.stack([a[:, 3] * b[:, 0] + a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 3] * b[:, 1] + a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 3] * b[:, 2] + a[:, 2] * b[:, 3] + a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0],
                     a[:, 3] * b[:, 3] - a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2]], axis=1)


def _mv(M, v):
    return (M * v[:, None, :]).sum(axis=2)


def _abc(theta, sigma, s, small_t, small_s):
    """A, B, C of Sim3(update) and Sim3::log: the four branches on |sigma| < eps and the small-angle test"""
    one = np.ones_like(theta)
    th = np.where(small_t, one, theta)
    sg = np.where(small_s, one, sigma)
    th2, sg2 = th * th, sg * sg
    C = np.where(small_s, one, (s - 1) / sg)
    a, b = s * np.sin(th), s * np.cos(th)
    c = th2 + sg2
    A = np.where(small_s, np.where(small_t, 0.5 * one, (1 - np.cos(th)) / th2),
                 np.where(small_t, ((sg - 1) * s + 1) / sg2, (a * sg + (1 - b) * th) / (th * c)))
    B = np.where(small_s, np.where(small_t, one / 6, (th - np.sin(th)) / (th2 * th)),
                 np.where(small_t, ((0.5 * sg2 - sg + 1) * s) / (sg2 * sg), (C - ((b - 1) * sg + a * th) / c) * 1.0 / th2))
    return A, B, C


def sim3_exp(u, info=None):
    """Sim3(const Vector7d&), sim3.h:70-142, batched: u [n,7] = (omega, upsilon, sigma).  info: dict that receives the branch
    taken per row (0..3: sigma small & theta small, sigma small, theta small, neither)."""
    om, up, sigma = u[:, :3], u[:, 3:6], u[:, 6]
    theta = np.sqrt((om * om).sum(axis=1))
    Om = skew(om)
    Om2 = Om @ Om
    I = np.eye(3, dtype=u.dtype)
    s = np.exp(sigma)
    small_s, small_t = np.abs(sigma) < EPS, theta < EPS
    A, B, C = _abc(theta, sigma, s, small_t, small_s)
    th = np.where(small_t, np.ones_like(theta), theta)
    r1 = np.where(small_t, np.ones_like(theta), np.sin(th) / th)
    r2 = np.where(small_t, np.ones_like(theta), (1 - np.cos(th)) / (th * th))
    R = I + r1[:, None, None] * Om + r2[:, None, None] * Om2
    W = A[:, None, None] * Om + B[:, None, None] * Om2 + C[:, None, None] * I
    if info is not None:
        info["branch"] = np.where(small_s, np.where(small_t, 0, 1), np.where(small_t, 2, 3))
    return R2q(R), _mv(W, up), s


def sim3_mul(a, b):
    """Sim3::operator*, sim3.h:266-272"""
    qa, ta, sa = a
    qb, tb, sb = b
    return qmul(qa, qb), sa[:, None] * _mv(q2R(qa), tb) + ta, sa * sb


def sim3_inv(a):
    """Sim3::inverse, sim3.h:233-236"""
    q, t, s = a
    qc = q * np.array([-1, -1, -1, 1], dtype=q.dtype)
    return qc, _mv(q2R(qc), (-1.0 / s)[:, None] * t), 1.0 / s


def sim3_map(a, p):
    """Sim3::map, sim3.h:144-146"""
    q, t, s = a
    return s[:, None] * _mv(q2R(q), p) + t


def _lu3_solve(W, t):
    """W.lu().solve(t): Eigen's PartialPivLU on a batch of 3x3 systems (first largest |entry| of the column is the pivot)"""
    n = W.shape[0]
    A = np.concatenate([W, t[:, :, None]], axis=2).copy()
    ar = np.arange(n)
    for c in range(2):
        p = c + np.argmax(np.abs(A[:, c:, c]), axis=1)
        rc, rp = A[ar, c].copy(), A[ar, p].copy()
        A[ar, c], A[ar, p] = rp, rc
        for r in range(c + 1, 3):
            l = A[:, r, c] / A[:, c, c]
            A[:, r, c + 1:] -= l[:, None] * A[:, c, c + 1:]
    u = np.zeros((n, 3), dtype=W.dtype)
    u[:, 2] = A[:, 2, 3] / A[:, 2, 2]
    u[:, 1] = (A[:, 1, 3] - A[:, 1, 2] * u[:, 2]) / A[:, 1, 1]
    u[:, 0] = (A[:, 0, 3] - A[:, 0, 1] * u[:, 1] - A[:, 0, 2] * u[:, 2]) / A[:, 0, 0]
    return u


def sim3_log(S, info=None):
    """Sim3::log, sim3.h:148-230, batched: [n,7] = (omega, upsilon, sigma)"""
    q, t, s = S
    sigma = np.log(s)
    R = q2R(q)
    d = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1)
    dR = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    small_s, small_t = np.abs(sigma) < EPS, d > 1 - EPS
    dd = np.where(small_t, np.zeros_like(d), d)              # the small-angle rows take no part in acos / sqrt
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = np.arccos(dd)
        f = np.where(small_t, 0.5 * np.ones_like(d), theta / (2 * np.sqrt(1 - dd * dd)))
        A, B, C = _abc(theta, sigma, s, small_t, small_s)
    om = f[:, None] * dR
    Om = skew(om)
    I = np.eye(3, dtype=om.dtype)
    W = A[:, None, None] * Om + B[:, None, None] * (Om @ Om) + C[:, None, None] * I
    if info is not None:
        info["branch"] = np.where(small_s, np.where(small_t, 0, 1), np.where(small_t, 2, 3))
    return np.concatenate([om, _lu3_solve(W, t), sigma[:, None]], axis=1)


def oplus(S, u, fix_scale):
    """VertexSim3Expmap::oplusImpl, types_seven_dof_expmap.h:60-69"""
    u = np.array(u, dtype=S[0].dtype)
    if fix_scale:
        u[:, 6] = 0.0
    return sim3_mul(sim3_exp(u), S)


def _take(S, idx):
    return S[0][idx], S[1][idx], S[2][idx]


def errors(S, M, ei, ej, Si=None, Sj=None):
    """EdgeSim3::computeError of every edge: log(Sji * Si * Sj^-1), [m,7]"""
    Si = _take(S, ei) if Si is None else Si
    Sj = _take(S, ej) if Sj is None else Sj
    return sim3_log(sim3_mul(sim3_mul(M, Si), sim3_inv(Sj)))


def jacobians(S, M, ei, ej, fix_scale, delta=DELTA):
    """BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:131-205): central differences through oplus; J_i, J_j [m,7,7]"""
    dt = S[0].dtype
    m = len(ei)
    J = [np.zeros((m, 7, 7), dtype=dt), np.zeros((m, 7, 7), dtype=dt)]
    delta = dt.type(delta)
    scalar = dt.type(1.0) / (2 * delta)
    Si, Sj = _take(S, ei), _take(S, ej)
    for side in range(2):
        base = Sj if side else Si
        for k in range(7):
            u = np.zeros((m, 7), dtype=dt)
            u[:, k] = delta
            Sp, Sm = oplus(base, u, fix_scale), oplus(base, -u, fix_scale)
            ep = errors(S, M, ei, ej, Si if side else Sp, Sp if side else Sj)
            em = errors(S, M, ei, ej, Si if side else Sm, Sm if side else Sj)
            J[side][:, :, k] = scalar * (ep - em)
    return J


def build_system(e, Ji, Jj, ei, ej, free_of, nf):
    """BaseBinaryEdge::constructQuadraticForm of every edge in edge order (base_binary_edge.hpp:68-90): dense H [7nf,7nf], b [7nf]"""
    dt = e.dtype
    H4 = np.zeros((nf, nf, 7, 7), dtype=dt)
    b2 = np.zeros((nf, 7), dtype=dt)
    fi, fj = free_of[ei], free_of[ej]
    Hii = np.einsum("mka,mkc->mac", Ji, Ji)
    Hjj = np.einsum("mka,mkc->mac", Jj, Jj)
    Hij = np.einsum("mka,mkc->mac", Ji, Jj)
    bi = -np.einsum("mka,mk->ma", Ji, e)
    bj = -np.einsum("mka,mk->ma", Jj, e)
    a = fi >= 0
    c = fj >= 0
    np.add.at(H4, (fi[a], fi[a]), Hii[a])
    np.add.at(b2, fi[a], bi[a])
    np.add.at(H4, (fj[c], fj[c]), Hjj[c])
    np.add.at(b2, fj[c], bj[c])
    both = a & c
    np.add.at(H4, (fi[both], fj[both]), Hij[both])
    np.add.at(H4, (fj[both], fi[both]), np.transpose(Hij[both], (0, 2, 1)))
    return H4.transpose(0, 2, 1, 3).reshape(7 * nf, 7 * nf), b2.reshape(-1)


def chi2_of(e):
    return float((e * e).sum(axis=1).sum())


def move_points(S0, S1, pt, pt_ref, dtype=np.float64):
    """src/Optimizer.cpp:4511-4546: correctedSwr.map(Srw.map(P)) with the initial (S0) and final (S1) estimates [n,8]"""
    a, b = unpack(S0, dtype), unpack(S1, dtype)
    P = np.asarray(pt, dtype=dtype).reshape(-1, 3)
    return sim3_map(sim3_inv(_take(b, pt_ref)), sim3_map(_take(a, pt_ref), P))


def optimize(pr, dtype=np.float64, trace=True, its=None):
    """optimize(its) of Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:4481-4482) on one graph"""
    dt = np.dtype(dtype)
    S = unpack(pr.S, dt)
    M = unpack(pr.edge_S, dt)
    ei, ej = np.asarray(pr.edge_i, dtype=int), np.asarray(pr.edge_j, dtype=int)
    fixed = np.asarray(pr.fixed).astype(bool)
    fix = bool(pr.fix_scale)
    its = int(pr.its if its is None else its)
    free_of = np.full(len(fixed), -1)
    free_of[~fixed] = np.arange((~fixed).sum())
    vert_of = np.nonzero(~fixed)[0]
    nf = len(vert_of)
    res = SimpleNamespace(status=0, its_done=0, lm_trials=0, stop=0, chi2_initial=0.0, chi2_final=0.0, lambda_final=0.0, trace=[],
                          H0=None, b0=None, x0=None, lambda0=float(pr.lambda_init))
    lam, ni, nb, cj, cur = float(pr.lambda_init), 2.0, 0, 0, 0.0
    for it in range(its):
        e = errors(S, M, ei, ej)
        cur = chi2_of(e)
        ini = cur
        Ji, Jj = jacobians(S, M, ei, ej, fix)
        H, b = build_system(e, Ji, Jj, ei, ej, free_of, nf)
        H, b = H.astype(np.float64), b.astype(np.float64)
        if it == 0:
            res.chi2_initial = cur
            res.H0, res.b0 = H, b
        q = 0
        while True:
            Sbk = S
            ok = True
            try:
                L = np.linalg.cholesky(H + lam * np.eye(7 * nf))     # fails on a non-positive pivot, as the LDL^T check does
                x = np.linalg.solve(L.T, np.linalg.solve(L, b))
            except np.linalg.LinAlgError:
                ok, x = False, np.zeros(7 * nf)
            if not np.all(np.isfinite(x)):
                ok, x = False, np.zeros(7 * nf)
            if res.x0 is None:
                res.x0 = x.copy()
            if ok:
                upd = oplus(_take(S, vert_of), x.reshape(nf, 7).astype(dt), fix)
                S = tuple(a.copy() for a in S)
                for k in range(3):
                    S[k][vert_of] = upd[k]
            tmp = chi2_of(errors(S, M, ei, ej))
            if not ok:
                tmp = DBL_MAX
            rho = cur - tmp
            rho /= float(x @ (lam * x + b)) + 1e-3
            good = rho > 0 and np.isfinite(tmp)
            res.trace.append((cur, tmp, bool(good)))
            if good:
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = tmp
            else:
                lam *= ni
                ni *= 2
                S = Sbk                                  # pop()
            q += 1
            if not (rho < 0 and q < 10):
                break
        cj += 1
        res.lm_trials += q
        if q == 10:
            res.stop = 1
            break
        if rho == 0:
            res.stop = 2
            break
        nb = nb + 1 if (ini - cur) * 1e3 < ini else 0
        if nb >= 3:
            res.stop = 3
            break
    res.its_done, res.chi2_final, res.lambda_final = cj, cur, lam
    res.S = pack(S).astype(np.float64)
    res.S_dt = pack(S)
    return res


def decidable(tr, rel=1e-10):
    """True when every LM trial of the list changed the cost by more than `rel` relative: none was decided by rounding"""
    return all(abs(c0 - c1) > rel * abs(c0) for c0, c1, _ in tr)
