"""NumPy restatement of the reference's loop-closure Sim3 refinement -- TEST INFRASTRUCTURE, the yardstick of the Sim3 tests.

The reference (Optimizer::OptimizeSim3, src/Optimizer.cpp:4579-4785, with g2o's VertexSim3Expmap / EdgeSim3ProjectXYZ /
EdgeInverseSim3ProjectXYZ, types_seven_dof_expmap.h:48-170, Sim3 of sim3.h:41-292 and the Levenberg-Marquardt loop of
optimization_algorithm_levenberg.cpp:61-164) cannot be compiled here (no Eigen, no OpenCV), so this file restates it the
way tests/stage_ref.py restates the Schur stages.  Nothing of the library is imported: the GPU kernel k_sim3_opt
(mc_slam_amd/csrc/vba_sim3.h) is compared WITH this file, never built from it.

    optimize(problem, jac="analytic" | "numeric", trace=False) -> Sim3Ref

`problem` is anything with the attributes of mc_slam_amd.abi.Sim3Problem (S12 = t(3) q(4, xyzw) s, p1c, p2c, uv1, uv2, w1, w2,
K1, K2, th2, huber, fix_scale, its_stage1, its_stage2_bad, its_stage2_clean, min_inliers).
  jac="analytic": the closed-form Jacobians the kernel uses.
  jac="numeric":  what the reference itself does -- central differences with step 1e-9 through oplus (base_binary_edge.hpp:147-148;
                  linearizeOplus of both edges is commented out in the reference).
  trace=True:     Sim3Ref.trace[stage] lists (cost before, cost after, accepted) of every LM trial, so a test can tell a decision
                  taken on a real cost change from one taken on rounding.

Two readings of the reference that matter for parity:
  * chi2() of an edge reads the error g2o STORED at its last computeActiveErrors: when the last LM trial of an optimize() was
    rejected, the vertex is popped back but the stored errors stay those of the rejected trial.  The outlier tests here read
    the same stored values.
  * Sim3(update) builds its rotation as Quaterniond(R).  Here (and in the kernel) that quaternion is normalised, so the estimate
    stays a similarity; the two differ only in the theta < 1e-5 branch, by O(theta^2) <= 1e-10.
"""
from types import SimpleNamespace

import numpy as np

EPS = 1e-5
DBL_MAX = np.finfo(np.float64).max


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def q2R(q):
    """Eigen::Quaterniond::toRotationMatrix, q = x y z w"""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def R2q(m):
    """Eigen's quaternion from a rotation matrix (x y z w), then normalised"""
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q / np.sqrt(q @ q)


def qmul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def sim3_exp(u, info=None):
    """Sim3(const Vector7d&), sim3.h:70-142: (q, t, s) of exp(u), u = (omega, upsilon, sigma).  info: dict that receives the
    branch taken (0..3)."""
    u = np.asarray(u, dtype=np.float64)
    om, up, sg = u[:3], u[3:6], float(u[6])
    th = float(np.sqrt(om @ om))
    Om = skew(om)
    Om2 = Om @ Om
    I = np.eye(3)
    s = float(np.exp(sg))
    if abs(sg) < EPS:
        C = 1.0
        if th < EPS:
            branch, A, B = 0, 0.5, 1.0 / 6.0
            R = I + Om + Om2
        else:
            branch = 1
            th2 = th * th
            A = (1 - np.cos(th)) / th2
            B = (th - np.sin(th)) / (th2 * th)
            R = I + np.sin(th) / th * Om + (1 - np.cos(th)) / (th * th) * Om2
    else:
        C = (s - 1) / sg
        if th < EPS:
            branch = 2
            sg2 = sg * sg
            A = ((sg - 1) * s + 1) / sg2
            B = ((0.5 * sg2 - sg + 1) * s) / (sg2 * sg)
            R = I + Om + Om2
        else:
            branch = 3
            R = I + np.sin(th) / th * Om + (1 - np.cos(th)) / (th * th) * Om2
            a, b = s * np.sin(th), s * np.cos(th)
            th2, sg2 = th * th, sg * sg
            c = th2 + sg2
            A = (a * sg + (1 - b) * th) / (th * c)
            B = (C - ((b - 1) * sg + a * th) / c) * 1.0 / th2
    if info is not None:
        info["branch"] = branch
    W = A * Om + B * Om2 + C * I
    return R2q(R), W @ up, s


def sim3_mul(a, b):
    """Sim3::operator*, sim3.h:266-272"""
    qa, ta, sa = a
    qb, tb, sb = b
    return qmul(qa, qb), sa * (q2R(qa) @ tb) + ta, sa * sb


def oplus(S, u, fix_scale):
    """VertexSim3Expmap::oplusImpl, types_seven_dof_expmap.h:60-69"""
    u = np.array(u, dtype=np.float64)
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u), S)


def errors(S, pr):
    """both computeError() (types_seven_dof_expmap.h:138-167) for every pair: e12 [n,2], e21 [n,2], y, z"""
    q, t, s = S
    R = q2R(q)
    y = s * (pr.p2c @ R.T) + t
    e12 = pr.uv1 - (y[:, :2] / y[:, 2:3] * pr.K1[:2] + pr.K1[2:])
    ti = R.T @ ((-1.0 / s) * t)                      # Sim3::inverse, sim3.h:233-236
    z = (1.0 / s) * (pr.p1c @ R) + ti
    e21 = pr.uv2 - (z[:, :2] / z[:, 2:3] * pr.K2[:2] + pr.K2[2:])
    return e12, e21, y, z


def _dproj(P, K):
    """d(K pi(P))/dP, [n,2,3]"""
    n = len(P)
    d = np.zeros((n, 2, 3))
    iz = 1.0 / P[:, 2]
    d[:, 0, 0] = K[0] * iz
    d[:, 0, 2] = -K[0] * P[:, 0] * iz * iz
    d[:, 1, 1] = K[1] * iz
    d[:, 1, 2] = -K[1] * P[:, 1] * iz * iz
    return d


def _gen(P):
    """[ -[P]x | I | P ]  ([n,3,7]): derivative of exp(d) P at d = 0"""
    n = len(P)
    D = np.zeros((n, 3, 7))
    D[:, 0, 1], D[:, 0, 2] = P[:, 2], -P[:, 1]
    D[:, 1, 0], D[:, 1, 2] = -P[:, 2], P[:, 0]
    D[:, 2, 0], D[:, 2, 1] = P[:, 1], -P[:, 0]
    D[:, 0, 3] = D[:, 1, 4] = D[:, 2, 5] = 1.0
    D[:, :, 6] = P
    return D


def jac_analytic(S, pr, y, z, fix_scale):
    """J12 = -dpi(y) [ -[y]x | I | y ],  J21 = +dpi(z) (R^T / s) [ -[P1c]x | I | P1c ]   ([n,2,7] each)"""
    q, _, s = S
    R = q2R(q)
    J12 = -np.einsum("nij,njk->nik", _dproj(y, pr.K1), _gen(y))
    M = np.einsum("nij,jk->nik", _dproj(z, pr.K2), R.T / s)
    J21 = np.einsum("nij,njk->nik", M, _gen(pr.p1c))
    if fix_scale:
        J12[:, :, 6] = 0.0
        J21[:, :, 6] = 0.0
    return J12, J21


def jac_numeric(S, pr, fix_scale, step=1e-9):
    """central differences through oplus, as BaseBinaryEdge::linearizeOplus does for both edges (base_binary_edge.hpp:147-148)"""
    n = len(pr.p1c)
    J12 = np.zeros((n, 2, 7))
    J21 = np.zeros((n, 2, 7))
    for k in range(7):
        u = np.zeros(7)
        u[k] = step
        a = errors(oplus(S, u, fix_scale), pr)
        b = errors(oplus(S, -u, fix_scale), pr)
        J12[:, :, k] = (a[0] - b[0]) / (2 * step)
        J21[:, :, k] = (a[1] - b[1]) / (2 * step)
    return J12, J21


def huber(e2, delta):
    """RobustKernelHuber::robustify: rho(e2) and rho'(e2)"""
    d2 = delta * delta
    sq = np.sqrt(np.where(e2 <= d2, 1.0, e2))
    return np.where(e2 <= d2, e2, 2 * sq * delta - d2), np.where(e2 <= d2, 1.0, delta / sq)


class _Graph:
    """the optimizer's state: estimate, active pairs, and the chi2 g2o stored at the last computeActiveErrors"""

    def __init__(self, pr, S):
        self.pr, self.S = pr, S
        n = len(pr.p1c)
        self.act = np.ones(n, dtype=bool)
        self.c12 = np.zeros(n)
        self.c21 = np.zeros(n)

    def compute_errors(self):
        """computeActiveErrors + activeRobustChi2"""
        pr, a = self.pr, self.act
        e12, e21, y, z = errors(self.S, pr)
        c12 = pr.w1 * (e12[:, 0] * e12[:, 0] + e12[:, 1] * e12[:, 1])
        c21 = pr.w2 * (e21[:, 0] * e21[:, 0] + e21[:, 1] * e21[:, 1])
        self.c12[a], self.c21[a] = c12[a], c21[a]
        self.last = (e12, e21, y, z)
        return float(np.sum(huber(c12[a], pr.huber)[0] + huber(c21[a], pr.huber)[0]))


def _lm(g, its, fix_scale, jac, tr):
    """OptimizationAlgorithmLevenberg::solve called `its` times by SparseOptimizer::optimize (levenberg.cpp:61-164)"""
    pr, a = g.pr, g.act
    lam, ni, nb, cj, cur = 0.0, 2.0, 0, 0, 0.0
    for it in range(its):
        cur = g.compute_errors()
        ini = cur
        e12, e21, y, z = g.last
        J12, J21 = jac_numeric(g.S, pr, fix_scale) if jac == "numeric" else jac_analytic(g.S, pr, y, z, fix_scale)
        H = np.zeros((7, 7))
        b = np.zeros(7)
        for e, J, c, w in ((e12, J12, g.c12, pr.w1), (e21, J21, g.c21, pr.w2)):
            rw = (huber(c[a], pr.huber)[1] * w[a])
            H += np.einsum("n,nij,nik->jk", rw, J[a], J[a])
            b -= np.einsum("n,nij,ni->j", rw, J[a], e[a])
        if it == 0:
            lam = 1e-5 * float(np.abs(np.diag(H)).max())
            ni, nb = 2.0, 0
        q = 0
        while True:
            Sbk = g.S
            A = H + lam * np.eye(7)
            ok = True
            try:
                L = np.linalg.cholesky(A)               # fails on a non-positive pivot, as the dense LDL^T check does
                x = np.linalg.solve(L.T, np.linalg.solve(L, b))
            except np.linalg.LinAlgError:
                ok, x = False, np.zeros(7)
            if not np.all(np.isfinite(x)):
                ok, x = False, np.zeros(7)
            g.S = oplus(g.S, x, fix_scale)
            tmp = g.compute_errors()
            if not ok:
                tmp = DBL_MAX
            rho = cur - tmp
            rho /= float(x @ (lam * x + b)) + 1e-3
            good = rho > 0 and np.isfinite(tmp)
            if tr is not None:
                tr.append((cur, tmp, bool(good)))
            if good:
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = tmp
            else:
                lam *= ni
                ni *= 2
                g.S = Sbk                                # pop(): the estimate, not the stored errors
            q += 1
            if not (rho < 0 and q < 10):
                break
        cj += 1
        if q == 10 or rho == 0:
            break
        nb = nb + 1 if (ini - cur) * 1e3 < ini else 0
        if nb >= 3:
            break
    return cj, cur


def check_problem(pr):
    n = len(pr.p1c)
    for name, shape in (("p1c", (n, 3)), ("p2c", (n, 3)), ("uv1", (n, 2)), ("uv2", (n, 2)), ("w1", (n,)), ("w2", (n,))):
        if np.asarray(getattr(pr, name)).shape != shape:
            raise ValueError("sim3_ref: %s has shape %s, expected %s" % (name, np.asarray(getattr(pr, name)).shape, shape))
    S = np.asarray(pr.S12, dtype=np.float64)
    if S.shape != (8,) or not np.all(np.isfinite(S)):
        raise ValueError("sim3_ref: S12 must be 8 finite numbers (t, q xyzw, s)")
    if not S[7] > 0:
        raise ValueError("sim3_ref: scale must be positive")
    if not (S[3:7] @ S[3:7]) > 0:
        raise ValueError("sim3_ref: zero quaternion")
    if min(pr.its_stage1, pr.its_stage2_bad, pr.its_stage2_clean) < 1:
        raise ValueError("sim3_ref: iteration budgets must be at least 1")


def optimize(pr, jac="analytic", trace=False):
    """The protocol of Optimizer::OptimizeSim3 (src/Optimizer.cpp:4722-4784) on one candidate."""
    if jac not in ("analytic", "numeric"):
        raise ValueError("sim3_ref: jac must be 'analytic' or 'numeric'")
    check_problem(pr)
    n = len(pr.p1c)
    fix = bool(pr.fix_scale)
    S_in = np.array(pr.S12, dtype=np.float64)
    res = SimpleNamespace(n_inliers=0, status=0, n_bad_stage1=0, its_done=(0, 0), chi2_stage=np.zeros(2),
                          outlier=np.zeros(n, dtype=np.uint8), chi2_12=np.zeros(n), chi2_21=np.zeros(n), S12=S_in.copy(),
                          chi2_first=(np.zeros(n), np.zeros(n)), stage2_budget=0, trace=([], []) if trace else None)
    if n == 0:
        return res
    g = _Graph(pr, (S_in[3:7].copy(), S_in[:3].copy(), float(S_in[7])))
    it1, chi1 = _lm(g, pr.its_stage1, fix, jac, res.trace[0] if trace else None)
    bad = (g.c12 > pr.th2) | (g.c21 > pr.th2)               # :4736
    nbad = int(bad.sum())
    g.act = ~bad
    res.n_bad_stage1 = nbad
    res.its_done = (it1, 0)
    res.chi2_stage[0] = chi1
    res.outlier[:] = bad
    res.chi2_12[:], res.chi2_21[:] = g.c12, g.c21
    res.chi2_first = (g.c12.copy(), g.c21.copy())            # what the first test read, for every pair
    if n - nbad < pr.min_inliers:                            # :4755: S12 is not written back
        return res
    res.stage2_budget = pr.its_stage2_bad if nbad > 0 else pr.its_stage2_clean            # nMoreIterations, :4748-4752
    it2, chi2 = _lm(g, res.stage2_budget, fix, jac, res.trace[1] if trace else None)
    out = bad | (g.act & ((g.c12 > pr.th2) | (g.c21 > pr.th2)))   # :4771
    res.its_done = (it1, it2)
    res.chi2_stage[1] = chi2
    res.outlier[:] = out
    res.chi2_12[:], res.chi2_21[:] = g.c12, g.c21
    res.n_inliers = int((~out).sum())
    q, t, s = g.S
    res.S12 = np.concatenate([t, q, [s]])
    return res


def decidable(tr, rel=1e-10):
    """True when every LM trial of the list changed the cost by more than `rel` relative: none was decided by rounding"""
    return all(abs(c0 - c1) > rel * abs(c0) for c0, c1, _ in tr)


def gate_margin(res, th2):
    """smallest relative distance from the gate of any chi2 that either outlier test read"""
    c = np.concatenate([res.chi2_12, res.chi2_21, res.chi2_first[0], res.chi2_first[1]])
    return float(np.min(np.abs(c / th2 - 1.0))) if len(c) else np.inf
