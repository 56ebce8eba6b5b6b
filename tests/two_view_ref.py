"""NumPy restatement of Initializer::Initialize (src/Initializer.cpp:36-130) behind the drawing of the 8-sets: the yardstick of
vba_two_view_init (test infrastructure, like triangulate_ref.py).

Everything runs in the dtype asked for (np.float32: what the reference's CV_32F does, np.float64: what the library does,
np.longdouble: the yardstick's own error bar).  The SVDs are one-sided (Hestenes) Jacobi iterations over the columns of A written
out here so that they run in all three: nine columns in the round-robin order of the kernel (in round r column c meets column
(r - c) mod 9), three and four columns cyclically; all hypotheses of a pair are computed side by side (arrays over the hypothesis
index), all matches of an (R, t) likewise.  Where the reference compares a float with a double literal (0.40, 0.99998, 1.00001,
0.7 * maxGood, 0.75 * bestGood, 0.9 * N) the comparison is made in at least float64, as C++ promotes it; `th` and `thScore` are
the reference's float variables.  In float32 the scores are summed match by match as the reference does; the library sums them
in another (fixed) order, which is part of the float64 rounding the tolerances cover.

Sign convention of the 3x3 SVDs (svd3): singular values descending (the first among equals first), (u_i, v_i) flipped together so
that the largest-magnitude component of u_i (the first among equals) is positive; `complete` (DecomposeE, where sigma_3 = 0):
u_3 = u_1 x u_2, v_3 = v_1 x v_2.  flip=True is the opposite convention everywhere an SVD is free to choose (every u_i's largest
component negative, u_3 = -(u_1 x u_2) with v_3 unchanged, the 9-vectors negated): ok, reason, R21, t21, the points and the
sorted rt_good must not change (tests/test_two_view_ref.py).

The yardstick also records the margin of every comparison it evaluates (`margins`: name -> the smallest |value - threshold|,
relative where the threshold is not zero) and the relative gap between the two smallest singular values of every 9-column A.
"""
import numpy as np

SWEEPS9 = {np.float32: 10, np.float64: 10, np.longdouble: 14}
SWEEPS34 = {np.float32: 8, np.float64: 8, np.longdouble: 12}
PAIRS9 = [(c, (r - c) % 9) for r in range(9) for c in range(9) if c < (r - c) % 9]
PAIRS4 = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
PAIRS3 = ((0, 1), (0, 2), (1, 2))
assert len(PAIRS9) == 36 and len(set(PAIRS9)) == 36


def _wide(dtype):
    return np.promote_types(dtype, np.float64).type


def _coldot(U, p, q):
    """sum over the rows of U[:, :, p] * U[:, :, q], row after row"""
    s = U[:, 0, p] * U[:, 0, q]
    for r in range(1, U.shape[1]):
        s = s + U[:, r, p] * U[:, r, q]
    return s


def hestenes(A, pairs, sweeps, dtype):
    """one-sided Jacobi on A [n, rows, cols]: (A V [n, rows, cols], V [n, cols, cols]); fixed sweeps, no pivoting"""
    U = np.array(A, dtype=dtype)
    n, _, nc = U.shape
    V = np.zeros((n, nc, nc), dtype=dtype)
    for i in range(nc):
        V[:, i, i] = 1
    one, two = dtype(1), dtype(2)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in pairs:
                alpha, beta, gamma = _coldot(U, p, p), _coldot(U, q, q), _coldot(U, p, q)
                zeta = (beta - alpha) / (two * gamma)
                t = np.copysign(one, zeta) / (np.abs(zeta) + np.sqrt(zeta * zeta + one))
                t = np.where(gamma == 0, dtype(0), t).astype(dtype)
                c = one / np.sqrt(t * t + one)
                s = t * c
                for M in (U, V):
                    mp, mq = M[:, :, p].copy(), M[:, :, q].copy()
                    M[:, :, p] = c[:, None] * mp - s[:, None] * mq
                    M[:, :, q] = s[:, None] * mp + c[:, None] * mq
    return U, V


def null9(A, dtype, flip=False):
    """the right singular vector of the smallest singular value of A [n, rows, 9] (the first among equals), and the relative gap
    (s_b - s_a) / s_b between the two smallest singular values"""
    U, V = hestenes(A, PAIRS9, SWEEPS9[dtype], dtype)
    n2 = np.stack([_coldot(U, k, k) for k in range(9)], axis=1)
    k = np.argmin(n2, axis=1)
    v = V[np.arange(len(V)), :, k]
    s = np.sqrt(np.sort(n2.astype(np.float64), axis=1))
    with np.errstate(all="ignore"):
        gap = (s[:, 1] - s[:, 0]) / s[:, 1]
    return (-v if flip else v), gap


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def svd3(A, dtype, complete=False, flip=False):
    """SVD of A [n,3,3] under the convention of the module docstring: U [n,3,3] (columns u_i), w [n,3] descending, V [n,3,3]"""
    B, V = hestenes(A, PAIRS3, SWEEPS34[dtype], dtype)
    n2 = np.stack([_coldot(B, k, k) for k in range(3)], axis=1)
    order = np.argsort(-n2, axis=1, kind="stable")
    ar = np.arange(len(B))
    w = np.sqrt(np.take_along_axis(n2, order, axis=1))
    Uo, Vo = np.zeros_like(B), np.zeros_like(V)
    with np.errstate(all="ignore"):
        for i in range(3):
            u = B[ar, :, order[:, i]] / w[:, i:i + 1]
            v = V[ar, :, order[:, i]]
            big = u[ar, np.argmax(np.abs(u), axis=1)]
            sg = np.where(big < 0, dtype(-1), dtype(1)).astype(dtype)
            if flip:
                sg = -sg
            Uo[:, :, i] = sg[:, None] * u
            Vo[:, :, i] = sg[:, None] * v
    if complete:
        Uo[:, :, 2] = _cross(Uo[:, :, 0], Uo[:, :, 1]) * (dtype(-1) if flip else dtype(1))
        Vo[:, :, 2] = _cross(Vo[:, :, 0], Vo[:, :, 1])
    return Uo, w, Vo


def _mm(A, B):
    """A B for stacks of 3x3 (or one 3x3 broadcast), every entry summed k = 0, 1, 2 as cv::Mat's product does"""
    A, B = np.asarray(A), np.asarray(B)
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + A[..., :, 2, None] * B[..., None, 2, :]


def _det3(m):
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1]) - m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0])) \
        + m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0])


def _inv3(m, dtype):
    """inverse by cofactors (a singular matrix gives non-finite entries)"""
    with np.errstate(all="ignore"):
        idet = dtype(1) / _det3(m)
    o = np.empty_like(m)
    o[..., 0, 0] = m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1]
    o[..., 0, 1] = m[..., 0, 2] * m[..., 2, 1] - m[..., 0, 1] * m[..., 2, 2]
    o[..., 0, 2] = m[..., 0, 1] * m[..., 1, 2] - m[..., 0, 2] * m[..., 1, 1]
    o[..., 1, 0] = m[..., 1, 2] * m[..., 2, 0] - m[..., 1, 0] * m[..., 2, 2]
    o[..., 1, 1] = m[..., 0, 0] * m[..., 2, 2] - m[..., 0, 2] * m[..., 2, 0]
    o[..., 1, 2] = m[..., 0, 2] * m[..., 1, 0] - m[..., 0, 0] * m[..., 1, 2]
    o[..., 2, 0] = m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]
    o[..., 2, 1] = m[..., 0, 1] * m[..., 2, 0] - m[..., 0, 0] * m[..., 2, 1]
    o[..., 2, 2] = m[..., 0, 0] * m[..., 1, 1] - m[..., 0, 1] * m[..., 1, 0]
    with np.errstate(all="ignore"):
        return (o * idet[..., None, None]).astype(dtype)


def _seqsum(x):
    """sum along the last axis, element after element"""
    if x.shape[-1] == 0:
        return np.zeros(x.shape[:-1], dtype=x.dtype)
    return np.add.accumulate(x, axis=-1)[..., -1]


class Margins(dict):
    """name -> the smallest distance of a compared value from its threshold"""

    def note(self, name, value):
        v = np.abs(np.asarray(value, dtype=np.float64)).ravel()
        v = v[~np.isnan(v)]
        if v.size:
            self[name] = min(self.get(name, np.inf), float(v.min()))


def normalize(uv, dtype):
    """Normalize (:893-946): (vNormalizedPoints, T, Tinv); Tinv is the analytic inverse of the triangular T"""
    wd = _wide(dtype)
    n = uv.shape[0]
    uv = np.asarray(uv, dtype=dtype)
    with np.errstate(all="ignore"):
        mean = (_seqsum(uv.T) / dtype(n)).astype(dtype)
        c = uv - mean
        dev = (_seqsum(np.abs(c).T) / dtype(n)).astype(dtype)
        s = (wd(1) / dev.astype(wd)).astype(dtype)                      # float sX = 1.0 / meanDevX
        pn = c * s
        T = np.array([[s[0], 0, -mean[0] * s[0]], [0, s[1], -mean[1] * s[1]], [0, 0, 1]], dtype=dtype)
        Tinv = np.array([[(wd(1) / wd(s[0])), 0, mean[0]], [0, (wd(1) / wd(s[1])), mean[1]], [0, 0, 1]], dtype=dtype)
    return pn, T, Tinv


def build_A(p, pn1, pn2, dtype):
    """A of ComputeH21 [nh,16,9] (:267-297) and of ComputeF21 [nh,8,9] (:323-342) for every set"""
    m = p.match[p.sets]                                                 # [nh,8,2]
    a, b = pn1[m[..., 0]], pn2[m[..., 1]]
    u1, v1, u2, v2 = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
    nh = p.n_hyp
    one, zero = np.ones_like(u1), np.zeros_like(u1)
    AH = np.zeros((nh, 16, 9), dtype=dtype)
    AH[:, 0::2] = np.stack([zero, zero, zero, -u1, -v1, -one, v2 * u1, v2 * v1, v2], axis=-1)
    AH[:, 1::2] = np.stack([u1, v1, one, zero, zero, zero, -u2 * u1, -u2 * v1, -u2], axis=-1)
    AF = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, one], axis=-1).astype(dtype)
    return AH, AF


def check_h(H21, H12, P, sigma, dtype, M=None):
    """CheckHomography (:362-461) of hypotheses H21 / H12 [nh,3,3] over the matches P = (u1, v1, u2, v2): (score [nh], flags [nh,N])"""
    wd = _wide(dtype)
    u1, v1, u2, v2 = (x[None, :] for x in P)
    th = dtype(np.float32(5.991))
    g = lambda Hm, i, j: Hm[:, i, j, None]
    with np.errstate(all="ignore"):
        inv_s2 = dtype(wd(1) / wd(dtype(sigma) * dtype(sigma)))
        w = (wd(1) / ((g(H12, 2, 0) * u2 + g(H12, 2, 1) * v2) + g(H12, 2, 2)).astype(wd)).astype(dtype)
        x = ((g(H12, 0, 0) * u2 + g(H12, 0, 1) * v2) + g(H12, 0, 2)) * w
        y = ((g(H12, 1, 0) * u2 + g(H12, 1, 1) * v2) + g(H12, 1, 2)) * w
        chi1 = ((u1 - x) * (u1 - x) + (v1 - y) * (v1 - y)) * inv_s2
        w = (wd(1) / ((g(H21, 2, 0) * u1 + g(H21, 2, 1) * v1) + g(H21, 2, 2)).astype(wd)).astype(dtype)
        x = ((g(H21, 0, 0) * u1 + g(H21, 0, 1) * v1) + g(H21, 0, 2)) * w
        y = ((g(H21, 1, 0) * u1 + g(H21, 1, 1) * v1) + g(H21, 1, 2)) * w
        chi2 = ((u2 - x) * (u2 - x) + (v2 - y) * (v2 - y)) * inv_s2
        bad1, bad2 = chi1 > th, chi2 > th
    if M is not None:
        M.note("chi2_h", chi1 / th - 1); M.note("chi2_h", chi2 / th - 1)
    terms = np.stack([np.where(bad1, dtype(0), th - chi1), np.where(bad2, dtype(0), th - chi2)], axis=-1).astype(dtype)
    return _seqsum(terms.reshape(terms.shape[0], -1)), ~(bad1 | bad2)


def check_f(F, P, sigma, dtype, M=None):
    """CheckFundamental (:465-545)"""
    wd = _wide(dtype)
    u1, v1, u2, v2 = (x[None, :] for x in P)
    th, th_score = dtype(np.float32(3.841)), dtype(np.float32(5.991))
    g = lambda i, j: F[:, i, j, None]
    with np.errstate(all="ignore"):
        inv_s2 = dtype(wd(1) / wd(dtype(sigma) * dtype(sigma)))
        a2, b2, c2 = (g(0, 0) * u1 + g(0, 1) * v1) + g(0, 2), (g(1, 0) * u1 + g(1, 1) * v1) + g(1, 2), (g(2, 0) * u1 + g(2, 1) * v1) + g(2, 2)
        num2 = (a2 * u2 + b2 * v2) + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2
        a1, b1, c1 = (g(0, 0) * u2 + g(1, 0) * v2) + g(2, 0), (g(0, 1) * u2 + g(1, 1) * v2) + g(2, 1), (g(0, 2) * u2 + g(1, 2) * v2) + g(2, 2)
        num1 = (a1 * u1 + b1 * v1) + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2
        bad1, bad2 = chi1 > th, chi2 > th
    if M is not None:
        M.note("chi2_f", chi1 / th - 1); M.note("chi2_f", chi2 / th - 1)
    terms = np.stack([np.where(bad1, dtype(0), th_score - chi1), np.where(bad2, dtype(0), th_score - chi2)], axis=-1).astype(dtype)
    return _seqsum(terms.reshape(terms.shape[0], -1)), ~(bad1 | bad2)


def scan(score, M=None, name=""):
    """:179 / :233: strict > against 0.0 in hypothesis order: (best index or -1, its score).  Margin: how far the best score is
    above every other one, relative to it (an exact tie counts as 0)"""
    best, bi = score.dtype.type(0), -1
    for h, s in enumerate(score):
        if s > best:
            best, bi = s, h
    if M is not None and bi >= 0:
        others = np.delete(np.asarray(score, dtype=np.float64), bi)
        others = others[~np.isnan(others)]
        if others.size:
            M.note("scan_" + name, (float(best) - others.max()) / float(best))
    return bi, best


def check_rt(R, t, K, P, flags, th2, dtype, M=None):
    """CheckRT (:950-1082) of one (R, t): dict(state [N] 0 rejected / 1 counted / 2 counted and flagged, x [N,3], cos [N], n_good,
    parallax)"""
    from triangulate_ref import hestenes4, smallest
    wd = _wide(dtype)
    u1, v1, u2, v2 = P
    N = u1.shape[0]
    fx, fy, cx, cy = (dtype(k) for k in K)
    idx = np.nonzero(flags)[0]
    state, X, C = np.zeros(N, dtype=np.uint8), np.zeros((N, 3), dtype=dtype), np.zeros(N, dtype=dtype)
    out = dict(state=state, x=X, cos=C, n_good=0, parallax=dtype(0))
    if idx.size == 0:
        return out
    u1, v1, u2, v2 = u1[idx], v1[idx], u2[idx], v2[idx]
    n = idx.size
    Rt = np.hstack([R, t[:, None]]).astype(dtype)
    with np.errstate(all="ignore"):
        P2 = np.stack([fx * Rt[0] + cx * Rt[2], fy * Rt[1] + cy * Rt[2], Rt[2]])          # K [R | t] (:982-985)
        O2 = -((R[0] * t[0] + R[1] * t[1]) + R[2] * t[2])                                   # -R^T t (:987)
        A = np.zeros((n, 4, 4), dtype=dtype)
        A[:, 0, 0] = -fx; A[:, 0, 2] = u1 - cx
        A[:, 1, 1] = -fy; A[:, 1, 2] = v1 - cy
        A[:, 2] = u2[:, None] * P2[2] - P2[0]
        A[:, 3] = v2[:, None] * P2[2] - P2[1]
        sig2, V = hestenes4(A, dtype)
        v = smallest(sig2, V)
        x = v[:, :3] / v[:, 3:4]
        live = np.isfinite(x).all(axis=1)                                                   # :1014
        n2 = x - O2
        d1 = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        d2 = np.sqrt((n2[:, 0] * n2[:, 0] + n2[:, 1] * n2[:, 1]) + n2[:, 2] * n2[:, 2])
        cos = ((x[:, 0] * n2[:, 0] + x[:, 1] * n2[:, 1]) + x[:, 2] * n2[:, 2]) / (d1 * d2)
        par = cos.astype(wd) < wd(0.99998)

        def note(name, val, where):
            if M is not None:
                M.note(name, np.asarray(val, dtype=np.float64)[where])

        note("rt_cos", cos.astype(wd) - wd(0.99998), live)
        note("rt_z1", x[:, 2], live)
        live &= ~((x[:, 2] <= 0) & par)                                                     # :1031
        y = np.stack([(R[k, 0] * x[:, 0] + R[k, 1] * x[:, 1]) + R[k, 2] * x[:, 2] for k in range(3)], axis=1) + t
        note("rt_z2", y[:, 2], live)
        live &= ~((y[:, 2] <= 0) & par)                                                     # :1038
        iz = (wd(1) / x[:, 2].astype(wd)).astype(dtype)
        ex, ey = (fx * x[:, 0] * iz + cx) - u1, (fy * x[:, 1] * iz + cy) - v1
        e1 = ex * ex + ey * ey
        note("rt_err1", e1 / dtype(th2) - 1, live)
        live &= ~(e1 > dtype(th2))                                                          # :1049
        iz = (wd(1) / y[:, 2].astype(wd)).astype(dtype)
        ex, ey = (fx * y[:, 0] * iz + cx) - u2, (fy * y[:, 1] * iz + cy) - v2
        e2 = ex * ex + ey * ey
        note("rt_err2", e2 / dtype(th2) - 1, live)
        live &= ~(e2 > dtype(th2))                                                          # :1060
    state[idx] = np.where(live, np.where(par, 2, 1), 0)
    X[idx] = np.where(live[:, None], x, dtype(0))
    C[idx] = cos
    ng = int(live.sum())
    out["n_good"] = ng
    if ng > 0:
        cs = np.sort(cos[live], kind="stable")
        k = min(50, ng - 1)
        with np.errstate(all="ignore"):
            out["parallax"] = dtype((np.arccos(cs[k]) * dtype(180)).astype(wd) / wd(np.pi))   # :1074
    return out


def decompose_e(F21, K, dtype, flip=False):
    """E = K^T F K (:569), DecomposeE (:1095-1117): [(R1,t), (R2,t), (R1,-t), (R2,-t)]"""
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], dtype=dtype)
    E = _mm(_mm(Km.T, F21), Km)
    U, w, V = svd3(E[None], dtype, complete=True, flip=flip)
    U, V = U[0], V[0]
    t = U[:, 2]
    t = t / np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=dtype)
    R1, R2 = _mm(_mm(U, W), V.T), _mm(_mm(U, W.T), V.T)
    R1 = -R1 if _det3(R1) < 0 else R1
    R2 = -R2 if _det3(R2) < 0 else R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def decompose_h(H21, K, dtype, M=None, flip=False):
    """ReconstructH (:687-790): the eight Faugeras hypotheses, or None where :699 returns false"""
    wd = _wide(dtype)
    one = dtype(1)
    with np.errstate(all="ignore"):
        Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], dtype=dtype)
        Ki = np.array([[one / K[0], 0, -K[2] / K[0]], [0, one / K[1], -K[3] / K[1]], [0, 0, 1]], dtype=dtype)
        A = _mm(_mm(Ki, H21), Km)
        U, w, V = svd3(A[None], dtype, complete=False, flip=flip)
        U, w, V = U[0], w[0], V[0]
        Vt = V.T
        s = _det3(U) * _det3(Vt)
        d1, d2, d3 = w
        if M is not None:
            M.note("h_ratio", [wd(d1 / d2) - wd(1.00001), wd(d2 / d3) - wd(1.00001)])
        if wd(d1 / d2) < wd(1.00001) or wd(d2 / d3) < wd(1.00001):                          # :699
            return None
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        st = [aux_st, -aux_st, -aux_st, aux_st]
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        out = []
        for h in range(8):
            i = h & 3
            if h < 4:
                Rp = np.array([[ct, 0, -st[i]], [0, 1, 0], [st[i], 0, ct]], dtype=dtype)
                tp = np.array([x1[i], 0, -x3[i]], dtype=dtype) * (d1 - d3)
            else:
                Rp = np.array([[cp, 0, sp[i]], [0, -1, 0], [sp[i], 0, -cp]], dtype=dtype)
                tp = np.array([x1[i], 0, x3[i]], dtype=dtype) * (d1 + d3)
            R = _mm(_mm(s * U, Rp), Vt)
            t = (U[:, 0] * tp[0] + U[:, 1] * tp[1]) + U[:, 2] * tp[2]
            out.append((R.astype(dtype), (t / np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])).astype(dtype)))
    return out


def two_view(p, dtype=np.float64, flip=False):
    """the fields of vba_two_view_result for the abi.TwoViewProblem p, computed in dtype, plus `margins`, `gap_h`, `gap_f` (the
    relative gap of the two smallest singular values of every A) and `rt` (what check_rt returned for every (R, t))"""
    wd = _wide(dtype)
    M = Margins()
    nh, N, nk1 = p.n_hyp, p.n_matches, p.n_keys1
    K = np.asarray(p.K, dtype=dtype)
    r = dict(status=0, ok=0, model=0, reason=0, best_hyp_h=-1, best_hyp_f=-1, n_inliers_h=0, n_inliers_f=0, n_rt=0, best_rt=-1,
             rt_good=np.zeros(8, dtype=np.int32), score_h=dtype(0), score_f=dtype(0), rh=dtype(0), H21=np.zeros((3, 3), dtype=dtype),
             F21=np.zeros((3, 3), dtype=dtype), rt_parallax=np.zeros(8, dtype=dtype), R21=None, t21=None,
             inlier_h=np.zeros(N, dtype=np.uint8), inlier_f=np.zeros(N, dtype=np.uint8), x3d=None, triangulated=None,
             hyp_score_h=np.zeros(nh, dtype=dtype), hyp_score_f=np.zeros(nh, dtype=dtype), margins=M, gap_h=np.zeros(0), gap_f=np.zeros(0), rt=[])
    uv1, uv2 = np.asarray(p.uv1, dtype=dtype), np.asarray(p.uv2, dtype=dtype)
    P = (uv1[p.match[:, 0], 0], uv1[p.match[:, 0], 1], uv2[p.match[:, 1], 0], uv2[p.match[:, 1], 1])
    if nh > 0:
        pn1, T1, _ = normalize(uv1, dtype)
        pn2, T2, T2inv = normalize(uv2, dtype)
        AH, AF = build_A(p, pn1, pn2, dtype)
        vH, r["gap_h"] = null9(AH, dtype, flip)
        vF, r["gap_f"] = null9(AF, dtype, flip)
        H21 = _mm(_mm(T2inv, vH.reshape(nh, 3, 3)), T1).astype(dtype)                       # :172
        H12 = _inv3(H21, dtype)                                                             # :173
        U, w, V = svd3(vF.reshape(nh, 3, 3), dtype, flip=flip)                              # :350-354
        Fn = U[:, :, 0, None] * w[:, 0, None, None] * V[:, None, :, 0] + U[:, :, 1, None] * w[:, 1, None, None] * V[:, None, :, 1]
        F21 = _mm(_mm(T2.T, Fn.astype(dtype)), T1).astype(dtype)                            # :228
        sh, fh = check_h(H21, H12, P, p.sigma, dtype, M)
        sf, ff = check_f(F21, P, p.sigma, dtype, M)
        r["hyp_score_h"], r["hyp_score_f"] = sh, sf
        bh, SH = scan(sh, M, "h")
        bf, SF = scan(sf, M, "f")
        r["best_hyp_h"], r["best_hyp_f"], r["score_h"], r["score_f"] = bh, bf, SH, SF
        if bh >= 0:
            r["H21"], r["inlier_h"] = H21[bh], fh[bh].astype(np.uint8)
        if bf >= 0:
            r["F21"], r["inlier_f"] = F21[bf], ff[bf].astype(np.uint8)
        r["n_inliers_h"], r["n_inliers_f"] = int(r["inlier_h"].sum()), int(r["inlier_f"].sum())
    SH, SF = dtype(r["score_h"]), dtype(r["score_f"])
    with np.errstate(all="ignore"):
        RH = SH / (SH + SF)                                                                 # :120
    r["rh"] = RH
    is_h = bool(wd(RH) > wd(0.40))                                                          # :123
    if not np.isnan(RH):
        M.note("rh", wd(RH) - wd(0.40))
    r["model"] = 1 if is_h else 2
    if (r["best_hyp_h"] if is_h else r["best_hyp_f"]) < 0:
        r["reason"] = 1
        return r
    flags = (r["inlier_h"] if is_h else r["inlier_f"]).astype(bool)
    Nin = int(flags.sum())
    hyps = decompose_h(r["H21"], K, dtype, M, flip) if is_h else decompose_e(r["F21"], K, dtype, flip)
    if hyps is None:
        r["reason"] = 2
        return r
    th2 = wd(4.0) * wd(dtype(p.sigma) * dtype(p.sigma))                                     # 4.0 * mSigma2
    rt = [check_rt(R, t, K, P, flags, th2, dtype, M) for R, t in hyps]
    r["rt"], r["n_rt"] = rt, len(rt)
    good = [c["n_good"] for c in rt]
    r["rt_good"][:len(rt)] = good
    r["rt_parallax"][:len(rt)] = [c["parallax"] for c in rt]
    win = -1
    if not is_h:                                                                            # ReconstructF (:590-667)
        max_good = max(good)
        n_min_good = max(int(0.9 * Nin), p.min_triangulated)
        nsimilar = sum(1 for g in good if g > 0.7 * max_good)
        M.note("f_min_good", max_good - n_min_good + 0.5)
        M.note("f_similar", [g - 0.7 * max_good for g in good])
        if max_good < n_min_good or nsimilar > 1:
            r["reason"] = 4
            return r
        k = good.index(max_good)
        M.note("f_parallax", float(rt[k]["parallax"]) - float(dtype(p.min_parallax)))
        if rt[k]["parallax"] > dtype(p.min_parallax):
            win = k
        else:
            r["reason"] = 5
            return r
    else:                                                                                   # ReconstructH (:793-835)
        best, second, bi, bpar = 0, 0, -1, dtype(-1)
        for k, g in enumerate(good):
            if g > best:
                second, best, bi, bpar = best, g, k, rt[k]["parallax"]
            elif g > second:
                second = g
        M.note("h_second", second - 0.75 * best)
        M.note("h_parallax", float(bpar) - float(dtype(p.min_parallax)))
        M.note("h_min_tri", best - p.min_triangulated - 0.5)
        M.note("h_n90", best - 0.9 * Nin)
        if second < 0.75 * best and bpar >= dtype(p.min_parallax) and best > p.min_triangulated and best > 0.9 * Nin:
            win = bi
        else:
            r["reason"] = 3
            return r
    r["ok"], r["best_rt"] = 1, win
    r["R21"], r["t21"] = hyps[win]
    x3d, tri = np.zeros((nk1, 3), dtype=dtype), np.zeros(nk1, dtype=np.uint8)
    c = rt[win]
    g = c["state"] > 0
    x3d[p.match[g, 0]] = c["x"][g]
    tri[p.match[g, 0]] = c["state"][g] == 2
    r["x3d"], r["triangulated"] = x3d, tri
    return r
