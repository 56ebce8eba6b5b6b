"""NumPy restatement of the geometric part of LocalMapping::CreateNewMapPoints (src/LocalMapping.cpp:1358-1517, monocular): the
yardstick of vba_triangulate (test infrastructure, like sim3_ransac_ref.py).

Everything runs in the dtype asked for (np.float32: what the reference's CV_32F does, np.float64: what the library does,
np.longdouble: the yardstick's own error bar).  The SVD of the 4x4 A is a one-sided (Hestenes) Jacobi iteration over A's columns
written out here so that it runs in all three; all matches of a pair are computed side by side (arrays over the match index).
Where the reference compares a float with a double literal (0.9998 at :1389, 5.991 * sigma2 at :1450 / :1479) the comparison is
made in at least float64, as C++ promotes it.

Per match the yardstick returns the reason (the codes of include/vislam_ba.h), the point and the margin of every comparison it
evaluated (inf where the reference never reaches the comparison): absolute for the cosine, the homogeneous coordinate, the depths
and the distances, relative to the threshold for the chi-square and the ratio tests.
"""
import numpy as np

SWEEPS = {np.float32: 8, np.float64: 8, np.longdouble: 12}
_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
MARGINS = ("cos_pos", "cos_max", "w", "z1", "z2", "chi2_1", "chi2_2", "dist", "ratio_lo", "ratio_hi")


def _dot4(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + (a[:, 2] * b[:, 2] + a[:, 3] * b[:, 3])


def hestenes4(A, dtype=np.float64):
    """one-sided Jacobi on A [n,4,4]: (squared singular values [n,4], unsorted; right singular vectors [n,4,4] as columns).
    Rotations in the (p, q) planes of the columns make them mutually orthogonal; fixed sweeps, no pivoting"""
    U = np.array(A, dtype=dtype)
    n = U.shape[0]
    V = np.zeros((n, 4, 4), dtype=dtype)
    for i in range(4):
        V[:, i, i] = 1
    one, two = dtype(1), dtype(2)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS[dtype]):
            for p, q in _PAIRS:
                ap, aq = U[:, :, p].copy(), U[:, :, q].copy()
                alpha, beta, gamma = _dot4(ap, ap), _dot4(aq, aq), _dot4(ap, aq)
                zeta = (beta - alpha) / (two * gamma)
                t = np.copysign(one, zeta) / (np.abs(zeta) + np.sqrt(zeta * zeta + one))
                t = np.where(gamma == 0, dtype(0), t).astype(dtype)
                c = one / np.sqrt(t * t + one)
                s = t * c
                U[:, :, p] = c[:, None] * ap - s[:, None] * aq
                U[:, :, q] = s[:, None] * ap + c[:, None] * aq
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = c[:, None] * vp - s[:, None] * vq
                V[:, :, q] = s[:, None] * vp + c[:, None] * vq
    sig2 = np.stack([_dot4(U[:, :, k], U[:, :, k]) for k in range(4)], axis=1)
    return sig2, V


def smallest(sig2, V):
    """the column of V of the smallest singular value (the first one among equals)"""
    k = np.argmin(sig2, axis=1)
    return V[np.arange(len(V)), :, k]


def build_A(p, dtype):
    """xn1, xn2 (:1360-1361) and A (:1393-1397) of every match"""
    d = lambda a: np.asarray(a, dtype=dtype)
    one = dtype(1)
    K1, K2 = d(p.K1), d(p.K2)
    uv1, uv2 = d(p.uv1), d(p.uv2)
    n = uv1.shape[0]
    xn1 = np.stack([(uv1[:, 0] - K1[2]) * (one / K1[0]), (uv1[:, 1] - K1[3]) * (one / K1[1]), np.ones(n, dtype=dtype)], axis=1)
    xn2 = np.stack([(uv2[:, 0] - K2[2]) * (one / K2[0]), (uv2[:, 1] - K2[3]) * (one / K2[1]), np.ones(n, dtype=dtype)], axis=1)
    T1 = np.hstack([d(p.Rcw1), d(p.tcw1)[:, None]])
    T2 = np.hstack([d(p.Rcw2), d(p.tcw2)[:, None]])
    A = np.zeros((n, 4, 4), dtype=dtype)
    A[:, 0] = xn1[:, 0:1] * T1[2] - T1[0]
    A[:, 1] = xn1[:, 1:2] * T1[2] - T1[1]
    A[:, 2] = xn2[:, 0:1] * T2[2] - T2[0]
    A[:, 3] = xn2[:, 1:2] * T2[2] - T2[1]
    return xn1, xn2, A


def _dot3(r, x):
    """r [3] . x [n,3] in the order of cv::Mat::dot"""
    return (r[0] * x[:, 0] + r[1] * x[:, 1]) + r[2] * x[:, 2]


def _norm3(x):
    return np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])


def triangulate(p, dtype=np.float64):
    """dict(reason [n] uint8, x3d [n,3] (zeros for reasons 1 and 2), n_accepted, margins [n, len(MARGINS)], margin [n] (the
    smallest of a match), cos [n], v [n,4] the singular vector)"""
    d = lambda a: np.asarray(a, dtype=dtype)
    wide = np.promote_types(dtype, np.float64)
    w = lambda a: np.asarray(a, dtype=wide)
    one = dtype(1)
    n = p.n_matches
    reason = np.zeros(n, dtype=np.uint8)
    M = np.full((n, len(MARGINS)), np.inf)
    mi = {k: i for i, k in enumerate(MARGINS)}
    if n == 0:
        return dict(reason=reason, x3d=np.zeros((0, 3), dtype=dtype), n_accepted=0, margins=M, margin=np.zeros(0), cos=np.zeros(0, dtype=dtype),
                    v=np.zeros((0, 4), dtype=dtype))
    R1, t1, O1, K1 = d(p.Rcw1), d(p.tcw1), d(p.Ow1), d(p.K1)
    R2, t2, O2, K2 = d(p.Rcw2), d(p.tcw2), d(p.Ow2), d(p.K2)
    uv1, uv2 = d(p.uv1), d(p.uv2)
    with np.errstate(all="ignore"):
        xn1, xn2, A = build_A(p, dtype)
        ray1 = np.stack([_dot3(R1[:, k], xn1) for k in range(3)], axis=1)     # Rwc1 * xn1 = Rcw1^T xn1 (:1364)
        ray2 = np.stack([_dot3(R2[:, k], xn2) for k in range(3)], axis=1)
        cos = ((ray1[:, 0] * ray2[:, 0] + ray1[:, 1] * ray2[:, 1]) + ray1[:, 2] * ray2[:, 2]) / (_norm3(ray1) * _norm3(ray2))
        live = np.ones(n, dtype=bool)

        def drop(bad, code):
            nonlocal live
            reason[live & bad] = code
            live = live & ~bad

        def note(name, value):
            M[live, mi[name]] = np.abs(np.asarray(value, dtype=np.float64))[live]

        # :1389 cosParallaxRays > 0 && cosParallaxRays < 0.9998 (&& short-circuits), else :1423
        note("cos_pos", cos)
        pos = cos > 0
        M[live & pos, mi["cos_max"]] = np.abs(np.asarray(w(cos) - w(p.cos_max), dtype=np.float64))[live & pos]
        drop(~(pos & (w(cos) < w(p.cos_max))), 1)
        sig2, V = hestenes4(A, dtype)
        v = smallest(sig2, V)
        note("w", v[:, 3])
        drop(v[:, 3] == 0, 2)                                                  # :1404
        x = v[:, :3] / v[:, 3:4]                                               # :1408
        z1 = _dot3(R1[2], x) + t1[2]
        note("z1", z1)
        drop(z1 <= 0, 3)                                                       # :1429
        z2 = _dot3(R2[2], x) + t2[2]
        note("z2", z2)
        drop(z2 <= 0, 4)                                                       # :1433
        for side, (R, t, K, uv, z, oc, sg, code) in enumerate(((R1, t1, K1, uv1, z1, p.oct1, p.level_sigma2_1, 5),
                                                               (R2, t2, K2, uv2, z2, p.oct2, p.level_sigma2_2, 6))):
            sigma2 = d(sg)[np.asarray(oc, dtype=np.int64)]
            xc, yc = _dot3(R[0], x) + t[0], _dot3(R[1], x) + t[1]
            invz = (w(1) / w(z)).astype(dtype)                                 # const float invz1 = 1.0 / z1 (:1440)
            u, vv = K[0] * xc * invz + K[2], K[1] * yc * invz + K[3]           # :1445-1446
            ex, ey = u - uv[:, 0], vv - uv[:, 1]
            err, th = w(ex * ex + ey * ey), w(p.chi2_th) * w(sigma2)
            note("chi2_%d" % (side + 1), err / th - 1)
            drop(err > th, code)                                               # :1450, :1479
        dist1, dist2 = _norm3(x - O1), _norm3(x - O2)                          # :1499-1503
        note("dist", np.minimum(dist1, dist2))
        drop((dist1 == 0) | (dist2 == 0), 7)                                   # :1505
        ratio_dist = dist2 / dist1
        ratio_oct = d(p.scale_1)[np.asarray(p.oct1, dtype=np.int64)] / d(p.scale_2)[np.asarray(p.oct2, dtype=np.int64)]
        rf = dtype(p.ratio_factor)
        lo = ratio_dist * rf < ratio_oct                                       # :1516 (|| short-circuits)
        note("ratio_lo", ratio_dist * rf / ratio_oct - one)
        M[live & ~lo, mi["ratio_hi"]] = np.abs(np.asarray(ratio_dist / (ratio_oct * rf) - one, dtype=np.float64))[live & ~lo]
        drop(lo | (ratio_dist > ratio_oct * rf), 8)
    x3d = np.where((reason == 1)[:, None] | (reason == 2)[:, None], dtype(0), x).astype(dtype)
    return dict(reason=reason, x3d=x3d, n_accepted=int((reason == 0).sum()), margins=M, margin=M.min(axis=1), cos=cos, v=v)
