"""NumPy restatement of Sim3Solver::iterate / ComputeSim3 / CheckInliers (src/Sim3Solver.cpp:138-220, :253-359, :363-388): the
yardstick of vba_sim3_ransac (test infrastructure, like sim3_ref.py).

Everything runs in the dtype asked for (np.float32: what the reference's CV_32F does, np.float64: what the library does,
np.longdouble: the yardstick's own error bar).  The eigen-solve is a cyclic Jacobi iteration written out here so that it runs in all
three; the rotation is formed by the reference's route (atan2 of the eigenvector's parts, then Rodrigues, :305-312).  All
hypotheses of a call are computed side by side (arrays over the hypothesis index).

Per hypothesis the yardstick also reports the two numbers the GPU comparison rests on:
  gap     (lambda1 - lambda2) / |lambda1| of Horn's N: how well the dominant eigenvector is determined
  margin  the smallest |err / gate - 1| over all pairs and both sides: how far the closest pair is from changing its flag
"""
import numpy as np

SWEEPS = {np.float32: 8, np.float64: 8, np.longdouble: 12}
_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def jacobi4(N, dtype=np.float64):
    """eigenvalues [H,4] (unsorted) and eigenvectors [H,4,4] (columns) of symmetric N [H,4,4]: cyclic Jacobi, fixed sweeps"""
    A = np.array(N, dtype=dtype)
    H = A.shape[0]
    V = np.zeros((H, 4, 4), dtype=dtype)
    for i in range(4):
        V[:, i, i] = 1
    one, two = dtype(1), dtype(2)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS[dtype]):
            for p, q in _PAIRS:
                apq = A[:, p, q].copy()
                theta = (A[:, q, q] - A[:, p, p]) / (two * apq)
                t = np.copysign(one, theta) / (np.abs(theta) + np.sqrt(theta * theta + one))
                t = np.where(apq == 0, dtype(0), t).astype(dtype)
                c = one / np.sqrt(t * t + one)
                s = t * c
                A[:, p, p] -= t * apq
                A[:, q, q] += t * apq
                A[:, p, q] = 0
                A[:, q, p] = 0
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                        A[:, r, p] = A[:, p, r] = c * arp - s * arq
                        A[:, r, q] = A[:, q, r] = s * arp + c * arq
                    vrp, vrq = V[:, r, p].copy(), V[:, r, q].copy()
                    V[:, r, p] = c * vrp - s * vrq
                    V[:, r, q] = s * vrp + c * vrq
    return A[:, np.arange(4), np.arange(4)], V


def horn_N(p, samples, dtype):
    """centroids, centred triples and Horn's N of every hypothesis (:256-293)"""
    P1 = np.asarray(p.p1c, dtype=dtype)[samples]   # [H,3 points,3 xyz]
    P2 = np.asarray(p.p2c, dtype=dtype)[samples]
    three = dtype(3)
    O1 = ((P1[:, 0] + P1[:, 1]) + P1[:, 2]) / three
    O2 = ((P2[:, 0] + P2[:, 1]) + P2[:, 2]) / three
    Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
    M = np.zeros((len(samples), 3, 3), dtype=dtype)   # M = Pr2 Pr1^T
    for a in range(3):
        for b in range(3):
            M[:, a, b] = (Pr2[:, 0, a] * Pr1[:, 0, b] + Pr2[:, 1, a] * Pr1[:, 1, b]) + Pr2[:, 2, a] * Pr1[:, 2, b]
    N = np.zeros((len(samples), 4, 4), dtype=dtype)
    N[:, 0, 0] = (M[:, 0, 0] + M[:, 1, 1]) + M[:, 2, 2]
    N[:, 0, 1] = N[:, 1, 0] = M[:, 1, 2] - M[:, 2, 1]
    N[:, 0, 2] = N[:, 2, 0] = M[:, 2, 0] - M[:, 0, 2]
    N[:, 0, 3] = N[:, 3, 0] = M[:, 0, 1] - M[:, 1, 0]
    N[:, 1, 1] = (M[:, 0, 0] - M[:, 1, 1]) - M[:, 2, 2]
    N[:, 1, 2] = N[:, 2, 1] = M[:, 0, 1] + M[:, 1, 0]
    N[:, 1, 3] = N[:, 3, 1] = M[:, 2, 0] + M[:, 0, 2]
    N[:, 2, 2] = (-M[:, 0, 0] + M[:, 1, 1]) - M[:, 2, 2]
    N[:, 2, 3] = N[:, 3, 2] = M[:, 1, 2] + M[:, 2, 1]
    N[:, 3, 3] = (-M[:, 0, 0] - M[:, 1, 1]) + M[:, 2, 2]
    return O1, O2, Pr1, Pr2, N


def hypotheses(p, samples, dtype=np.float64):
    """ComputeSim3 of every triple of samples [H,3]: dict of sR12 [H,3,3], t12 [H,3], sR21, t21, t, q (xyzw, unit eigenvector with
    w >= 0), s, gap"""
    samples = np.asarray(samples, dtype=np.int64).reshape(-1, 3)
    H = len(samples)
    O1, O2, Pr1, Pr2, N = horn_N(p, samples, dtype)
    lam, V = jacobi4(N, dtype)
    with np.errstate(all="ignore"):
        k = np.argmax(lam, axis=1)   # the first one among equals, as the kernel
        e = V[np.arange(H), :, k]    # (w, x, y, z)
        ls = np.sort(lam, axis=1)
        gap = (ls[:, 3] - ls[:, 2]) / np.abs(ls[:, 3])
        # rotation: ang = atan2(|vec|, w); vec = 2 ang vec / |vec|; Rodrigues (:305-312)
        vec = e[:, 1:4]
        nv = np.sqrt((vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1]) + vec[:, 2] * vec[:, 2])
        th = dtype(2) * np.arctan2(nv, e[:, 0])
        ax = vec / np.where(nv == 0, dtype(1), nv)[:, None]   # |vec| == 0 is the identity (the reference divides 0 by 0 there)
        sn, cs = np.sin(th), np.cos(th)
        K = np.zeros((H, 3, 3), dtype=dtype)
        K[:, 0, 1], K[:, 0, 2] = -ax[:, 2], ax[:, 1]
        K[:, 1, 0], K[:, 1, 2] = ax[:, 2], -ax[:, 0]
        K[:, 2, 0], K[:, 2, 1] = -ax[:, 1], ax[:, 0]
        R = np.eye(3, dtype=dtype)[None] + sn[:, None, None] * K + (dtype(1) - cs)[:, None, None] * (K @ K)
        R = R.astype(dtype)
        if p.fix_scale:
            s = np.ones(H, dtype=dtype)
        else:
            P3 = np.einsum("hab,hib->hia", R, Pr2)   # R Pr2, per point
            nom = np.zeros(H, dtype=dtype)
            den = np.zeros(H, dtype=dtype)
            for i in range(3):
                nom = nom + ((Pr1[:, i, 0] * P3[:, i, 0] + Pr1[:, i, 1] * P3[:, i, 1]) + Pr1[:, i, 2] * P3[:, i, 2])
                den = den + ((P3[:, i, 0] * P3[:, i, 0] + P3[:, i, 1] * P3[:, i, 1]) + P3[:, i, 2] * P3[:, i, 2])
            s = nom / den
        t = O1 - s[:, None] * np.einsum("hab,hb->ha", R, O2)
        sR12 = s[:, None, None] * R
        sR21 = (dtype(1) / s)[:, None, None] * np.transpose(R, (0, 2, 1))
        t21 = -np.einsum("hab,hb->ha", sR21, t)
        en = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + (e[:, 2] * e[:, 2] + e[:, 3] * e[:, 3]))
        sg = np.where(e[:, 0] < 0, dtype(-1), dtype(1))
        q = (sg / en)[:, None] * e[:, [1, 2, 3, 0]]
    out = dict(sR12=sR12, t12=t, sR21=sR21, t21=t21, t=t, q=q, s=s, gap=gap, lam=lam, V=V, N=N)
    return {k_: np.asarray(v, dtype=dtype) for k_, v in out.items()}


def hypothesis(p, triple, dtype=np.float64):
    """ComputeSim3 of one triple: the entries of hypotheses() without the leading axis"""
    return {k: v[0] for k, v in hypotheses(p, [triple], dtype).items()}


def _pixel(K, P, dtype):
    invz = dtype(1) / P[..., 2]
    return np.stack([K[0] * (P[..., 0] * invz) + K[2], K[1] * (P[..., 1] * invz) + K[3]], axis=-1)


def check_inliers(p, hyp, dtype=np.float64):
    """CheckInliers (:363-388) of every hypothesis: flags [H,n] bool, margin [H]"""
    p1 = np.asarray(p.p1c, dtype=dtype)
    p2 = np.asarray(p.p2c, dtype=dtype)
    K1, K2 = np.asarray(p.K1, dtype=dtype), np.asarray(p.K2, dtype=dtype)
    g1, g2 = np.asarray(p.max_err1, dtype=dtype), np.asarray(p.max_err2, dtype=dtype)
    H, n = hyp["s"].shape[0], p1.shape[0]
    with np.errstate(all="ignore"):
        im1, im2 = _pixel(K1, p1, dtype), _pixel(K2, p2, dtype)
        y = np.einsum("hab,ib->hia", hyp["sR12"], p2) + hyp["t12"][:, None]
        z = np.einsum("hab,ib->hia", hyp["sR21"], p1) + hyp["t21"][:, None]
        d1 = im1[None] - _pixel(K1, y.astype(dtype), dtype)
        d2 = _pixel(K2, z.astype(dtype), dtype) - im2[None]
        e1 = d1[..., 0] * d1[..., 0] + d1[..., 1] * d1[..., 1]
        e2 = d2[..., 0] * d2[..., 0] + d2[..., 1] * d2[..., 1]
        flags = (e1 < g1[None]) & (e2 < g2[None])
        if n:
            m = np.minimum(np.abs(e1 / g1[None] - 1), np.abs(e2 / g2[None] - 1))
            margin = np.where(np.isfinite(m), m, np.inf).min(axis=1)
        else:
            margin = np.full(H, np.inf)
    return flags, np.asarray(margin, dtype=np.float64)


def counts(p, samples, dtype=np.float64):
    """inlier count of every hypothesis [H] int32 (and the flags, the margins and the hypotheses they come from)"""
    samples = np.asarray(samples, dtype=np.int64).reshape(-1, 3)
    if len(samples) == 0:
        return np.zeros(0, dtype=np.int32), np.zeros((0, p.n_pairs), dtype=bool), np.zeros(0), None
    hyp = hypotheses(p, samples, dtype)
    flags, margin = check_inliers(p, hyp, dtype)
    return flags.sum(axis=1).astype(np.int32), flags, margin, hyp


def scan(c, min_inliers, best):
    """iterate's accept rule (:193-211) over the counts in order: (hit, its_done, best_hyp, best_inliers)"""
    b, best_hyp, hit = int(best), -1, -1
    for h, ch in enumerate(c):
        if ch >= b:                 # a later tie replaces the best (:193)
            b, best_hyp = int(ch), h
            if ch > min_inliers:    # strict (:203)
                hit = h
                break
    return hit, (hit + 1 if hit >= 0 else len(c)), best_hyp, b


def ransac(p, dtype=np.float64):
    """what vba_sim3_ransac returns for abi.Sim3RansacProblem p, plus gap and margin per hypothesis"""
    c, flags, margin, hyp = counts(p, p.sample, dtype)
    hit, its_done, best_hyp, b = scan(c, p.min_inliers, p.best_inliers)
    S = lambda h: np.concatenate([hyp["t"][h], hyp["q"][h], [hyp["s"][h]]]).astype(dtype)
    return dict(hyp_inliers=c, hit=hit, its_done=its_done, best_hyp=best_hyp, best_inliers=b,
                n_inliers=int(c[hit]) if hit >= 0 else 0,
                S12=S(hit) if hit >= 0 else None, inlier=flags[hit].astype(np.uint8) if hit >= 0 else None,
                best_S12=S(best_hyp) if best_hyp >= 0 else np.asarray(p.best_S12, dtype=dtype),
                gap=None if hyp is None else np.asarray(hyp["gap"], dtype=np.float64), margin=margin, hyp=hyp, flags=flags)
