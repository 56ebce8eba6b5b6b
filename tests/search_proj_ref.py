"""NumPy yardstick of vba_search_by_projection: a literal SEQUENTIAL restatement, loop for loop, of
ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cpp:1511-1665, monocular) and of Frame::isInFrustum
(src/Frame.cpp:492-550) followed by ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cpp:63-156), both over
Frame::GetFeaturesInArea (src/Frame.cpp:562-620).  The queries run one after the other against a model of mvpMapPoints that each
match mutates, exactly as the reference does; the fixed-point iteration of the kernel is NOT used here.  The floating-point part runs
in the dtype asked for (float32, float64, longdouble) on the inputs as given; the ratio test (:147) and the bin (:1628-1633) are
float32 in every dtype, as the reference computes them.

search_proj_ref(p, dtype, ignore_claims=False) returns a dict: n_matches, n_before_filter, hist, ind, best_idx, best_dist, best_dist2,
level, view_cos and uv (in the dtype), bin, state, key_match, and the margin bookkeeping of tests/fuse_ref.py (margin, n_fp,
margin_r, n_round).  ignore_claims=True answers every query as if no query of the call had claimed a keypoint (occupied still
counts): what an independent-query kernel would give.  The one deviation of the entry point is restated too: a non-finite
projection leaves with state 3; and a match needs a keypoint (th_high = 256 with every candidate taken)."""
import numpy as np

from fuse_ref import _Fp, descriptor_distance, features_in_area

HISTO = 30


def three_maxima(hist):
    """ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cpp:1800-1841) over the bin sizes"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(hist):
        s = int(s)
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def rot_bin(angle_q, angle_k):
    """:1628-1633 in float32 with C round"""
    rot = np.float32(angle_q) - np.float32(angle_k)
    if rot < 0.0:
        rot = np.float32(rot + np.float32(360.0))
    t = np.float32(rot * np.float32(np.float32(1.0) / np.float32(HISTO)))
    b = int(np.sign(t) * np.floor(np.abs(t) + np.float32(0.5)))
    return 0 if b == HISTO else b


def search_proj_ref(p, dtype=np.float64, ignore_claims=False):
    T = np.dtype(dtype).type
    fp = _Fp()
    n, nk = p.n_q, p.n_keys
    local = bool(p.local)
    ori = (not local) and bool(p.check_orientation)
    R, t, Ow = p.Rcw.astype(T), p.tcw.astype(T), p.Ow.astype(T)
    fx, fy, cx, cy = (T(k) for k in p.K)
    min_x, max_x, min_y, max_y = (T(b) for b in p.bounds)
    uvT = p.uv.astype(T)
    scale = p.scale.astype(T)
    th, cos_view, logsf = T(p.th), T(p.cos_view), T(p.log_scale_factor)
    nn_ratio = np.float32(p.nn_ratio)
    n_levels, th_high = p.n_levels, int(p.th_high)
    best_idx = np.full(n, -1, dtype=np.int32)
    best_dist = np.full(n, 256, dtype=np.uint16)
    best_dist2 = np.full(n, 256, dtype=np.uint16)
    level = np.full(n, -128, dtype=np.int8)
    view_cos = np.full(n, np.nan, dtype=T)
    uv = np.full((n, 2), np.nan, dtype=T)
    bins = np.full(n, 255, dtype=np.uint8)
    state = np.zeros(n, dtype=np.uint8)
    # mvpMapPoints of the frame: ORIG = what the frame held before the call (taken iff occupied), else the query that wrote it last
    ORIG = -1
    holder = np.full(nk, ORIG, dtype=np.int64)
    rot_hist = [[] for _ in range(HISTO)]
    nmatches = 0

    def taken(k):
        if holder[k] == ORIG or ignore_claims:
            return bool(p.occupied[k])
        return bool(p.q_blocks[holder[k]])

    with np.errstate(all="ignore"):
        for i in range(n):
            if p.q_skip[i]:
                state[i] = 1
                continue
            w = p.q_pos[i].astype(T)
            xc = ((R[0, 0] * w[0] + R[0, 1] * w[1]) + R[0, 2] * w[2]) + t[0]
            yc = ((R[1, 0] * w[0] + R[1, 1] * w[1]) + R[1, 2] * w[2]) + t[1]
            zc = ((R[2, 0] * w[0] + R[2, 1] * w[1]) + R[2, 2] * w[2]) + t[2]
            invz = T(1) / zc
            if (fp.lt(zc, T(0)) if local else fp.lt(invz, T(0))):               # Frame.cpp:506 / ORBmatcher.cpp:1553
                state[i] = 2
                continue
            u = (fx * xc) * invz + cx
            v = (fy * yc) * invz + cy
            uv[i] = (u, v)
            if not (np.isfinite(u) and np.isfinite(v)):                          # the deviation
                state[i] = 3
                continue
            if fp.lt(u, min_x) or fp.gt(u, max_x) or fp.lt(v, min_y) or fp.gt(v, max_y):   # :513-516 / :1559-1562
                state[i] = 3
                continue
            if local:
                po = w - Ow
                dist = np.sqrt((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2])
                if fp.lt(dist, T(p.q_dist_min[i])) or fp.gt(dist, T(p.q_dist_max[i])):    # :525
                    state[i] = 4
                    continue
                nrm = p.q_normal[i].astype(T)
                vc = ((po[0] * nrm[0] + po[1] * nrm[1]) + po[2] * nrm[2]) / dist
                view_cos[i] = vc
                if fp.lt(vc, cos_view):                                          # :532
                    state[i] = 5
                    continue
                lv = fp.ceil(np.log(T(p.q_pred_max[i]) / dist) / logsf)         # PredictScale
                if not (lv >= 0 and lv < n_levels):                              # :537
                    state[i] = 6
                    level[i] = 127 if lv >= 127 else (int(lv) if lv > -128 else -128)
                    continue
                lv = int(lv)
                level[i] = lv
                r = T(2.5) if fp.gt(vc, T(0.998)) else T(4.0)                   # RadiusByViewingCos
                if th != T(1.0):                                                 # :67, :88
                    r = r * th
                radius = r * scale[lv]                                           # :93
                lo, hi = lv - 1, lv
            else:
                o = int(p.q_oct[i])
                radius = th * scale[o]                                           # :1567
                lo, hi = o - 1, o + 1                                            # :1580
            cand = features_in_area(p, fp, T, uvT, u, v, radius, lo, hi)
            if not cand:                                                         # :96 / :1582
                state[i] = 7 if local else 4
                continue
            bd, bd2, bl, bl2, bi = 256, 256, -1, -1, -1
            for idx in cand:
                if taken(idx):                                                   # :113-115 / :1596-1598
                    continue
                dist_h = descriptor_distance(p.q_desc[i], p.desc[idx])
                if dist_h < bd:                                                  # :129-141 / :1613
                    bd2, bd = bd, dist_h
                    bl2, bl = bl, int(p.oct[idx])
                    bi = idx
                elif dist_h < bd2:
                    bl2, bd2 = int(p.oct[idx]), dist_h
            best_idx[i], best_dist[i] = bi, bd
            if local:
                best_dist2[i] = bd2
            if not (bd <= th_high and bi >= 0):                                  # :145 / :1621
                state[i] = 8 if local else 5
                continue
            if local and bl == bl2 and np.float32(bd) > nn_ratio * np.float32(bd2):   # :147, the product in float32
                state[i] = 9
                continue
            holder[bi] = i                                                       # :150 / :1623
            nmatches += 1
            state[i] = 0
            if ori:
                b = rot_bin(p.q_angle[i], p.angle[bi])
                bins[i] = b
                rot_hist[b].append((bi, i))
    n_before = nmatches
    hist = np.array([len(h) for h in rot_hist], dtype=np.int32)
    ind = (-1, -1, -1)
    key_match = holder.astype(np.int32)
    if ori:
        ind = three_maxima(hist)
        for b in range(HISTO):
            if b not in ind:
                for bi, i in rot_hist[b]:
                    key_match[bi] = -2                                           # :1657
                    state[i] = 6
                    nmatches -= 1
    return dict(n_matches=nmatches, n_before_filter=n_before, hist=hist, ind=np.array(ind, dtype=np.int32), best_idx=best_idx, best_dist=best_dist,
                best_dist2=best_dist2, level=level, view_cos=view_cos, uv=uv, bin=bins, state=state, key_match=key_match,
                margin=fp.margin, n_fp=fp.n_fp, margin_r=fp.margin_r, n_round=fp.n_round)


INT_KEYS = ("n_matches", "n_before_filter", "hist", "ind", "best_idx", "best_dist", "best_dist2", "level", "bin", "state", "key_match")


def differences(a, b):
    """names of the integer outputs in which two results differ"""
    return [k for k in INT_KEYS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


def real_difference(a, b, key):
    """the largest |a - b| of a floating-point output over the entries both hold finite; inf if their non-finite patterns differ"""
    ua, ub = np.asarray(a[key], dtype=np.longdouble), np.asarray(b[key], dtype=np.longdouble)
    fa, fb = np.isfinite(ua), np.isfinite(ub)
    same = np.array_equal(fa, fb) and np.array_equal(np.isnan(ua), np.isnan(ub)) and np.array_equal(ua[~fa & ~np.isnan(ua)], ub[~fb & ~np.isnan(ub)])
    if not same:
        return np.inf
    return float(np.abs(ua[fa] - ub[fa]).max()) if fa.any() else 0.0
