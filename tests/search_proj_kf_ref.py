"""NumPy yardstick of vba_search_by_projection_kf: a literal SEQUENTIAL restatement, loop for loop, of
ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cpp:354-475, over
KeyFrame::GetFeaturesInArea, src/KeyFrame.cpp:1071-1115) and of ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF,
sAlreadyFound, th, ORBdist) (:1667-1797, over Frame::GetFeaturesInArea, src/Frame.cpp:562-620).  The queries run one after the other
against a model of vpMatched / mvpMapPoints that each match mutates, exactly as the reference does; the fixed-point iteration of the
kernel is NOT used here (conflict_pass below is a prototype of it, for tests/test_search_proj_kf_ref.py).  The floating-point part
runs in the dtype asked for (float32, float64, longdouble) on the inputs as given; the bin (:1760-1765) is float32 in every dtype.

search_proj_kf_ref(p, dtype, ignore_claims=False) returns a dict: n_matches, n_before_filter, hist, ind, best_idx, best_dist, level, uv
(in the dtype), bin, state, key_match, and the margin bookkeeping of tests/fuse_ref.py (margin, n_fp: the comparisons; margin_r,
n_round: the floor and ceil arguments).  ignore_claims=True answers every query as if no query of the call had taken a keypoint
(occupied still counts): what an independent-query kernel would give.  The deviations of the entry point are restated too: a level
outside 0 .. n_levels - 1 leaves with its own state, a non-finite projection leaves as outside the image, and a match needs a
keypoint (th_dist = 256 with every candidate failing)."""
import numpy as np

from fuse_ref import _Fp, descriptor_distance, features_in_area
from search_proj_ref import HISTO, real_difference, rot_bin, three_maxima   # noqa: F401

INT_KEYS = ("n_matches", "n_before_filter", "hist", "ind", "best_idx", "best_dist", "level", "bin", "state", "key_match")


def _gates(p, T, fp):
    """phase 1 of every query: (state or None when the query reaches the area, u, v, level, radius) per query, and the uv and level
    arrays the entry point reports"""
    n = p.n_q
    reloc = bool(p.reloc)
    R, t, Ow = p.Rcw.astype(T), p.tcw.astype(T), p.Ow.astype(T)
    fx, fy, cx, cy = (T(k) for k in p.K)
    min_x, max_x, min_y, max_y = (T(b) for b in p.bounds)
    scale = p.scale.astype(T)
    th, cos_view, logsf = T(p.th), T(p.cos_view), T(p.log_scale_factor)
    level = np.full(n, -128, dtype=np.int8)
    uv = np.full((n, 2), np.nan, dtype=T)
    out = []
    for i in range(n):
        if p.q_skip[i]:                                                          # :385 / :1688-1690
            out.append((1, None, None, None, None))
            continue
        w = p.q_pos[i].astype(T)
        xc = ((R[0, 0] * w[0] + R[0, 1] * w[1]) + R[0, 2] * w[2]) + t[0]
        yc = ((R[1, 0] * w[0] + R[1, 1] * w[1]) + R[1, 2] * w[2]) + t[1]
        zc = ((R[2, 0] * w[0] + R[2, 1] * w[1]) + R[2, 2] * w[2]) + t[2]
        if not reloc:
            if fp.lt(zc, T(0)):                                                  # :395
                out.append((2, None, None, None, None))
                continue
            invz = T(1) / zc
            u = fx * (xc * invz) + cx                                            # :399-404
            v = fy * (yc * invz) + cy
            uv[i] = (u, v)
            if not (fp.ge(u, min_x) and fp.lt(u, max_x) and fp.ge(v, min_y) and fp.lt(v, max_y)):   # :407
                out.append((3, None, None, None, None))
                continue
        else:
            invz = T(1) / zc                                                     # :1698, no depth test
            u = (fx * xc) * invz + cx                                            # :1700-1701
            v = (fy * yc) * invz + cy
            uv[i] = (u, v)
            if not (np.isfinite(u) and np.isfinite(v)):                          # the deviation
                out.append((2, None, None, None, None))
                continue
            if fp.lt(u, min_x) or fp.gt(u, max_x) or fp.lt(v, min_y) or fp.gt(v, max_y):   # :1703-1706
                out.append((2, None, None, None, None))
                continue
        po = w - Ow
        dist = np.sqrt((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2])
        if fp.lt(dist, T(p.q_dist_min[i])) or fp.gt(dist, T(p.q_dist_max[i])):   # :417 / :1716
            out.append((3 if reloc else 4, None, None, None, None))
            continue
        if not reloc:
            nrm = p.q_normal[i].astype(T)
            if fp.lt((po[0] * nrm[0] + po[1] * nrm[1]) + po[2] * nrm[2], cos_view * dist):   # :423
                out.append((5, None, None, None, None))
                continue
        lv = fp.ceil(np.log(T(p.q_pred_max[i]) / dist) / logsf)                 # PredictScale (:426 / :1719)
        if not (lv >= 0 and lv < p.n_levels):                                    # the deviation: the reference indexes unchecked
            level[i] = 127 if lv >= 127 else (int(lv) if lv > -128 else -128)
            out.append((4 if reloc else 6, None, None, None, None))
            continue
        lv = int(lv)
        level[i] = lv
        out.append((None, u, v, lv, th * scale[lv]))                             # :430 / :1722
    return out, uv, level


def _search(p, T, fp, uvT, i, gate, taken):
    """the area and the candidate loop of query i: (state, best_idx, best_dist)"""
    _, u, v, lv, radius = gate
    reloc = bool(p.reloc)
    if reloc:
        cand = features_in_area(p, fp, T, uvT, u, v, radius, lv - 1, lv + 1)     # :1724
    else:
        cand = features_in_area(p, fp, T, uvT, u, v, radius)                     # :432
    if not cand:                                                                 # :434 / :1727
        return (5 if reloc else 7), -1, 256
    bd, bi = 256, -1
    for idx in cand:
        if taken(idx):                                                           # :446 / :1738
            continue
        if not reloc:
            kl = int(p.oct[idx])
            if kl < lv - 1 or kl > lv:                                           # :451
                continue
        d = descriptor_distance(p.q_desc[i], p.desc[idx])
        if d < bd:                                                               # :458 / :1745
            bd, bi = d, idx
    if not (bd <= int(p.th_dist) and bi >= 0):                                   # :466 / :1752
        return (6 if reloc else 8), bi, bd
    return 0, bi, bd


def _finish(p, T, fp, uv, level, state, best_idx, best_dist, extra=None):
    """the apply loop in query order, the histogram, ComputeThreeMaxima and the drop; the result dict"""
    n, nk = p.n_q, p.n_keys
    ori = bool(p.reloc) and bool(p.check_orientation)
    key_match = np.full(nk, -1, dtype=np.int32)
    bins = np.full(n, 255, dtype=np.uint8)
    rot_hist = [[] for _ in range(HISTO)]
    nmatches = 0
    for i in range(n):
        if state[i] != 0:
            continue
        key_match[best_idx[i]] = i                                               # :468 / :1754
        nmatches += 1
        if ori:
            b = rot_bin(p.q_angle[i], p.angle[best_idx[i]])                      # :1760-1765
            bins[i] = b
            rot_hist[b].append((int(best_idx[i]), i))
    n_before = nmatches
    hist = np.array([len(h) for h in rot_hist], dtype=np.int32)
    ind = (-1, -1, -1)
    if ori:
        ind = three_maxima(hist)
        for b in range(HISTO):
            if b not in ind:
                for bi, i in rot_hist[b]:
                    key_match[bi] = -2                                           # :1789
                    state[i] = 7
                    nmatches -= 1
    out = dict(n_matches=nmatches, n_before_filter=n_before, hist=hist, ind=np.array(ind, dtype=np.int32), best_idx=best_idx, best_dist=best_dist,
               level=level, uv=uv, bin=bins, state=state, key_match=key_match, margin=fp.margin, n_fp=fp.n_fp, margin_r=fp.margin_r, n_round=fp.n_round)
    out.update(extra or {})
    return out


def search_proj_kf_ref(p, dtype=np.float64, ignore_claims=False):
    T = np.dtype(dtype).type
    fp = _Fp()
    n, nk = p.n_q, p.n_keys
    uvT = p.uv.astype(T)
    best_idx = np.full(n, -1, dtype=np.int32)
    best_dist = np.full(n, 256, dtype=np.uint16)
    state = np.zeros(n, dtype=np.uint8)
    held = np.array(p.occupied != 0)                                             # vpMatched[idx] / mvpMapPoints[i2] != NULL
    with np.errstate(all="ignore"):
        gates, uv, level = _gates(p, T, fp)
        for i in range(n):
            if gates[i][0] is not None:
                state[i] = gates[i][0]
                continue
            state[i], best_idx[i], best_dist[i] = _search(p, T, fp, uvT, i, gates[i], lambda k: bool(held[k]))
            if state[i] == 0 and not ignore_claims:
                held[best_idx[i]] = True
    return _finish(p, T, fp, uv, level, state, best_idx, best_dist)


def conflict_pass(p, dtype=np.float64):
    """a prototype of the kernel's order-preserving conflict pass: the gates once, then rounds in which every open query q >= round
    walks against the claim table of the round before (claim[k]: -1 occupied, else the smallest query whose result is k, INT_MAX for
    none; q treats k as taken iff claim[k] < q), the table is rebuilt, until a round changes no claim.  Returns the result dict with
    `rounds`"""
    T = np.dtype(dtype).type
    fp = _Fp()
    n, nk = p.n_q, p.n_keys
    uvT = p.uv.astype(T)
    INT_MAX = 2 ** 31 - 1
    best_idx = np.full(n, -1, dtype=np.int32)
    best_dist = np.full(n, 256, dtype=np.uint16)
    state = np.zeros(n, dtype=np.uint8)
    with np.errstate(all="ignore"):
        gates, uv, level = _gates(p, T, fp)
        prev = np.full(n, -1, dtype=np.int64)
        for i in range(n):
            if gates[i][0] is not None:
                state[i] = gates[i][0]
                prev[i] = -2
        base = np.where(p.occupied != 0, -1, INT_MAX).astype(np.int64)
        claim = base.copy()
        rounds = 0
        for rnd in range(n + 1):
            changed = False
            for q in range(rnd, n):
                if prev[q] == -2:
                    continue
                state[q], best_idx[q], best_dist[q] = _search(p, T, fp, uvT, q, gates[q], lambda k: claim[k] < q)
                now = best_idx[q] if state[q] == 0 else -1
                changed |= now != prev[q]
                prev[q] = now
            rounds = rnd + 1
            if not changed:
                break
            claim = base.copy()
            for q in range(n):
                if prev[q] >= 0:
                    claim[prev[q]] = min(claim[prev[q]], q)
    return _finish(p, T, fp, uv, level, state, best_idx, best_dist, dict(rounds=rounds))


def differences(a, b):
    """names of the integer outputs in which two results differ"""
    return [k for k in INT_KEYS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
