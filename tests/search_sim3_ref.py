"""NumPy yardstick of vba_search_by_sim3: a literal sequential restatement of ORBmatcher::SearchBySim3 (src/ORBmatcher.cpp:1258-1496)
with KeyFrame::GetFeaturesInArea (src/KeyFrame.cpp:1071-1115), IsInImage (:1119-1122) and MapPoint::PredictScale
(src/MapPoint.cpp:529-540), loop for loop, on an abi.SearchSim3Problem.  The floating-point part runs in the dtype asked for
(float32, float64, longdouble) on the inputs as given; sR12, sR21 and t21 are formed in that dtype as :1277-1279 write them.

search_sim3_ref(p, dtype, form) returns a dict: n_found, match1 / match2, best_dist1 / 2, level1 / 2, state1 / 2, match12 (all
integers: the function returns no floating-point value), and the margin bookkeeping:
  margin    the smallest relative distance |lhs - rhs| / |rhs| of an evaluated <, > or >= from its threshold (a zero threshold gives an
            infinite margin, and so does a non-finite left side, which compares alike in every dtype); inf without one
  n_fp      how many comparisons were evaluated
  margin_r  the smallest distance of a floor or ceil argument from the nearest integer over max(1, |arg|)
  n_round   how many were evaluated
form = "seq" is the reference's candidate loop; form = "min" takes, among the candidates that pass the level gate, the smallest
distance and, among equals, the first in walk order.  The one deviation of vba_search_by_sim3 is restated too: a predicted level
outside 0 .. n_levels - 1 of the target leaves with state 6, where the reference reads mvScaleFactors unchecked (:1354, :1439).
The state codes are those of include/vislam_ba.h."""
import numpy as np

from fuse_ref import _Fp, descriptor_distance, features_in_area


def _direction(fp, T, src, tgt, Rs, ts, sR, t, K, th, th_high, form):
    """one of the two loops (:1310-1392, :1398-1475): the keypoints of src with their map points into tgt"""
    n = src.n_keys
    fx, fy, cx, cy = (T(k) for k in K)
    min_x, max_x, min_y, max_y = (T(b) for b in tgt.bounds)
    uvT = tgt.uv.astype(T)
    scale, logsf = tgt.scale.astype(T), T(tgt.log_scale_factor)
    n_levels = tgt.n_levels
    match = np.full(n, -1, dtype=np.int32)
    best_dist = np.full(n, 256, dtype=np.uint16)
    level = np.full(n, -128, dtype=np.int8)
    state = np.zeros(n, dtype=np.uint8)
    mul = lambda M, b, w: ((M[0] * w[0] + M[1] * w[1]) + M[2] * w[2]) + b
    for i in range(n):
        if not src.has_pt[i]:                                                    # :1314, :1317
            state[i] = 1
            continue
        if src.matched[i]:                                                       # :1314
            state[i] = 2
            continue
        w = src.pos[i].astype(T)
        c1 = [mul(Rs[r], ts[r], w) for r in range(3)]                            # :1321
        xc, yc, zc = (mul(sR[r], t[r], c1) for r in range(3))                    # :1322
        if fp.lt(zc, T(0)):                                                      # :1325
            state[i] = 3
            continue
        invz = T(1) / zc
        u = fx * (xc * invz) + cx
        v = fy * (yc * invz) + cy
        if not (fp.ge(u, min_x) and fp.lt(u, max_x) and fp.ge(v, min_y) and fp.lt(v, max_y)):   # :1337
            state[i] = 4
            continue
        dist3d = np.sqrt((xc * xc + yc * yc) + zc * zc)                          # :1342
        if fp.lt(dist3d, T(src.dist_min[i])) or fp.gt(dist3d, T(src.dist_max[i])):   # :1345
            state[i] = 5
            continue
        lv = fp.ceil(np.log(T(src.pred_max[i]) / dist3d) / logsf)                # PredictScale
        if not (lv >= 0 and lv < n_levels):                                      # the deviation
            state[i] = 6
            level[i] = 127 if lv >= 127 else (int(lv) if lv > -128 else -128)
            continue
        lv = int(lv)
        level[i] = lv
        radius = T(th) * scale[lv]                                               # :1354
        cand = features_in_area(tgt, fp, T, uvT, u, v, radius)
        if not cand:                                                             # :1359
            state[i] = 7
            continue
        best, bidx = 256, -1                                                     # 256 stands for INT_MAX
        passing = []
        for pos_in_walk, idx in enumerate(cand):
            kl = int(tgt.oct[idx])
            if kl < lv - 1 or kl > lv:                                           # :1374
                continue
            dist = descriptor_distance(src.pt_desc[i], tgt.desc[idx])
            passing.append((dist, pos_in_walk, idx))
            if dist < best:                                                      # :1381
                best, bidx = dist, idx
        if form == "min" and passing:
            best, _, bidx = min(passing)
        best_dist[i] = best
        if bidx >= 0 and best <= int(th_high):                                   # :1388 (INT_MAX is above every TH_HIGH)
            match[i] = bidx
        else:
            state[i] = 8
    return match, best_dist, level, state


def transforms(p, T):
    """sR12, sR21, t21 in dtype T, in the order :1277-1279 write them"""
    s12, R12, t12 = T(p.s12), p.R12.astype(T), p.t12.astype(T)
    sR12 = s12 * R12
    sR21 = (T(1) / s12) * R12.T
    m = -sR21
    t21 = np.array([(m[r, 0] * t12[0] + m[r, 1] * t12[1]) + m[r, 2] * t12[2] for r in range(3)], dtype=T)
    return sR12, sR21, t21


def search_sim3_ref(p, dtype=np.float64, form="seq"):
    T = np.dtype(dtype).type
    fp = _Fp()
    with np.errstate(all="ignore"):
        sR12, sR21, t21 = transforms(p, T)
        a, b = p.kf1, p.kf2
        m1, d1, l1, s1 = _direction(fp, T, a, b, a.Rcw.astype(T), a.tcw.astype(T), sR21, t21, p.K, p.th, p.th_high, form)
        m2, d2, l2, s2 = _direction(fp, T, b, a, b.Rcw.astype(T), b.tcw.astype(T), sR12, p.t12.astype(T), p.K, p.th, p.th_high, form)
    match12 = np.full(a.n_keys, -1, dtype=np.int32)
    for i1 in range(a.n_keys):                                                   # :1480-1493
        idx2 = int(m1[i1])
        if idx2 >= 0 and int(m2[idx2]) == i1:
            match12[i1] = idx2
    return dict(n_found=int((match12 >= 0).sum()), match1=m1, match2=m2, best_dist1=d1, best_dist2=d2, level1=l1, level2=l2, state1=s1, state2=s2,
                match12=match12, margin=fp.margin, n_fp=fp.n_fp, margin_r=fp.margin_r, n_round=fp.n_round)


INT_KEYS = ("n_found", "match1", "match2", "best_dist1", "best_dist2", "level1", "level2", "state1", "state2", "match12")


def differences(a, b):
    """names of the outputs in which two results differ"""
    return [k for k in INT_KEYS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
