"""NumPy yardstick of vba_fuse: a literal sequential restatement of the search half of ORBmatcher::Fuse (src/ORBmatcher.cpp:958-1119;
the Sim3 overload :1123-1254 is the same search without the reprojection gate) with KeyFrame::GetFeaturesInArea
(src/KeyFrame.cpp:1071-1115), IsInImage (:1119-1122) and MapPoint::PredictScale (src/MapPoint.cpp:529-540), loop for loop.  The
floating-point part runs in the dtype asked for (float32, float64, longdouble) on the inputs as given.

fuse_ref(p, dtype, form) returns a dict: n_found, best_idx, best_dist, level, uv (in the dtype), state, and the margin bookkeeping:
  margin    the smallest relative distance |lhs - rhs| / |rhs| of an evaluated <, > or >= from its threshold (a zero threshold gives an
            infinite margin, and so does a non-finite left side, which compares alike in every dtype); inf without one
  n_fp      how many comparisons were evaluated
  margin_r  the smallest distance of a floor or ceil argument from the nearest integer over max(1, |arg|)
  n_round   how many were evaluated
form = "seq" is the reference's loop; form = "min" takes, among the candidates that pass every test, the smallest distance and,
among equals, the first in walk order.  The one deviation of vba_fuse is restated too: the level range check of :1027 runs in
both modes."""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance: the Hamming distance of two 32-byte rows"""
    return int(_POP[np.bitwise_xor(a, b)].sum())


class _Fp:
    """comparisons and roundings in one dtype, with the margin bookkeeping"""

    def __init__(self):
        self.margin = np.inf
        self.n_fp = 0
        self.margin_r = np.inf
        self.n_round = 0

    def _note(self, lhs, rhs):
        self.n_fp += 1
        if rhs != 0 and np.isfinite(lhs):
            self.margin = min(self.margin, float(abs(lhs - rhs) / abs(rhs)))

    def lt(self, lhs, rhs):
        self._note(lhs, rhs)
        return bool(lhs < rhs)

    def gt(self, lhs, rhs):
        self._note(lhs, rhs)
        return bool(lhs > rhs)

    def ge(self, lhs, rhs):
        self._note(lhs, rhs)
        return bool(lhs >= rhs)

    def _round(self, x, fn):
        self.n_round += 1
        if np.isfinite(x):
            self.margin_r = min(self.margin_r, float(abs(x - np.rint(x)) / max(1.0, abs(float(x)))))
        return fn(x)

    def floor(self, x):
        return self._round(x, np.floor)

    def ceil(self, x):
        return self._round(x, np.ceil)


def _to_int(x):
    """(int) of a floored or ceiled value; the cases keep these far inside the int range"""
    return int(x)


def cell_range(p, fp, T, x, y, r):
    """the clamped cell range (nMinCellX, nMaxCellX, nMinCellY, nMaxCellY) of GetFeaturesInArea; None after one of its four returns"""
    min_x, min_y = T(p.bounds[0]), T(p.bounds[2])
    iw, ih = T(p.grid_inv_w), T(p.grid_inv_h)
    cols, rows = int(p.grid_cols), int(p.grid_rows)
    n_min_x = max(0, _to_int(fp.floor((x - min_x - r) * iw)))
    if n_min_x >= cols:
        return None
    n_max_x = min(cols - 1, _to_int(fp.ceil((x - min_x + r) * iw)))
    if n_max_x < 0:
        return None
    n_min_y = max(0, _to_int(fp.floor((y - min_y - r) * ih)))
    if n_min_y >= rows:
        return None
    n_max_y = min(rows - 1, _to_int(fp.ceil((y - min_y + r) * ih)))
    if n_max_y < 0:
        return None
    return n_min_x, n_max_x, n_min_y, n_max_y


def features_in_area(p, fp, T, uvT, x, y, r, min_level=-1, max_level=-1):
    """KeyFrame::GetFeaturesInArea(x, y, r) and Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) (src/Frame.cpp:562-620, the same
    walk with a level filter in front of the pixel test; the defaults switch it off): the keypoint indices in walk order"""
    out = []
    cells = cell_range(p, fp, T, x, y, r)
    if cells is None:
        return out
    n_min_x, n_max_x, n_min_y, n_max_y = cells
    rows = int(p.grid_rows)
    check_levels = (min_level > 0) or (max_level >= 0)
    for ix in range(n_min_x, n_max_x + 1):
        for iy in range(n_min_y, n_max_y + 1):
            c = ix * rows + iy
            for j in range(p.cell_begin[c], p.cell_begin[c + 1]):
                idx = int(p.cell_feat[j])
                if check_levels:
                    if int(p.oct[idx]) < min_level:
                        continue
                    if max_level >= 0:
                        if int(p.oct[idx]) > max_level:
                            continue
                distx = uvT[idx, 0] - x
                disty = uvT[idx, 1] - y
                if fp.lt(abs(distx), r) and fp.lt(abs(disty), r):
                    out.append(idx)
    return out


def fuse_ref(p, dtype=np.float64, form="seq"):
    T = np.dtype(dtype).type
    fp = _Fp()
    n = p.n_pt
    R, t, Ow = p.Rcw.astype(T), p.tcw.astype(T), p.Ow.astype(T)
    fx, fy, cx, cy = (T(k) for k in p.K)
    min_x, max_x, min_y, max_y = (T(b) for b in p.bounds)
    uvT = p.uv.astype(T)
    scale, inv_sigma2 = p.scale.astype(T), p.inv_level_sigma2.astype(T)
    th, cos_view, chi2, logsf = T(p.th), T(p.cos_view), T(p.chi2_reproj), T(p.log_scale_factor)
    n_levels, th_low = p.n_levels, int(p.th_low)
    best_idx = np.full(n, -1, dtype=np.int32)
    best_dist = np.full(n, 256, dtype=np.uint16)
    level = np.full(n, -128, dtype=np.int8)
    uv = np.full((n, 2), np.nan, dtype=T)
    state = np.zeros(n, dtype=np.uint8)
    with np.errstate(all="ignore"):
        for i in range(n):
            if p.skip[i]:
                state[i] = 1
                continue
            w = p.pos[i].astype(T)
            xc = ((R[0, 0] * w[0] + R[0, 1] * w[1]) + R[0, 2] * w[2]) + t[0]
            yc = ((R[1, 0] * w[0] + R[1, 1] * w[1]) + R[1, 2] * w[2]) + t[1]
            zc = ((R[2, 0] * w[0] + R[2, 1] * w[1]) + R[2, 2] * w[2]) + t[2]
            if fp.lt(zc, T(0)):                                                  # :991
                state[i] = 2
                continue
            invz = T(1) / zc
            u = fx * (xc * invz) + cx
            v = fy * (yc * invz) + cy
            uv[i] = (u, v)
            if not (fp.ge(u, min_x) and fp.lt(u, max_x) and fp.ge(v, min_y) and fp.lt(v, max_y)):   # :1004
                state[i] = 3
                continue
            po = w - Ow
            dist3d = np.sqrt((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2])
            if fp.lt(dist3d, T(p.dist_min[i])) or fp.gt(dist3d, T(p.dist_max[i])):   # :1016
                state[i] = 4
                continue
            nrm = p.normal[i].astype(T)
            if fp.lt((po[0] * nrm[0] + po[1] * nrm[1]) + po[2] * nrm[2], cos_view * dist3d):   # :1023
                state[i] = 5
                continue
            lv = fp.ceil(np.log(T(p.pred_max[i]) / dist3d) / logsf)            # PredictScale
            if not (lv >= 0 and lv < n_levels):                                  # :1027
                state[i] = 6
                level[i] = 127 if lv >= 127 else (int(lv) if lv > -128 else -128)
                continue
            lv = int(lv)
            level[i] = lv
            radius = th * scale[lv]                                              # :1031
            cand = features_in_area(p, fp, T, uvT, u, v, radius)
            if not cand:                                                         # :1034
                state[i] = 7
                continue
            best, bidx = 256, -1
            passing = []
            for pos_in_walk, idx in enumerate(cand):
                kl = int(p.oct[idx])
                if kl < lv - 1 or kl > lv:                                       # :1052
                    continue
                if p.check_reproj:
                    ex = u - uvT[idx, 0]
                    ey = v - uvT[idx, 1]
                    if fp.gt((ex * ex + ey * ey) * inv_sigma2[kl], chi2):        # :1079
                        continue
                dist = descriptor_distance(p.pt_desc[i], p.desc[idx])
                passing.append((dist, pos_in_walk, idx))
                if dist < best:                                                  # :1087
                    best, bidx = dist, idx
            if form == "min" and passing:
                best, _, bidx = min(passing)
            best_idx[i], best_dist[i] = bidx, best
            state[i] = 0 if best <= th_low else 8                               # :1095
    return dict(n_found=int((state == 0).sum()), best_idx=best_idx, best_dist=best_dist, level=level, uv=uv, state=state,
                margin=fp.margin, n_fp=fp.n_fp, margin_r=fp.margin_r, n_round=fp.n_round)


INT_KEYS = ("n_found", "best_idx", "best_dist", "level", "state")


def differences(a, b):
    """names of the integer outputs in which two results differ"""
    return [k for k in INT_KEYS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


def uv_difference(a, b):
    """the largest |uv_a - uv_b| over the points whose projection both hold finite; inf if their non-finite patterns differ"""
    ua, ub = np.asarray(a["uv"], dtype=np.longdouble), np.asarray(b["uv"], dtype=np.longdouble)
    fa, fb = np.isfinite(ua), np.isfinite(ub)
    same = np.array_equal(fa, fb) and np.array_equal(np.isnan(ua), np.isnan(ub)) and np.array_equal(ua[~fa & ~np.isnan(ua)], ub[~fb & ~np.isnan(ub)])
    if not same:
        return np.inf
    return float(np.abs(ua[fa] - ub[fa]).max()) if fa.any() else 0.0
