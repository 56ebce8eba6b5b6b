"""NumPy restatement of MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:336-413) and MapPoint::UpdateNormalAndDepth
(:450-501) over an abi.MapPointProblem: the yardstick of vba_mappoint_update.

Descriptor part: the observations of good keyframes, the full Hamming matrix with its diagonal of 0, per row the entry
(int)(0.5 * (N - 1)) of the sorted row (np.partition), the first row with the smallest median (np.argmin).  best_obs indexes the
point's observation list, bad keyframes counted.

Normal part in three modes.  float64 and longdouble: the unit vectors summed in observation order, over ALL observations, then
divided by their count; dist * ref_scale and that / ref_top_scale.  float32: the reference's own arithmetic on the inputs narrowed
to float32 -- cv::Mat CV_32F subtraction, cv::norm accumulating the squares in double, `normali / norm` as a float32 product with
the float32 reciprocal (cv::Mat::convertTo scales 32F data with a float32 factor), float32 sums, `normal / n` likewise, (float)norm
for dist and float32 products for the two distances.  A point in an observer's camera centre (a norm of exactly 0) leaves with
normal_state 3 in every mode: the declared deviation (the reference stores NaN)."""
import numpy as np

from mc_slam_amd import abi

_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


def hamming_matrix(d):
    """[N,32] uint8 -> [N,N] int32, ORBmatcher::DescriptorDistance of every pair"""
    n = d.shape[0]
    out = np.zeros((n, n), dtype=np.int32)
    for i0 in range(0, n, 128):
        out[i0:i0 + 128] = _POP[d[i0:i0 + 128, None, :] ^ d[None, :, :]].sum(axis=2)
    return out


def distinctive(d):
    """(row, median) of [N,32] descriptors, N >= 1"""
    n = d.shape[0]
    k = int(0.5 * (n - 1))
    med = np.partition(hamming_matrix(d), k, axis=1)[:, k]
    row = int(np.argmin(med))
    return row, int(med[row])


def _norm(v, dt):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2], dtype=dt)


def _normal_real(pos, centers, ref, s_ref, s_top, dt):
    d = pos.astype(dt)[None, :] - centers.astype(dt)
    nn = _norm(d, dt)
    if (nn == 0).any():
        return None
    normal = np.cumsum(d / nn[:, None], axis=0, dtype=dt)[-1] / dt(len(nn))   # cumsum: the terms in order
    dist = _norm(pos.astype(dt) - ref.astype(dt), dt)
    dmax = dist * dt(s_ref)
    return normal, dmax, dmax / dt(s_top)


def _normal_f32(pos, centers, ref, s_ref, s_top):
    f = np.float32
    p = pos.astype(f)
    d = p[None, :] - centers.astype(f)                                        # :477
    d64 = d.astype(np.float64)
    nn = np.sqrt((d64 * d64).sum(axis=1))                                     # cv::norm: squares summed in double
    if (nn == 0).any():
        return None
    normal = np.zeros(3, dtype=f)
    for v, m in zip(d, nn):
        normal = normal + v * f(1.0 / m)                                      # :479
    pc = (p - ref.astype(f)).astype(np.float64)
    dist = f(np.sqrt((pc * pc).sum()))                                        # :485
    dmax = f(dist * f(s_ref))                                                 # :494
    return normal * f(1.0 / len(nn)), dmax, f(dmax / f(s_top))                # :498, :496


def mappoint_ref(p, mode="float64"):
    """dict of the fields of abi.MapPointResult; normal, dist_max, dist_min in the mode's type"""
    dt = {"float64": np.float64, "longdouble": np.longdouble, "float32": np.float32}[mode]
    n = p.n_pt
    r = dict(best_obs=np.full(n, -1, dtype=np.int32), best_median=np.full(n, -1, dtype=np.int32), n_desc=np.zeros(n, dtype=np.int32),
             desc=np.zeros((n, 32), dtype=np.uint8), normal=np.zeros((n, 3), dtype=dt), dist_max=np.zeros(n, dtype=dt), dist_min=np.zeros(n, dtype=dt),
             desc_state=np.zeros(n, dtype=np.uint8), normal_state=np.zeros(n, dtype=np.uint8))
    for i in range(n):
        b, e = int(p.obs_begin[i]), int(p.obs_begin[i + 1])
        kf = p.obs_kf[b:e]
        if not p.what[i] & abi.MAPPOINT_DESC:
            r["desc_state"][i] = 1
        elif e == b:
            r["desc_state"][i] = 2                                            # :349
        else:
            good = np.nonzero(p.kf_bad[kf] == 0)[0]                           # :360
            r["n_desc"][i] = len(good)
            if len(good) == 0:
                r["desc_state"][i] = 3                                        # :364
            else:
                row, med = distinctive(p.obs_desc[b:e][good])
                r["best_obs"][i], r["best_median"][i], r["desc"][i] = good[row], med, p.obs_desc[b + good[row]]
        if not p.what[i] & abi.MAPPOINT_NORMAL:
            r["normal_state"][i] = 1
        elif e == b:
            r["normal_state"][i] = 2                                          # :467
        else:
            args = (p.pos[i], p.kf_center[kf], p.kf_center[p.ref_kf[i]], p.ref_scale[i], p.ref_top_scale[i])
            v = _normal_f32(*args) if mode == "float32" else _normal_real(*args, dt)
            if v is None:
                r["normal_state"][i] = 3
            else:
                r["normal"][i], r["dist_max"][i], r["dist_min"][i] = v
    r["status"] = 0
    r["n_desc_done"] = int((r["desc_state"] == 0).sum())
    r["n_normal_done"] = int((r["normal_state"] == 0).sum())
    return r


def real_difference(a, b):
    """(largest absolute difference of normal, largest relative difference of the two distances) between two yardstick results"""
    dn = float(np.abs(a["normal"].astype(np.longdouble) - b["normal"].astype(np.longdouble)).max(initial=0))
    dd = 0.0
    for k in ("dist_max", "dist_min"):
        x, y = a[k].astype(np.longdouble), b[k].astype(np.longdouble)
        m = y != 0
        dd = max(dd, float((np.abs(x[m] - y[m]) / np.abs(y[m])).max(initial=0)))
    return dn, dd
