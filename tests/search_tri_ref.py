"""NumPy yardstick of vba_search_triangulation: a literal sequential restatement of ORBmatcher::SearchForTriangulation
(src/ORBmatcher.cpp:760-955, monocular) with CheckDistEpipolarLine (:167-192) and ComputeThreeMaxima (:1800-1841), loop for loop,
with the sequential best update and the lists of rotHist.  The floating-point part runs in the dtype asked for (float32, float64,
longdouble) on the inputs as given; the bin of the rotation histogram is float32 always, as the reference computes it.

search_tri_ref(p, dtype, form) returns a dict: n_matches, n_before_filter, hist [30], ind [3], match12, best_dist, state, pairs,
queries (the node join: (idx1, first, end) into node_feat2 in the order of the walk), margin (the smallest relative distance of
an evaluated floating-point comparison from its threshold, inf without one) and n_fp (how many were evaluated).
form = "seq" is the reference's loop; form = "min" takes, among the candidates that pass every test, the smallest distance, the
last one in list order among equals."""
import numpy as np

HISTO_LENGTH = 30
_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance: the Hamming distance of two 32-byte rows"""
    return int(_POP[np.bitwise_xor(a, b)].sum())


def round_half_away(x):
    """C round() of a non-negative float32: np.round rounds half to even"""
    f = np.floor(x)
    return int(f) + 1 if (x - f) >= np.float32(0.5) else int(f)


def rot_bin(angle1, angle2):
    """:898-903 in float32"""
    rot = np.float32(angle1) - np.float32(angle2)
    if rot < np.float32(0.0):
        rot = np.float32(rot + np.float32(360.0))
    factor = np.float32(1.0) / np.float32(HISTO_LENGTH)
    b = round_half_away(np.float32(rot * factor))
    if b == HISTO_LENGTH:
        b = 0
    assert 0 <= b < HISTO_LENGTH
    return b


def compute_three_maxima(sizes):
    """:1800-1841 on the sizes of the bins"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3 = s
            ind3 = i
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def node_join(p):
    """the `while` of :801-921: [(idx1, first, end)] for every keypoint of keyframe 1 without a map point in a shared node"""
    out = []
    i1 = i2 = 0
    n1, n2 = len(p.node_id1), len(p.node_id2)
    while i1 < n1 and i2 < n2:
        if p.node_id1[i1] == p.node_id2[i2]:
            for k in range(p.node_begin1[i1], p.node_begin1[i1 + 1]):
                idx1 = int(p.node_feat1[k])
                if p.has_mp1[idx1]:
                    continue
                out.append((idx1, int(p.node_begin2[i2]), int(p.node_begin2[i2 + 1])))
            i1 += 1
            i2 += 1
        elif p.node_id1[i1] < p.node_id2[i2]:
            i1 = int(np.searchsorted(p.node_id1, p.node_id2[i2], side="left"))   # lower_bound
        else:
            i2 = int(np.searchsorted(p.node_id2, p.node_id1[i1], side="left"))
    return out


class _Gates:
    """the two floating-point gates of a candidate in one dtype, with the margin bookkeeping"""

    def __init__(self, p, dtype):
        T = self.T = dtype
        self.F = p.F12.astype(T)
        self.ex, self.ey = T(p.epipole[0]), T(p.epipole[1])
        self.r2, self.chi2 = T(p.epipole_r2), T(p.chi2_epi)
        self.uv1, self.uv2 = p.uv1.astype(T), p.uv2.astype(T)
        self.sigma2, self.scale = p.level_sigma2_2.astype(T), p.scale_2.astype(T)
        self.oct2 = p.oct2
        self.margin = np.inf
        self.n_fp = 0

    def _cmp(self, lhs, rhs):
        self.n_fp += 1
        self.margin = min(self.margin, float(abs(lhs - rhs) / abs(rhs)) if rhs != 0 else np.inf)
        return lhs < rhs

    def line(self, idx1):
        F, (u, v) = self.F, self.uv1[idx1]
        a = (u * F[0, 0] + v * F[1, 0]) + F[2, 0]
        b = (u * F[0, 1] + v * F[1, 1]) + F[2, 1]
        c = (u * F[0, 2] + v * F[1, 2]) + F[2, 2]
        return a, b, c

    def near_epipole(self, idx2):   # :871-875
        u, v = self.uv2[idx2]
        dx, dy = self.ex - u, self.ey - v
        return self._cmp(dx * dx + dy * dy, self.r2 * self.scale[self.oct2[idx2]])

    def epipolar_ok(self, l, idx2):   # :167-192
        a, b, c = l
        u, v = self.uv2[idx2]
        num = (a * u + b * v) + c
        den = a * a + b * b
        if den == 0:
            return False
        return self._cmp(num * num / den, self.chi2 * self.sigma2[self.oct2[idx2]])


def search_tri_ref(p, dtype=np.float64, form="seq"):
    n1 = p.n_keys1
    g = _Gates(p, dtype)
    th_low = int(p.th_low)
    queries = node_join(p)
    match12 = np.full(n1, -1, dtype=np.int32)
    best_dist = np.full(n1, 255, dtype=np.uint8)
    state = np.where(p.has_mp1[:n1] != 0, 1, 2).astype(np.uint8)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for idx1, first, end in queries:
        d1 = p.desc1[idx1]
        l = g.line(idx1)
        best, best_idx2 = th_low, -1
        if form == "seq":
            for c in range(first, end):
                idx2 = int(p.node_feat2[c])
                if p.has_mp2[idx2]:
                    continue
                dist = descriptor_distance(d1, p.desc2[idx2])
                if dist > th_low or dist > best:
                    continue
                if g.near_epipole(idx2):
                    continue
                if g.epipolar_ok(l, idx2):
                    best_idx2 = idx2
                    best = dist
        else:
            passing = []
            for c in range(first, end):
                idx2 = int(p.node_feat2[c])
                if p.has_mp2[idx2]:
                    continue
                dist = descriptor_distance(d1, p.desc2[idx2])
                if dist > th_low or g.near_epipole(idx2) or not g.epipolar_ok(l, idx2):
                    continue
                passing.append((dist, c, idx2))
            if passing:
                lo = min(t[0] for t in passing)
                best, _, best_idx2 = [t for t in passing if t[0] == lo][-1]
        if best_idx2 >= 0:
            match12[idx1] = best_idx2
            best_dist[idx1] = best
            state[idx1] = 0
            nmatches += 1
            if p.check_orientation:
                rot_hist[rot_bin(p.angle1[idx1], p.angle2[best_idx2])].append(idx1)
        else:
            state[idx1] = 3
    n_before = nmatches
    hist = np.array([len(b) for b in rot_hist], dtype=np.int32)
    ind = (-1, -1, -1)
    if p.check_orientation:
        ind = compute_three_maxima([len(b) for b in rot_hist])
        for i in range(HISTO_LENGTH):
            if i in ind:
                continue
            for idx1 in rot_hist[i]:
                match12[idx1] = -1
                state[idx1] = 4
                nmatches -= 1
    pairs = np.array([(i, match12[i]) for i in range(n1) if match12[i] >= 0], dtype=np.int32).reshape(-1, 2)
    return dict(n_matches=nmatches, n_before_filter=n_before, hist=hist, ind=np.array(ind, dtype=np.int32), match12=match12,
                best_dist=best_dist, state=state, pairs=pairs, queries=queries, margin=g.margin, n_fp=g.n_fp)


INT_KEYS = ("n_matches", "n_before_filter", "hist", "ind", "match12", "best_dist", "state", "pairs")


def differences(a, b):
    """names of the integer outputs in which two results differ"""
    return [k for k in INT_KEYS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
