"""The yardstick of vba_search_by_bow: both ORBmatcher::SearchByBoW overloads (src/ORBmatcher.cpp:207-350 keyframe -> frame, :609-748
keyframe -> keyframe) restated in NumPy as the SEQUENTIAL loop they are, line by line, on an abi.SearchBowProblem.  Every output is
an integer; float32 appears in the ratio product and in the bin only, both in np.float32 here.

search_bow_fixed_point is a model of what the kernel does instead (rounds of every open query against the claim table of the round
before); tests/test_search_bow_ref.py asserts that it equals the sequential loop.  It is never the yardstick."""
import numpy as np

from mc_slam_amd import abi

HISTO = 30
POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)
INT_MAX = 0x7fffffff


def hamming(a, rows):
    """ORBmatcher::DescriptorDistance of one descriptor against several"""
    return POP[np.bitwise_xor(a[None, :], rows)].sum(axis=1)


def rot_bin(a1, a2):
    """:296-301 / :700-705 in float32 with C round"""
    rot = np.float32(a1) - np.float32(a2)
    if rot < 0.0:
        rot = np.float32(rot + np.float32(360.0))
    t = np.float32(rot * (np.float32(1.0) / np.float32(HISTO)))
    b = int(np.sign(t) * np.floor(np.abs(t) + np.float32(0.5)))
    return 0 if b == HISTO else b


def three_maxima(hist):
    """ComputeThreeMaxima (:1800-1841) over bin counts"""
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(hist):
        s = int(s)
        if s > max1:
            max3, max2, max1 = max2, max1, s
            i3, i2, i1 = i2, i1, i
        elif s > max2:
            max3, max2 = max2, s
            i3, i2 = i2, i
        elif s > max3:
            max3, i3 = s, i
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):
        i2 = i3 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        i3 = -1
    return [i1, i2, i3]


def shared_nodes(p):
    """the `while` of :229-322 / :639-725: the (node index of side 1, node index of side 2) of every shared node, in walk order"""
    i1 = i2 = 0
    out = []
    id1, id2 = p.node_id1, p.node_id2
    while i1 < len(id1) and i2 < len(id2):
        if id1[i1] == id2[i2]:
            out.append((i1, i2))
            i1 += 1
            i2 += 1
        elif id1[i1] < id2[i2]:
            i1 = int(np.searchsorted(id1, id2[i2], side="left"))     # lower_bound
        else:
            i2 = int(np.searchsorted(id2, id1[i1], side="left"))
    return out


def queries(p):
    """the queries in walk order: (idx1, candidates of side 2 in list order, rank among the queries of the node); and the largest
    number of queries in one node"""
    q, most = [], 0
    for a, b in shared_nodes(p):
        cand = p.node_feat2[p.node_begin2[b]:p.node_begin2[b + 1]]
        rank = 0
        for idx1 in p.node_feat1[p.node_begin1[a]:p.node_begin1[a + 1]]:
            if not p.good_mp1[idx1]:
                continue
            q.append((int(idx1), cand, rank))
            rank += 1
        most = max(most, rank)
    return q, most


def _decide(p, dist, cand, usable):
    """the candidate loop (:256-277, :661-687) over the usable candidates, then threshold and ratio test: (best_idx, d1, d2, state)"""
    best1 = best2 = 256
    best = -1
    for c in np.nonzero(usable)[0]:
        d = int(dist[c])
        if d < best1:
            best2, best1, best = best1, d, int(cand[c])
        elif d < best2:
            best2 = d
    passed = best1 < p.th_low if p.kf_kf else best1 <= p.th_low                 # :691 / :280
    if not passed:
        return best, best1, best2, 3
    if not (np.float32(best1) < np.float32(p.nn_ratio) * np.float32(best2)):    # :284, :693, the product in float32
        return best, best1, best2, 4
    return best, best1, best2, 0


def _finish(p, out):
    """what the reference does with the matches: match12 / match21, the bins, the histogram, the three maxima and the drop"""
    n1, n2 = p.n_keys1, p.n_keys2
    out["match12"] = np.full(n1, -1, dtype=np.int32)
    out["match21"] = np.full(n2, -1, dtype=np.int32)
    out["bin"] = np.full(n1, 255, dtype=np.uint8)
    out["hist"] = np.zeros(HISTO, dtype=np.int64)
    out["ind"] = np.array([-1, -1, -1])
    n = 0
    for i in range(n1):
        if out["state"][i] != 0:
            continue
        b = int(out["best_idx"][i])
        out["match12"][i] = b
        out["match21"][b] = i
        n += 1
        if p.check_orientation:
            out["bin"][i] = rot_bin(p.angle1[i], p.angle2[b])
            out["hist"][out["bin"][i]] += 1
    out["n_before_filter"] = n
    if p.check_orientation:
        out["ind"] = np.array(three_maxima(out["hist"]))
        for i in range(n1):
            b = out["bin"][i]
            if b == 255 or b in out["ind"]:
                continue
            out["match21"][out["match12"][i]] = -2
            out["match12"][i] = -1
            out["state"][i] = 5
            n -= 1
    out["n_matches"] = n
    return out


def _blank(p):
    n1 = p.n_keys1
    state = np.where(np.asarray(p.good_mp1[:n1]) != 0, 2, 1).astype(np.uint8)
    return dict(state=state, best_idx=np.full(n1, -1, dtype=np.int32), best_dist=np.full(n1, 256, dtype=np.uint16),
                best_dist2=np.full(n1, 256, dtype=np.uint16))


def search_bow_ref(p):
    """the sequential loop"""
    out = _blank(p)
    taken = np.zeros(p.n_keys2, dtype=bool)
    good2 = np.ones(p.n_keys2, dtype=bool) if not p.kf_kf else np.asarray(p.good_mp2) != 0
    qs, most = queries(p)
    for idx1, cand, _ in qs:
        dist = hamming(p.desc1[idx1], p.desc2[cand]) if len(cand) else np.zeros(0, dtype=np.int64)
        best, d1, d2, st = _decide(p, dist, cand, ~taken[cand] & good2[cand])
        out["best_idx"][idx1], out["best_dist"][idx1], out["best_dist2"][idx1], out["state"][idx1] = best, d1, d2, st
        if st == 0:
            taken[best] = True                                                   # :287, :696
    out["n_q"], out["max_node_q"] = len(qs), most
    return _finish(p, out)


def search_bow_fixed_point(p, node_local=True):
    """the kernel's conflict pass: claim[k] = the smallest walk index of a query whose current result is a match on k (-1: statically
    no candidate); query q treats k as taken iff claim[k] < q; rounds until no claim changes.  With node_local a query of rank r is
    skipped from round r + 1 on.  Returns the outputs and `rounds`"""
    out = _blank(p)
    good2 = np.ones(p.n_keys2, dtype=bool) if not p.kf_kf else np.asarray(p.good_mp2) != 0
    static = np.where(good2, INT_MAX, -1).astype(np.int64)
    claim = static.copy()
    qs, most = queries(p)
    dists = [hamming(p.desc1[i], p.desc2[c]) if len(c) else np.zeros(0, dtype=np.int64) for i, c, _ in qs]
    prev = [-1] * len(qs)
    rounds = 0
    for rnd in range((most if node_local else len(qs)) + 1):
        changed = False
        for q, (idx1, cand, rank) in enumerate(qs):
            if (rank if node_local else q) < rnd:
                continue
            best, d1, d2, st = _decide(p, dists[q], cand, claim[cand] >= q)
            out["best_idx"][idx1], out["best_dist"][idx1], out["best_dist2"][idx1], out["state"][idx1] = best, d1, d2, st
            now = best if st == 0 else -1
            changed |= now != prev[q]
            prev[q] = now
        rounds = rnd + 1
        if not changed:
            break
        claim = static.copy()
        for q, c in enumerate(prev):
            if c >= 0:
                claim[c] = min(claim[c], q)
    else:
        raise AssertionError("the pass did not stop by itself")
    out["n_q"], out["max_node_q"], out["rounds"] = len(qs), most, rounds
    return _finish(p, out)
