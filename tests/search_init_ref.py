"""NumPy yardstick of vba_search_for_initialization: a literal SEQUENTIAL restatement, loop for loop, of
ORBmatcher::SearchForInitialization (src/ORBmatcher.cpp:477-595) over Frame::GetFeaturesInArea(x, y, windowSize, 0, 0)
(src/Frame.cpp:562-620).  The keypoints of frame 1 run one after the other against vMatchedDistance and vnMatches21 as each match
mutates them, exactly as the reference does; the fixed-point iteration of the kernel is NOT used here (conflict_pass below is a
prototype of it, for tests/test_search_init_ref.py).  The area runs in the dtype asked for (float64, longdouble) on the inputs
widened; the ratio product (:536) and the bin (:550-555) are float32 in every dtype.

search_init_ref(p, dtype, ignore_claims=False) returns a dict: n_matches, n_before_filter, n_stolen, hist, ind, match12, best_idx,
best_dist, best_dist2, bin, state, prev_matched (float32), match21, matched_dist, n_cand (the candidates of the area per keypoint of
frame 1), and the margin bookkeeping of tests/fuse_ref.py (margin, n_fp: the comparisons; margin_r, n_round: the floor and ceil
arguments).  ignore_claims=True answers every query as if vMatchedDistance stayed at INT_MAX: what an independent-query kernel
would give in front of the apply loop."""
from types import SimpleNamespace

import numpy as np

from fuse_ref import _Fp, descriptor_distance, features_in_area
from search_proj_ref import HISTO, rot_bin, three_maxima   # noqa: F401

INT_MAX = 2 ** 31 - 1
INT_KEYS = ("n_matches", "n_before_filter", "n_stolen", "hist", "ind", "match12", "best_idx", "best_dist", "best_dist2", "bin", "state", "match21",
            "matched_dist")


def frame2(p):
    """frame 2 under the field names features_in_area reads"""
    return SimpleNamespace(bounds=p.bounds, grid_inv_w=p.grid_inv_w, grid_inv_h=p.grid_inv_h, grid_cols=p.grid_cols, grid_rows=p.grid_rows,
                           cell_begin=p.cell_begin, cell_feat=p.cell_feat, oct=p.oct2)


def _areas(p, T, fp):
    """per keypoint of frame 1: None above level 0 (:495), else the candidates of :498 in walk order"""
    f2, uvT, r = frame2(p), p.uv2.astype(T), T(p.window_size)
    out = []
    for i in range(p.n_keys1):
        if p.oct1[i] > 0:
            out.append(None)
            continue
        x, y = T(p.prev_matched[i, 0]), T(p.prev_matched[i, 1])
        out.append(features_in_area(f2, fp, T, uvT, x, y, r, 0, 0))
    return out


def _query(p, i, cand, matched_dist):
    """:501-536 for keypoint i of frame 1: (state, bestIdx2, bestDist, bestDist2) with INT_MAX for none; matched_dist(k) is what
    the query reads as vMatchedDistance[k]"""
    if not cand:                                                                     # :501
        return 2, -1, INT_MAX, INT_MAX
    bd = bd2 = INT_MAX
    bi = -1
    for k in cand:
        d = descriptor_distance(p.desc1[i], p.desc2[k])
        if matched_dist(k) <= d:                                                     # :518
            continue
        if d < bd:                                                                   # :521-530
            bd2, bd, bi = bd, d, k
        elif d < bd2:
            bd2 = d
    if not bd <= int(p.th_low):                                                      # :534
        return 3, bi, bd, bd2
    if not np.float32(bd) < np.float32(bd2) * np.float32(p.nn_ratio):                # :536
        return 4, bi, bd, bd2
    return 0, bi, bd, bd2


def _finish(p, fp, cands, state, best_idx, bd, bd2, extra=None):
    """the apply loop in index order (:538-558), ComputeThreeMaxima, the drop (:564-587) and the vbPrevMatched update (:590-592)"""
    n1, n2 = p.n_keys1, p.n_keys2
    ori = bool(p.check_orientation)
    match12 = np.full(n1, -1, dtype=np.int32)
    match21 = np.full(n2, -1, dtype=np.int32)
    mdist = np.full(n2, INT_MAX, dtype=np.int64)
    bins = np.full(n1, 255, dtype=np.uint8)
    rot_hist = [[] for _ in range(HISTO)]
    nmatches = stolen = 0
    for i in range(n1):
        if state[i] != 0:
            continue
        k = int(best_idx[i])
        if match21[k] >= 0:                                                          # :538-542
            match12[match21[k]] = -1
            state[match21[k]] = 5
            nmatches -= 1
            stolen += 1
        match12[i], match21[k], mdist[k] = k, i, bd[i]
        nmatches += 1
        if ori:
            b = rot_bin(p.angle1[i], p.angle2[k])
            bins[i] = b
            rot_hist[b].append(i)
    n_before = nmatches
    hist = np.array([len(h) for h in rot_hist], dtype=np.int32)
    ind = (-1, -1, -1)
    if ori:
        ind = three_maxima(hist)
        for b in range(HISTO):
            if b not in ind:
                for i in rot_hist[b]:
                    if match12[i] >= 0:                                              # :579-582
                        match12[i] = -1
                        state[i] = 6
                        nmatches -= 1
    prev = p.prev_matched.copy()
    for i in range(n1):
        if match12[i] >= 0:
            prev[i] = p.uv2[match12[i]].astype(np.float32)                           # :590-592
    out = dict(n_matches=nmatches, n_before_filter=n_before, n_stolen=stolen, hist=hist, ind=np.array(ind, dtype=np.int32), match12=match12,
               best_idx=best_idx, best_dist=np.minimum(bd, 256).astype(np.uint16), best_dist2=np.minimum(bd2, 256).astype(np.uint16), bin=bins,
               state=state, prev_matched=prev, match21=match21, matched_dist=np.minimum(mdist, 256).astype(np.uint16),
               n_cand=np.array([0 if c is None else len(c) for c in cands], dtype=np.int64),
               margin=fp.margin, n_fp=fp.n_fp, margin_r=fp.margin_r, n_round=fp.n_round)
    out.update(extra or {})
    return out


def search_init_ref(p, dtype=np.float64, ignore_claims=False):
    T = np.dtype(dtype).type
    fp = _Fp()
    n1, n2 = p.n_keys1, p.n_keys2
    best_idx = np.full(n1, -1, dtype=np.int32)
    bd = np.full(n1, INT_MAX, dtype=np.int64)
    bd2 = np.full(n1, INT_MAX, dtype=np.int64)
    state = np.ones(n1, dtype=np.uint8)
    mdist = np.full(n2, INT_MAX, dtype=np.int64)
    with np.errstate(all="ignore"):
        cands = _areas(p, T, fp)
    for i in range(n1):
        if cands[i] is None:
            continue
        state[i], best_idx[i], bd[i], bd2[i] = _query(p, i, cands[i], lambda k: mdist[k])
        if state[i] == 0 and not ignore_claims:
            mdist[best_idx[i]] = bd[i]                                               # :545
    return _finish(p, fp, cands, state, best_idx, bd, bd2)


def conflict_pass(p, dtype=np.float64):
    """a prototype of the kernel's pass over the level-0 keypoints of frame 1 as the query list: rounds in which every open query
    q >= round walks against the claimer lists of the round before (per keypoint of frame 2 the queries whose current result takes it,
    with their distances; q reads the minimum over the entries < q), the lists are rebuilt, until a round changes no claim (accepted,
    keypoint, distance).  Returns the result dict with `rounds`"""
    T = np.dtype(dtype).type
    fp = _Fp()
    n1 = p.n_keys1
    best_idx = np.full(n1, -1, dtype=np.int32)
    bd = np.full(n1, INT_MAX, dtype=np.int64)
    bd2 = np.full(n1, INT_MAX, dtype=np.int64)
    state = np.ones(n1, dtype=np.uint8)
    with np.errstate(all="ignore"):
        cands = _areas(p, T, fp)
    qs = [i for i in range(n1) if cands[i] is not None]
    nq = len(qs)
    claim = [None] * nq                       # (keypoint, distance) of an accepted query
    lists = {}
    rounds = 0
    for rnd in range(nq + 1):
        changed = False
        for q in range(rnd, nq):
            i = qs[q]
            seen = lambda k: min([d for pq, d in lists.get(k, ()) if pq < q], default=INT_MAX)
            state[i], best_idx[i], bd[i], bd2[i] = _query(p, i, cands[i], seen)
            now = (int(best_idx[i]), int(bd[i])) if state[i] == 0 else None
            changed |= now != claim[q]
            claim[q] = now
        rounds = rnd + 1
        if not changed:
            break
        lists = {}
        for q in reversed(range(nq)):         # any push order
            if claim[q] is not None:
                lists.setdefault(claim[q][0], []).append((q, claim[q][1]))
    return _finish(p, fp, cands, state, best_idx, bd, bd2, dict(rounds=rounds))


def differences(a, b):
    """names of the integer outputs in which two results differ"""
    return [k for k in INT_KEYS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
