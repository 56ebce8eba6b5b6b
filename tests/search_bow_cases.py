"""The cases of the vba_search_by_bow tests: hand-made pairs and synthetic ones (mc_slam_amd.synth.search_bow_scene), the smallest
shapes at which the kernel can still go wrong.  cases() builds every pair once; ref(name) is the yardstick's answer
(tests/search_bow_ref.py, the sequential loop), computed once and shared by the tests (treat both as read-only).

The hand-made pairs live on a line: the descriptor of position x has its first x bits set, so the Hamming distance of two keypoints
is |x1 - x2|.  A side is a list of (node id, x, good map point) in keypoint order; a node lists its keypoints in that order."""
import functools

import numpy as np

from mc_slam_amd import abi, synth
import search_bow_ref as ref_mod

KF_FRAME, KF_KF = abi.SEARCH_BOW_KF_FRAME, abi.SEARCH_BOW_KF_KF
CHAIN = 40


def line_desc(x):
    bits = np.zeros(256, dtype=np.uint8)
    bits[:x] = 1
    return np.packbits(bits)


def pair(mode, side1, side2, angle1=None, angle2=None, **kw):
    """a hand-made pair from two lists of (node id, x, good map point)"""
    def side(s):
        fv = {}
        for i, (node, _, _) in enumerate(s):
            fv.setdefault(node, []).append(i)
        desc = np.array([line_desc(x) for _, x, _ in s], dtype=np.uint8).reshape(-1, 32)
        return desc, np.array([g for _, _, g in s], dtype=np.uint8), abi.feat_vec_csr(fv)

    d1, g1, (id1, b1, f1) = side(side1)
    d2, g2, (id2, b2, f2) = side(side2)
    ori = angle1 is not None
    return abi.SearchBowProblem(mode=mode, desc1=d1, desc2=d2, good_mp1=g1, good_mp2=g2 if mode == KF_KF else None, node_id1=id1, node_begin1=b1,
                                node_feat1=f1, node_id2=id2, node_begin2=b2, node_feat2=f2, check_orientation=ori,
                                angle1=np.asarray(angle1, dtype=np.float32) if ori else None, angle2=np.asarray(angle2, dtype=np.float32) if ori else None,
                                **kw)


# ---- hand-made pairs with hand-worked expectations: keypoint of side 1 -> (state, best_idx, best_dist, best_dist2)
def _micro():
    """one node, one query, one candidate: 3 < 0.75f * 256"""
    return pair(KF_FRAME, [(5, 0, 1)], [(5, 3, 1)]), {0: (0, 0, 3, 256)}


def _states():
    """one keypoint per state but 5.  Node 5 is shared; node 7 is on side 1 only.  Keypoint 0 matches candidate 0 (distance 2, second
    40); keypoint 1 has no good map point (state 1, although its node is shared); keypoint 2 sits in node 7 (state 2); keypoint 3
    (x = 200) finds candidate 0 taken and is 160 and 78 away from the others: 78 > 50 (state 3); keypoint 4 (x = 80) has 40 and 42 to
    choose from: 40 < 0.75f * 42 = 31.5 fails (state 4); keypoint 5 has no good map point AND no shared node: 1 wins over 2"""
    s1 = [(5, 0, 1), (5, 0, 0), (7, 0, 1), (5, 200, 1), (5, 80, 1), (7, 0, 0)]
    s2 = [(5, 2, 1), (5, 40, 1), (5, 122, 1)]
    return pair(KF_FRAME, s1, s2), {0: (0, 0, 2, 40), 1: (1, -1, 256, 256), 2: (2, -1, 256, 256), 3: (3, 2, 78, 160), 4: (4, 1, 40, 42),
                                     5: (1, -1, 256, 256)}


def _ratio_flip_fail():
    """keypoint 1 would match candidate 0 (distances 1, 9, 11); keypoint 0 takes it first, and 9 < 0.75f * 11 = 8.25 fails"""
    return pair(KF_FRAME, [(5, 0, 1), (5, 1, 1)], [(5, 2, 1), (5, 10, 1), (5, 12, 1)]), {0: (0, 0, 2, 10), 1: (4, 1, 9, 11)}


def _ratio_flip_pass():
    """keypoint 1 alone fails the ratio test (9 against 10: 9 < 7.5 fails); keypoint 0 takes the candidate 10 away and it passes with
    9 against 20"""
    return pair(KF_FRAME, [(5, 10, 1), (5, 20, 1)], [(5, 10, 1), (5, 11, 1), (5, 40, 1)]), {0: (0, 0, 0, 1), 1: (0, 1, 9, 20)}


def _all_taken():
    """three queries, two candidates: the third finds every candidate taken and leaves with state 3, -1 and 256"""
    return pair(KF_FRAME, [(5, 0, 1), (5, 0, 1), (5, 0, 1)], [(5, 1, 1), (5, 2, 1)]), {0: (0, 0, 1, 2), 1: (0, 1, 2, 256), 2: (3, -1, 256, 256)}


def _tie_fails():
    """equal best distances: the first in list order is the best, the equal one is bestDist2, and 3 < 0.75f * 3 fails"""
    return pair(KF_FRAME, [(5, 5, 1)], [(5, 30, 1), (5, 2, 1), (5, 8, 1)]), {0: (4, 1, 3, 3)}


def _tie_first_wins():
    """the same with nn_ratio = 1.5: 3 < 4.5 passes and the FIRST of the equal candidates is the match"""
    return pair(KF_FRAME, [(5, 5, 1)], [(5, 30, 1), (5, 8, 1), (5, 2, 1)], nn_ratio=1.5), {0: (0, 1, 3, 3)}


def _th_equal(mode):
    """bestDist1 == th_low: <= matches in KF_FRAME mode (:280), < does not in KF_KF mode (:691)"""
    return pair(mode, [(5, 0, 1)], [(5, 50, 1)]), {0: (0 if mode == KF_FRAME else 3, 0, 50, 256)}


def _th_zero(mode):
    """th_low = 0: only an exact descriptor passes <=, nothing passes <"""
    return pair(mode, [(5, 7, 1), (5, 9, 1)], [(5, 7, 1), (5, 10, 1)], th_low=0), {0: (0 if mode == KF_FRAME else 3, 0, 0, 3),
                                                                                   1: (3, 1, 1, 2) if mode == KF_KF else (3, 1, 1, 256)}


def _th_255(mode):
    """th_low = 255 with nn_ratio = 1 (255 < 256): 255 <= 255 matches, 255 < 255 does not; 254 matches in both modes"""
    return pair(mode, [(5, 0, 1), (6, 0, 1)], [(5, 255, 1), (6, 254, 1)], th_low=255, nn_ratio=1.0), {0: (0 if mode == KF_FRAME else 3, 0, 255, 256), 1: (0, 1, 254, 256)}


def _bad_mp2():
    """KF_KF: candidate 0 would be the best of keypoint 0 but has no good map point; candidate 1 (distance 10, second 30) is.  In
    KF_FRAME mode (good_mp2 not read) candidate 0 is the match"""
    s1, s2 = [(5, 0, 1)], [(5, 1, 0), (5, 10, 1), (5, 30, 1)]
    return pair(KF_KF, s1, s2), {0: (0, 1, 10, 30)}, pair(KF_FRAME, s1, s2), {0: (0, 0, 1, 10)}


def _float32_product():
    """nn_ratio = 0.6f = 0.60000002384: 0.6f * 10 is 6.0000002384 exactly and 6.0 in float32 (a tie, rounded to even), so
    (float)6 < 0.6f * (float)10 is false as the reference computes it and true in float64.  The match is refused (state 4)"""
    return pair(KF_FRAME, [(5, 0, 1)], [(5, 6, 1), (5, 10, 1)], nn_ratio=0.6), {0: (4, 0, 6, 10)}


def float32_flips(nn_ratio):
    """every (bestDist1, bestDist2) in 0 .. 256 at which the float32 product and the float64 product of the float32 ratio decide
    the ratio test differently"""
    r32 = np.float32(nn_ratio)
    b1 = np.arange(257)[:, None]
    b2 = np.arange(257)[None, :]
    f32 = b1.astype(np.float32) < r32 * b2.astype(np.float32)
    f64 = b1.astype(np.float64) < np.float64(r32) * b2.astype(np.float64)
    return [(int(a), int(b)) for a, b in zip(*np.nonzero(f32 != f64))]


def _orientation_drop():
    """six matches in six nodes with the bins 0, 0, 0, 1, 2 and 3: ComputeThreeMaxima keeps 0, 1 and 2, the match of keypoint 5 is
    dropped (state 5, match21 = -2)"""
    s1 = [(10 + i, 0, 1) for i in range(6)]
    s2 = [(10 + i, 1, 1) for i in range(6)]
    return (pair(KF_KF, s1, s2, angle1=[10, 11, 12, 40, 70, 100], angle2=[5, 5, 5, 5, 5, 5]),
            {i: (0 if i < 5 else 5, i, 1, 256) for i in range(6)})


def _one_sided_nodes():
    """nodes on one side only, so that both lower_bound branches run, also over several nodes at once and at both ends"""
    s1 = [(1, 0, 1), (5, 0, 1), (6, 0, 1), (7, 0, 1), (9, 0, 1), (20, 0, 1)]
    s2 = [(2, 1, 1), (3, 1, 1), (5, 1, 1), (9, 2, 1), (12, 1, 1), (13, 1, 1)]
    e = {i: (2, -1, 256, 256) for i in range(6)}
    e[1] = (0, 2, 1, 256)
    e[4] = (0, 3, 2, 256)
    return pair(KF_FRAME, s1, s2), e


def _chain(n_nodes):
    """CHAIN queries with one descriptor, spread over n_nodes nodes; every node holds as many candidates at the distances 1, 2, ...
    With nn_ratio = 1 the k-th query of a node takes the k-th candidate, after k rounds of the pass"""
    per = CHAIN // n_nodes
    s1 = [(5 + 2 * (i // per), 0, 1) for i in range(CHAIN)]
    s2 = [(5 + 2 * (i // per), 1 + i % per, 1) for i in range(CHAIN)]
    return pair(KF_FRAME, s1, s2, nn_ratio=1.0)


def _random_pair(seed, mode, sizes1, sizes2, twins=0.3, flip=10):
    """all keypoints of side 1 are queries: node k holds sizes1[k] of them and sizes2[k] candidates; a share `twins` of the
    candidates is a query's descriptor with up to `flip` bits flipped, several of them for the same query"""
    r = np.random.default_rng(seed)
    n1, n2 = sum(sizes1), sum(sizes2)
    node1 = np.repeat(np.arange(len(sizes1)), sizes1)
    node2 = np.repeat(np.arange(len(sizes2)), sizes2)
    d1 = r.integers(0, 256, (n1, 32), dtype=np.uint8)
    d2 = r.integers(0, 256, (n2, 32), dtype=np.uint8)
    for j in range(n2):
        src = np.nonzero(node1 == node2[j])[0]
        if len(src) and r.random() < twins:
            bits = np.unpackbits(d1[src[int(r.integers(len(src)))]])
            bits[r.permutation(256)[:int(r.integers(0, flip + 1))]] ^= 1
            d2[j] = np.packbits(bits)
    p1, p2 = r.permutation(n1), r.permutation(n2)
    fv1, fv2 = {}, {}
    for new in range(n1):
        fv1.setdefault(int(node1[p1[new]]), []).append(new)
    for new in range(n2):
        fv2.setdefault(int(node2[p2[new]]), []).append(new)
    id1, b1, f1 = abi.feat_vec_csr(fv1)
    id2, b2, f2 = abi.feat_vec_csr(fv2)
    a1 = r.uniform(0, 359, n1).astype(np.float32)
    a2 = r.uniform(0, 359, n2).astype(np.float32)
    return abi.SearchBowProblem(mode=mode, desc1=d1[p1], desc2=d2[p2], good_mp1=np.ones(n1, dtype=np.uint8),
                                good_mp2=(r.random(n2) < 0.85).astype(np.uint8) if mode == KF_KF else None, node_id1=id1, node_begin1=b1, node_feat1=f1,
                                node_id2=id2, node_begin2=b2, node_feat2=f2, angle1=a1, angle2=a2)


HAND = {}


def _hand():
    if not HAND:
        HAND.update(micro=_micro(), states=_states(), ratio_flip_fail=_ratio_flip_fail(), ratio_flip_pass=_ratio_flip_pass(), all_taken=_all_taken(),
                    tie_fails=_tie_fails(), tie_first_wins=_tie_first_wins(), float32_product=_float32_product(), orientation_drop=_orientation_drop(),
                    one_sided_nodes=_one_sided_nodes(), bad_mp2_kf=_bad_mp2()[:2], bad_mp2_frame=_bad_mp2()[2:])
        for mode, tag in ((KF_FRAME, "frame"), (KF_KF, "kf")):
            HAND["th_equal_" + tag] = _th_equal(mode)
            HAND["th_zero_" + tag] = _th_zero(mode)
            HAND["th_255_" + tag] = _th_255(mode)
    return HAND


@functools.lru_cache(maxsize=None)
def cases():
    c = {k: v[0] for k, v in _hand().items()}
    c["chain_40"] = _chain(1)
    c["chain_8x5"] = _chain(8)
    c["empty_keys1"] = synth.search_bow_scene(21, KF_FRAME, n_keys1=0, n_keys2=40, n_nodes=5)
    c["empty_keys2"] = synth.search_bow_scene(22, KF_KF, n_keys1=40, n_keys2=0, n_nodes=5)
    c["no_shared_node"] = pair(KF_KF, [(1, 0, 1), (3, 0, 1)], [(2, 0, 1), (4, 0, 1)])
    # the lane stride wraps: 256, 257 and 513 queries; one node with more than 64 and one with more than 256 queries
    c["queries_256"] = _random_pair(256, KF_FRAME, [16] * 16, [16] * 16)
    c["queries_257"] = _random_pair(257, KF_KF, [16] * 15 + [17], [12] * 16)
    c["queries_513"] = _random_pair(513, KF_FRAME, [27] * 19, [20] * 19)
    c["node_70"] = _random_pair(70, KF_KF, [70, 9], [75, 9], twins=0.5)
    c["node_300"] = _random_pair(300, KF_FRAME, [5, 300], [5, 280], twins=0.5)
    for mode, tag in ((KF_FRAME, "frame"), (KF_KF, "kf")):
        c["synth_small_" + tag] = synth.search_bow_scene(31, mode, n_keys1=200, n_keys2=180, n_nodes=12)
        c["realistic_" + tag] = synth.search_bow_scene(41, mode, n_keys1=1500, n_keys2=1500, n_nodes=100)
        c["crowd_" + tag] = synth.search_bow_scene(51, mode, n_keys1=300, n_keys2=120, n_nodes=6, near_dup=0.5, mp1=1.0)
    c["no_orientation"] = synth.search_bow_scene(31, KF_KF, n_keys1=200, n_keys2=180, n_nodes=12, check_orientation=False)
    # the largest side 2 the entry point takes: the claim table fills the dynamic LDS
    c["max_keys"] = synth.search_bow_scene(61, KF_FRAME, n_keys1=96, n_keys2=abi.SEARCH_BOW_MAX_KEYS, n_nodes=40, twins=1.0)
    return c


def expect(name):
    return _hand()[name][1]


@functools.lru_cache(maxsize=None)
def ref(name):
    return ref_mod.search_bow_ref(cases()[name])


INTS = ("state", "match12", "best_idx", "best_dist", "best_dist2", "bin", "match21", "hist", "ind")


def check_against(what, got, want):
    """a library result against a yardstick result: every output equal for every keypoint of both sides, nothing excused; and
    1 <= rounds <= (largest number of queries in one node) + 1"""
    assert got.status == 0, what
    for k in INTS:
        g, w = np.asarray(getattr(got, k)), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (what, k, bad[:8], g[bad[:8]], w[bad[:8]])
    assert (got.n_matches, got.n_before_filter) == (want["n_matches"], want["n_before_filter"]), what
    assert 1 <= got.rounds <= want["max_node_q"] + 1, (what, got.rounds, want["max_node_q"])
