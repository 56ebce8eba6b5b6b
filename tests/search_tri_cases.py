"""The cases of the vba_search_triangulation tests: synthetic keyframe pairs (mc_slam_amd.synth.synth_match_pair) and hand-made
ones, at most a few hundred keypoints each.  cases() builds every problem once; ref(name, dtype, form) is the yardstick's answer,
computed once and shared by the tests (treat both as read-only).

The hand-made pairs use F12 = [[0 0 0] [0 0 -1] [0 1 0]]: the epipolar line of (u1, v1) is v2 = v1, num^2 / den = (v2 - v1)^2
against 3.84 * sigma2, so a candidate one pixel off passes and one ten pixels off fails, both far from the threshold."""
import functools

import numpy as np

from mc_slam_amd import abi, synth
import search_tri_ref as ref_mod

F_RECT = np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])
FAR = np.array([1.0e6, 0.0])          # an epipole no keypoint is near


def base_desc(seed):
    return np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8)


def flip(d, k, start=0):
    """d with the k bits start .. start + k - 1 flipped: Hamming distance k from d"""
    b = np.unpackbits(d)
    b[start:start + k] ^= 1
    return np.packbits(b)


def key(desc, u, v, node, angle=0.0, oct=0, mp=0):
    return dict(desc=desc, u=u, v=v, node=node, angle=angle, oct=oct, mp=mp)


def craft(k1, k2, F12=F_RECT, epipole=FAR, n_levels=8, **kw):
    """a pair from two lists of key(): a node lists its keypoints in list order, except that the nodes named in kw['reverse2']
    list those of keyframe 2 backwards (node_feat_2 not ascending)"""
    reverse2 = kw.pop("reverse2", ())
    scale, sigma2 = synth.level_tables(n_levels)

    def side(ks, rev):
        fv = {}
        for i, k in enumerate(ks):
            if k["node"] is not None:
                fv.setdefault(k["node"], []).append(i)
        for n in rev:
            fv[n] = fv[n][::-1]
        a = lambda name, dt: np.array([k[name] for k in ks], dtype=dt)
        return (a("desc", np.uint8).reshape(-1, 32), a("mp", np.uint8), np.stack([a("u", np.float64), a("v", np.float64)], axis=1).reshape(-1, 2),
                a("angle", np.float32), a("oct", np.uint8)) + abi.feat_vec_csr(fv)

    d1, m1, uv1, a1, _, id1, b1, f1 = side(k1, ())
    d2, m2, uv2, a2, o2, id2, b2, f2 = side(k2, reverse2)
    return abi.SearchTriProblem(desc1=d1, desc2=d2, has_mp1=m1, has_mp2=m2, node_id1=id1, node_begin1=b1, node_feat1=f1, node_id2=id2,
                                node_begin2=b2, node_feat2=f2, uv1=uv1, uv2=uv2, angle1=a1, angle2=a2, oct2=o2, level_sigma2_2=sigma2,
                                scale_2=scale, F12=F12, epipole=epipole, **kw)


def _micro():
    """one pair, one scenario per node; keypoint indices are those of the lists below.  expect: idx1 -> (idx2, state)"""
    k1, k2, expect = [], [], {}
    D = [base_desc(100 + i) for i in range(12)]

    def q(*a, **k):
        k1.append(key(*a, **k)); return len(k1) - 1

    def c(*a, **k):
        k2.append(key(*a, **k)); return len(k2) - 1

    # node 10: duplicated descriptors in keyframe 2: equal distances, the last passing one in LIST order wins; the node lists
    # keyframe 2 backwards, so list order is c3 c2 c1 c0: c3 fails the epipolar test, c2 c1 c0 pass, c0 is last
    i = q(D[0], 100, 50, 10)
    c0 = c(flip(D[0], 7), 300, 50, 10); c(flip(D[0], 7), 310, 51, 10); c(flip(D[0], 7), 320, 50, 10); c(flip(D[0], 7), 330, 60, 10)
    expect[i] = (c0, 0, 7)
    # node 11: an earlier candidate passes with distance 10, a later one with distance 5 fails the epipolar test, a last one with
    # distance 10 passes again and replaces the first (dist > bestDist is false for an equal distance)
    i = q(D[1], 100, 80, 11)
    c(flip(D[1], 10), 300, 80, 11); c(flip(D[1], 5), 300, 95, 11); c2 = c(flip(D[1], 10, 20), 305, 81, 11)
    expect[i] = (c2, 0, 10)
    # the same without the last one: the first stays
    i = q(D[2], 100, 120, 12)
    c0 = c(flip(D[2], 10), 300, 120, 12); c(flip(D[2], 5), 300, 135, 12)
    expect[i] = (c0, 0, 10)
    # node 13: distances of exactly 50 and 51 (th_low = 50)
    i = q(D[3], 100, 160, 13)
    c(flip(D[3], 51), 300, 160, 13); c1 = c(flip(D[3], 50, 100), 300, 161, 13)
    expect[i] = (c1, 0, 50)
    i = q(D[4], 100, 200, 14)
    c(flip(D[4], 51), 300, 200, 14)
    expect[i] = (-1, 3, 255)
    # node 15: map points on either side: the query with one leaves with state 1, a perfect candidate with one is passed over
    i = q(D[5], 100, 240, 15, mp=1)
    expect[i] = (-1, 1, 255)
    i = q(D[5], 101, 240, 15)
    c(D[5], 300, 240, 15, mp=1); c1 = c(flip(D[5], 20), 301, 240, 15)
    expect[i] = (c1, 0, 20)
    # node 16 (with the epipole at (600, 300)): 3 pixels off at octave 0 is inside the radius, 11 pixels off at octave 3 too
    # (121 < 100 * 1.728), 11 pixels off at octave 0 is outside (121 > 100)
    i = q(D[6], 100, 300, 16)
    c(D[6], 603, 300, 16); c(flip(D[6], 1), 611, 300, 16, oct=3); c2 = c(flip(D[6], 2), 589, 300, 16)
    expect[i] = (c2, 0, 2)
    # node 17: two queries that legitimately return the same idx2 (vbMatched2 is never set)
    i = q(D[7], 100, 340, 17); j = q(flip(D[7], 3), 110, 341, 17)
    c0 = c(flip(D[7], 1, 50), 300, 340, 17)
    expect[i] = (c0, 0, 1); expect[j] = (c0, 0, 4)
    # a keypoint in a node keyframe 2 does not have, one in no node at all, one with a map point in no node
    expect[q(D[8], 100, 380, 18)] = (-1, 2, 255)
    expect[q(D[8], 100, 380, None)] = (-1, 2, 255)
    expect[q(D[8], 100, 380, None, mp=1)] = (-1, 1, 255)
    c(D[8], 300, 380, 19)
    return craft(k1, k2, epipole=np.array([600.0, 300.0]), check_orientation=False, reverse2=(10,)), expect


def _jumps():
    """nodes present on one side only at the start, in the middle and at the end of the id lists: shared are 5, 20, 31"""
    ids1, ids2 = [1, 2, 5, 6, 7, 20, 30, 31, 50, 51], [0, 5, 9, 10, 20, 25, 31, 40]
    D = {n: base_desc(200 + n) for n in set(ids1) | set(ids2)}
    k1 = [key(flip(D[n], j), 100 + j, 10.0 * n, n) for n in ids1 for j in range(2)]
    k2 = [key(flip(D[n], 2 + j, 40), 300 + j, 10.0 * n, n) for n in ids2 for j in range(3)]
    return craft(k1, k2, check_orientation=False)


def _den0():
    """F12 = [[0 0 0] [0 1 -50] [0 -50 2500]]: a = 0, b = v1 - 50, c = -50 (v1 - 50), so den == 0 exactly for a query with v1 = 50
    and num^2 / den = (v2 - 50)^2 for the others"""
    F = np.array([[0.0, 0, 0], [0, 1, -50], [0, -50, 2500]])
    D = base_desc(300)
    k1 = [key(D, 100, 50, 1), key(flip(D, 2), 100, 70, 1), key(flip(D, 3), 120, 20, 1)]
    k2 = [key(flip(D, 1, 60), 300, 50, 1), key(flip(D, 1, 90), 300, 51, 1), key(D, 300, 70, 1)]
    return craft(k1, k2, F12=F, check_orientation=False)


def half_rot(k):
    """a float32 rot with rot * (1.0f / 30) == k + 0.5 exactly in float32"""
    factor = np.float32(1.0) / np.float32(30)
    for toward in (np.float32(0.0), np.float32(400.0)):
        x = np.float32(30.0 * (k + 0.5))
        for _ in range(8):
            if np.float32(x * factor) == np.float32(k + 0.5):
                return x
            x = np.nextafter(x, toward)
    raise AssertionError("no float32 rot lands on %g" % (k + 0.5))


def _ori(rots, check=True):
    """one query per entry of rots, each alone in its node with one perfect candidate; rot = angle1 - angle2 in float32: a
    non-negative rot is (rot, 0), a negative one (0, -rot)"""
    k1, k2 = [], []
    for n, rot in enumerate(rots):
        d = base_desc(400 + n)
        rot = np.float32(rot)
        a1, a2 = (rot, np.float32(0)) if rot >= 0 else (np.float32(0), -rot)
        k1.append(key(d, 100, 5.0 * n, n, angle=a1))
        k2.append(key(flip(d, n % 9), 300, 5.0 * n, n, angle=a2))
    return craft(k1, k2, check_orientation=check)


def _bins(counts):
    return [30.0 * b for b, n in counts.items() for _ in range(n)]


@functools.lru_cache(maxsize=None)
def cases():
    S = synth.synth_match_pair
    micro, _ = _micro()
    out = dict(
        synth_small=S(1),
        synth_mid=S(2, n_true=150, n_distract1=60, n_distract2=50, n_nodes=20, flip_bits=20, mp1=0.2, mp2=0.2),
        synth_loose=S(3, n_true=120, n_distract1=30, n_distract2=30, n_nodes=6, flip_bits=25, unshared=0.2),   # distances around th_low
        synth_no_ori=S(4, n_true=90, n_distract1=25, n_distract2=35, n_nodes=10, check_orientation=False),
        synth_3_levels=S(5, n_true=70, n_levels=3, n_nodes=5, noise=1.5),
        big_node=S(6, n_true=380, n_distract1=40, n_distract2=30, n_nodes=60, big_node=300, flip_bits=16),
        empty1=S(7, n_true=40).copy(desc1=np.zeros((0, 32), np.uint8), has_mp1=[], uv1=np.zeros((0, 2)), angle1=[], node_id1=[], node_begin1=[0], node_feat1=[]),
        empty2=S(8, n_true=40).copy(desc2=np.zeros((0, 32), np.uint8), has_mp2=[], uv2=np.zeros((0, 2)), angle2=[], oct2=[], node_id2=[], node_begin2=[0], node_feat2=[]),
        micro=micro,
        jumps=_jumps(),
        den0=_den0(),
        # rot < 0 (-340 -> 20 -> bin 1; -15 -> 345 -> bin 12; -345 -> 15 -> 0.5 -> bin 1), and rot * factor on .5 exactly: 0.5 -> 1 and 4.5 -> 5 (half to
        # even: 0 and 4)
        ori_round=_ori([-340.0, -340.0, -15.0, -345.0, half_rot(0), half_rot(0), half_rot(4), half_rot(4), half_rot(4), 30.0, 150.0]),
        ori_max2_cut=_ori(_bins({3: 21, 5: 2, 7: 1})),           # max2 = 2 < 0.1f * 21: ind2 = ind3 = -1
        ori_max3_cut=_ori(_bins({3: 21, 5: 10, 7: 2})),          # max3 = 2 < 0.1f * 21: ind3 = -1
        ori_edge=_ori(_bins({3: 20, 5: 2, 7: 2})),               # 0.1f * 20.0f == 2.0f: 2 < 2 is false, all three kept
        ori_equal=_ori(_bins({2: 5, 4: 5, 6: 5, 8: 5})),         # the strict > picks the first three; bin 8 is dropped
        ori_one_bin=_ori(_bins({4: 12})),
    )
    out["no_shared"] = out["jumps"].copy(node_id2=out["jumps"].node_id2 + np.uint32(1000))
    return out


def toggled(p):
    """the same pair with check_orientation the other way"""
    return p.copy(check_orientation=not p.check_orientation)


@functools.lru_cache(maxsize=None)
def ref(name, dtype="float64", form="seq", toggle=False):
    p = cases()[name]
    return ref_mod.search_tri_ref(toggled(p) if toggle else p, dtype=getattr(np, dtype), form=form)


def micro_expect():
    return _micro()[1]


def check_against(name, got, want):
    """got: an abi.SearchTriResult, want: the yardstick's dict -- every integer output equal, nothing excused"""
    assert got.status == 0, name
    for k in ref_mod.INT_KEYS:
        g, w = np.asarray(getattr(got, k)), np.asarray(want[k])
        assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differs\n got  %s\n want %s" % (name, k, g, w)
