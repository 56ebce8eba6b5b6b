"""The cases of the vba_search_for_initialization tests: hand-made pairs and synthetic ones (mc_slam_amd.synth.search_init_scene), the
smallest shapes at which the kernel can still go wrong.  cases() builds every problem once; ref(name, dtype, ignore_claims) is the
yardstick's answer (tests/search_init_ref.py) and proto(name) the answer of its prototype of the kernel's pass, each computed once and
shared by the tests (treat all of them as read-only).

The hand-made pairs use the 80 x 60 image and the 8 x 6 grid (cells of 10 pixels) of tests/fuse_cases.py, windowSize 5, th_low 50,
nn_ratio 0.9 and no orientation filter unless a case says otherwise.  A keypoint of frame 2 lies on (integer + 1/8), a vbPrevMatched
entry on (integer + 1/4), so nothing sits on a threshold: tests/test_search_init_ref.py asserts the margins.  slot(n) is a lattice
of places 12 pixels apart: with windowSize 5 the areas of two slots do not meet.  flip(D, k) is k bits off D, and two such
descriptors of the same D are |k1 - k2| bits apart."""
import functools

import numpy as np

from mc_slam_amd import abi, synth
from fuse_cases import COLS, H, ROWS, W, base_desc, flip
import search_init_ref as ref_mod

D = [base_desc(900 + i) for i in range(24)]


def slot(n):
    return 8.0 + 12.0 * (n % 6), 8.0 + 12.0 * (n // 6)


def k2(x, y, desc, oct=0, angle=10.0):
    """a keypoint of frame 2 at (x + 1/8, y + 1/8)"""
    return dict(x=x + 0.125, y=y + 0.125, desc=desc, oct=oct, angle=angle)


def k1(x, y, desc, oct=0, angle=10.0):
    """a keypoint of frame 1 whose vbPrevMatched is (x + 1/4, y + 1/4)"""
    return dict(x=x + 0.25, y=y + 0.25, desc=desc, oct=oct, angle=angle)


def craft(keys1, keys2, insert_order=None, **kw):
    """a pair from lists of k1() and k2(); frame 2's grid is filled as AssignFeaturesToGrid does when it meets the keypoints in
    insert_order (ascending by default)"""
    uv2 = np.array([[k["x"], k["y"]] for k in keys2], dtype=float).reshape(-1, 2)
    order = list(range(len(keys2))) if insert_order is None else list(insert_order)
    inv_w, inv_h = COLS / W, ROWS / H
    begin, feat = abi.grid_csr(uv2[order], (0, W, 0, H), COLS, ROWS, inv_w, inv_h)
    feat = np.asarray(order, dtype=np.int32)[feat]
    col = lambda ks, name, dtype: np.array([k[name] for k in ks], dtype=dtype)
    args = dict(window_size=5.0, th_low=50, nn_ratio=0.9, check_orientation=False)
    args.update(kw)
    return abi.SearchInitProblem(desc1=col(keys1, "desc", np.uint8).reshape(-1, 32), oct1=col(keys1, "oct", np.uint8),
                                 prev_matched=np.array([[k["x"], k["y"]] for k in keys1], dtype=np.float32).reshape(-1, 2),
                                 angle1=col(keys1, "angle", np.float32), desc2=col(keys2, "desc", np.uint8).reshape(-1, 32), uv2=uv2,
                                 oct2=col(keys2, "oct", np.uint8), angle2=col(keys2, "angle", np.float32), bounds=(0, W, 0, H), grid_cols=COLS,
                                 grid_rows=ROWS, grid_inv_w=inv_w, grid_inv_h=inv_h, cell_begin=begin, cell_feat=feat, **args)


def _micro():
    """one keypoint of frame 1 per state, the filter on: every keypoint of frame 2 has angle 10, a match with angle 10 + 30 b falls
    into bin b.  The bins hold 3 (keypoints 0, 5 and 6 of frame 1; 5 is stolen and still counts), 1, 1 and 1 entries: the bins 0, 1, 2
    survive and the match of keypoint 9, in bin 3, is dropped"""
    s = slot
    keys2 = [k2(*s(0), D[0]),                                          # 0: the match of keypoint 0, 5 bits
             k2(*s(1), D[9], oct=2),                                   # 1: under keypoint 2, at another level: the area is empty
             k2(*s(2), flip(D[1], 60)),                                # 2: under keypoint 3, 60 bits off
             k2(*s(3), D[2]), k2(s(3)[0] + 1, s(3)[1] + 1, flip(D[2], 21, 100)),   # 3, 4: under keypoint 4, 10 and 11 bits off
             k2(*s(4), D[3]),                                          # 5: keypoint 5 takes it at 8 bits, keypoint 9 at 3
             k2(*s(5), D[4]), k2(*s(6), D[5]), k2(*s(7), D[6])]        # 6, 7, 8: the matches of the keypoints 6, 7, 8
    keys1 = [k1(*s(0), flip(D[0], 5)),                                 # 0: matched and kept, bin 0
             k1(*s(0), D[0], oct=1),                                   # 1: octave 1
             k1(*s(1), D[9]),                                          # 2: area empty
             k1(*s(2), D[1]),                                          # 3: 60 > th_low
             k1(*s(3), flip(D[2], 10, 100)),                           # 4: 10 < 11 * 0.9 fails
             k1(*s(4), flip(D[3], 8)),                                 # 5: matched, bin 0, then stolen by keypoint 9
             k1(*s(5), flip(D[4], 2)),                                 # 6: matched, bin 0
             k1(*s(6), flip(D[5], 2), angle=40.0),                     # 7: matched, bin 1
             k1(*s(7), flip(D[6], 2), angle=70.0),                     # 8: matched, bin 2
             k1(s(4)[0] + 1, s(4)[1], flip(D[3], 3), angle=100.0)]     # 9: steals keypoint 5 of frame 2, bin 3: dropped
    expect = dict(state=[0, 1, 2, 3, 4, 5, 0, 0, 0, 6], best_idx=[0, -1, -1, 2, 3, 5, 6, 7, 8, 5], best_dist=[5, 256, 256, 60, 10, 8, 2, 2, 2, 3],
                  best_dist2=[256, 256, 256, 256, 11, 256, 256, 256, 256, 256], match12=[0, -1, -1, -1, -1, -1, 6, 7, 8, -1],
                  match21=[0, -1, -1, -1, -1, 9, 6, 7, 8], matched_dist=[5, 256, 256, 256, 256, 3, 2, 2, 2], bin=[0, 255, 255, 255, 255, 0, 0, 1, 2, 3],
                  n_matches=4, n_before_filter=5, n_stolen=1, ind=[0, 1, 2])
    return craft(keys1, keys2, check_orientation=True), expect


def micro_expect():
    return _micro()[1]


def _steal():
    """keypoint 1 takes the keypoint of frame 2 that keypoint 0 holds, at a strictly smaller distance"""
    return craft([k1(*slot(0), flip(D[0], 8)), k1(*slot(0), flip(D[0], 3))], [k2(*slot(0), D[0]), k2(*slot(5), D[1])])


def _equal_no_steal():
    """an equal distance is skipped (<=): keypoint 1 falls back to its second candidate, 20 bits off; keypoint 3 has none and leaves at the threshold"""
    keys2 = [k2(*slot(0), D[0]), k2(slot(0)[0] + 2, slot(0)[1], flip(D[0], 25, 100)), k2(*slot(3), D[1])]
    keys1 = [k1(*slot(0), flip(D[0], 5)), k1(*slot(0), flip(D[0], 5, 100)), k1(*slot(3), flip(D[1], 7)), k1(*slot(3), flip(D[1], 7, 50))]
    return craft(keys1, keys2)


def _ratio_flip():
    """keypoint 1 sees the keypoints 0 and 1 of frame 2 at 10 and 11 bits: the ratio test fails -- unless keypoint 0 holds the first
    at 2 bits, which hides it (2 <= 10): then 11 stands alone and matches"""
    keys2 = [k2(*slot(0), D[0]), k2(slot(0)[0] + 1, slot(0)[1] + 1, flip(D[0], 21, 100))]
    return craft([k1(*slot(0), flip(D[0], 2)), k1(*slot(0), flip(D[0], 10, 100))], keys2)


def _int_max_ratio():
    """one candidate at 40 bits, nn_ratio 0.1: 40 < (float)INT_MAX * 0.1 matches; 40 < 256 * 0.1 would not"""
    return craft([k1(*slot(0), flip(D[0], 40))], [k2(*slot(0), D[0])], nn_ratio=0.1)


def _stolen_in_hist():
    """eleven matches over nine keypoints of frame 2; the keypoints 9 and 10 of frame 1 steal from 7 and 8.  The bins hold 4, 3, 1, 2, 1
    entries with the stolen ones counted (bin 3: one kept, one stolen; bin 4: one stolen): the bins 0, 1, 3 survive, the match of bin 2
    is dropped, and the stolen entry of bin 4 is not decremented again.  Without the stolen entries (4, 3, 1, 1, 0) bin 2 would
    survive and bin 3 would go"""
    bins = [0, 0, 0, 1, 1, 2, 3, 3, 4]                                 # the keypoints 0 .. 8 of frame 1, one keypoint of frame 2 each
    keys2 = [k2(*slot(i), D[i]) for i in range(9)]
    keys1 = [k1(*slot(i), flip(D[i], 9), angle=10.0 + 30.0 * b) for i, b in enumerate(bins)]
    keys1 += [k1(*slot(7), flip(D[7], 4), angle=10.0), k1(*slot(8), flip(D[8], 4), angle=40.0)]
    return craft(keys1, keys2, check_orientation=True)


def _steal_chain(n=40):
    """one keypoint of frame 2, n keypoints of frame 1 at 45, 44, ... bits: every one is accepted and steals from the one before"""
    return craft([k1(*slot(0), flip(D[0], 45 - i)) for i in range(n)], [k2(*slot(0), D[0])])


def _dep_chain(n=40):
    """a dependency chain: frame 2 holds k_1 .. k_n along a line, 1.5 pixels apart, k_j at 5 j + 1 bits from the one descriptor every
    keypoint of frame 1 has; windowSize 1.  Keypoint 0 of frame 1 sees k_1 alone, keypoint q sees k_q and k_(q+1).  Sequentially
    keypoint q finds k_q held at its own distance and takes k_(q+1); the pass learns that one query per round"""
    keys2 = [k2(2.0 + 1.5 * j, 30.0, flip(D[0], 5 * j + 1)) for j in range(1, n + 1)]
    keys1 = [k1(2.0 + 1.5 * (q + 1) - 0.875, 30.0, D[0]) for q in range(n)]   # 0.75 left of k_(q+1): k_q is 0.75 away too, k_(q+2) 2.25
    return craft(keys1, keys2, window_size=1.0, th_low=255, nn_ratio=1.0)


def _crowd_64():
    """64 keypoints of frame 1 on one keypoint of frame 2, at distances that go up and down: all 64 claim it in round 0"""
    dist = [1 + (37 * i + 11) % 50 for i in range(64)]
    return craft([k1(*slot(0), flip(D[0], d)) for d in dist], [k2(*slot(0), D[0]), k2(*slot(9), D[1])])


def _border():
    """the four early returns of GetFeaturesInArea (vbPrevMatched right of, left of, below and above the grid) and cell ranges that
    clamp at the first and the last column and row.  The keypoint at (79, 59) rounds to column 8 and row 6 and is in no cell"""
    keys2 = [k2(1, 1, D[0]), k2(74, 54, D[1]), k2(79, 59, D[2]), k2(40, 30, D[3])]
    keys1 = [k1(95, 30, D[3]), k1(-21, 30, D[3]), k1(40, 75, D[3]), k1(40, -21, D[3]), k1(0, 0, flip(D[0], 3)), k1(76, 56, flip(D[1], 3)),
             k1(78, 58, D[2]), k1(40, 30, flip(D[3], 3))]
    return craft(keys1, keys2)


def scene(seed, n1, n2, **kw):
    args = dict(size=(int(W), int(H)), cols=COLS, rows=ROWS, window_size=30.0)
    args.update(kw)
    return synth.search_init_scene(seed, n1, n2, **args)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["micro"] = _micro()[0]
    c["steal"] = _steal()
    c["equal_no_steal"] = _equal_no_steal()
    c["ratio_flip"] = _ratio_flip()
    c["int_max_ratio"] = _int_max_ratio()
    c["stolen_in_hist"] = _stolen_in_hist()
    c["steal_chain_40"] = _steal_chain()
    c["dep_chain_40"] = _dep_chain()
    c["crowd_64"] = _crowd_64()
    for n in (256, 257, 513):
        c["queries_%d" % n] = scene(400 + n, n, 400, level0=1.0, window_size=10.0)
    c["border"] = _border()
    c["upper_levels_only"] = c["steal"].copy(oct1=np.array([1, 3], dtype=np.uint8))
    c["empty_keys1"] = scene(41, 0, 60)
    c["empty_keys2"] = scene(42, 60, 0)
    c["max_keys"] = scene(43, 12, abi.SEARCH_INIT_MAX_KEYS, window_size=5.0, twins=0.0)
    for k in range(3):
        c["crowd_%d" % k] = scene(50 + k, 150, 150)
    return c


HAND_MADE = ("micro", "steal", "equal_no_steal", "ratio_flip", "int_max_ratio", "stolen_in_hist", "steal_chain_40", "dep_chain_40", "crowd_64", "border")


@functools.lru_cache(maxsize=None)
def ref(name, dtype="float64", ignore_claims=False):
    return ref_mod.search_init_ref(cases()[name], np.dtype(dtype), ignore_claims)


@functools.lru_cache(maxsize=None)
def proto(name):
    return ref_mod.conflict_pass(cases()[name])


def n_queries(p):
    return int((p.oct1 == 0).sum())


def check_against(what, got, want):
    """a library result against a yardstick result: every integer output equal for every keypoint of both frames, prev_matched bit for bit"""
    assert got.status == 0, what
    for k in ("state", "best_idx", "best_dist", "best_dist2", "match12", "bin", "match21", "matched_dist", "hist", "ind"):
        g, w = np.asarray(getattr(got, k)), np.asarray(want[k])
        bad = np.nonzero(g != w)[0]
        assert g.shape == w.shape and len(bad) == 0, (what, k, bad[:8], g[bad[:8]], w[bad[:8]])
    assert (got.n_matches, got.n_before_filter, got.n_stolen) == (want["n_matches"], want["n_before_filter"], want["n_stolen"]), what
    assert got.prev_matched.dtype == np.float32 and got.prev_matched.tobytes() == want["prev_matched"].tobytes(), what
