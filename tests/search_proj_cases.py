"""The cases of the vba_search_by_projection tests: hand-made problems and synthetic ones (mc_slam_amd.synth.search_proj_scene), the
smallest shapes at which the kernel can still go wrong.  cases() builds every problem once; ref(name, dtype) is the yardstick's answer
(tests/search_proj_ref.py, the sequential loop), computed once and shared by the tests (treat both as read-only).

The hand-made problems use the frame of tests/fuse_cases.py: the identity pose, an 80 x 60 image with K = (50, 50, 40, 30), an 8 x 6
grid (cells of 10 pixels) and four levels of factor 1.2.  In last-frame mode they use th = 3 (radii 3, 3.6, 4.32 and 5.184 pixels by
octave); in local-map mode th = 1 and every hand-made point is seen along its normal (viewCos = 1 > 0.998), so the radii are 2.5, 3,
3.6 and 4.32 pixels by level.  Apart from z_zero no case puts a quantity on a threshold: tests/test_search_proj_ref.py asserts the
margins."""
import functools

import numpy as np

from mc_slam_amd import abi, synth
import fuse_cases as fc
import search_proj_ref as ref_mod
from fuse_cases import D, FILLER, flip, key, point

LAST, LOCAL = abi.SEARCH_PROJ_LAST_FRAME, abi.SEARCH_PROJ_LOCAL_MAP

# the largest differences between the float64 and the longdouble yardstick over all cases (tests/test_search_proj_ref.py prints them and
# asserts these bounds on them); the tolerances are ten times that, rounded up to one digit
UV_LONGDOUBLE = 2e-13
UV_TOL = 2e-12
COS_LONGDOUBLE = 3e-16
COS_TOL = 3e-15


def from_fuse(f, mode, q_oct=None, angle=None, q_angle=None, occupied=None, q_blocks=None, **kw):
    """the frame and the points of a vba_fuse problem as a problem of `mode`; a last-frame problem needs q_oct"""
    common = dict(mode=mode, Rcw=f.Rcw, tcw=f.tcw, K=f.K, bounds=f.bounds, desc=f.desc, uv=f.uv, oct=f.oct, scale=f.scale, grid_cols=f.grid_cols,
                  grid_rows=f.grid_rows, grid_inv_w=f.grid_inv_w, grid_inv_h=f.grid_inv_h, cell_begin=f.cell_begin, cell_feat=f.cell_feat,
                  occupied=np.zeros(f.n_keys, dtype=np.uint8) if occupied is None else occupied, q_pos=f.pos, q_desc=f.pt_desc, q_skip=f.skip,
                  q_blocks=np.ones(f.n_pt, dtype=np.uint8) if q_blocks is None else q_blocks)
    if mode == LOCAL:
        common.update(Ow=f.Ow, log_scale_factor=f.log_scale_factor, q_normal=f.normal, q_dist_min=f.dist_min, q_dist_max=f.dist_max, q_pred_max=f.pred_max,
                      th=1.0)
    else:
        common.update(q_oct=np.asarray(q_oct, dtype=np.uint8), th=3.0, check_orientation=angle is not None,
                      angle=np.zeros(f.n_keys, dtype=np.float32) if angle is None else angle,
                      q_angle=np.zeros(f.n_pt, dtype=np.float32) if q_angle is None else q_angle)
    common.update(kw)
    return abi.SearchProjProblem(**common)


def _micro_last():
    """one query per state of the last-frame mode.  The matches fall into the bins 0, 0, 1, 2 and 3: ComputeThreeMaxima keeps 0, 1 and 2,
    the match of query 4 is dropped and its keypoint cleared.  expect: query -> (state, best_idx, best_dist, bin, uv or None)"""
    keys = [key(10, 10, 0, flip(D[0], 5)), key(30, 10, 0, flip(D[1], 4)), key(50, 10, 0, flip(D[2], 3)), key(70, 10, 0, flip(D[3], 2)),
            key(10, 30, 0, flip(D[4], 1)),
            key(30, 30, 1, flip(D[5], 60)),          # 5: the only candidate of query 9, 60 bits off
            key(50, 50, 3, D[6])]                    # 6: in the area of query 8 with its exact descriptor, outside its octave window
    pts = [point(10.5, 10.5, 4.0, D[0]), point(30.5, 10.5, 4.0, D[1]), point(50.5, 10.5, 4.0, D[2]), point(70.5, 10.5, 4.0, D[3]),
           point(10.5, 30.5, 4.0, D[4]),
           point(10.5, 10.5, 4.0, D[0], skip=1),     # 5: skipped
           point(40.5, 30.5, -5.0, D[7]),            # 6: behind
           point(85.0, 30.5, 4.0, D[7]),             # 7: right of the image
           point(50.5, 50.5, 4.0, D[6]),             # 8: the window 0 .. 1 holds no keypoint of its area
           point(30.5, 30.5, 4.0, D[5])]             # 9: a candidate, but 60 > th_high
    q_oct = [0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    angle = np.full(len(keys), 10.0, dtype=np.float32)
    q_angle = np.array([10, 10, 40, 70, 100, 10, 10, 10, 10, 10], dtype=np.float32)
    p = from_fuse(fc.craft(keys, pts), LAST, q_oct=q_oct, angle=angle, q_angle=q_angle, th_high=50)
    expect = {0: (0, 0, 5, 0, (10.5, 10.5)), 1: (0, 1, 4, 0, (30.5, 10.5)), 2: (0, 2, 3, 1, (50.5, 10.5)), 3: (0, 3, 2, 2, (70.5, 10.5)),
              4: (6, 4, 1, 3, (10.5, 30.5)), 5: (1, -1, 256, 255, None), 6: (2, -1, 256, 255, None), 7: (3, -1, 256, 255, (85.0, 30.5)),
              8: (4, -1, 256, 255, (50.5, 50.5)), 9: (5, 5, 60, 255, (30.5, 30.5))}
    totals = dict(n_matches=4, n_before_filter=5, hist=[2, 1, 1, 1] + [0] * 26, ind=[0, 1, 2], key_match=[0, 1, 2, 3, -2, -1, -1])
    return p, expect, totals


def _micro_local():
    """one query per state of the local-map mode.  expect: query -> (state, best_idx, best_dist, best_dist2, level, uv or None)"""
    keys = [key(20, 20, 0, flip(D[0], 5)),           # 0: the match of query 0, alone in its area
            key(61, 41, 1, flip(D[1], 60)),          # 1: the only candidate of query 8, 60 bits off
            key(60, 20, 1, flip(D[2], 10)),          # 2 and 3: both candidates of query 9 at one level, 10 and 11 bits off
            key(61, 21, 1, flip(D[2], 11, 100))] + FILLER
    pts = [point(20.5, 20.5, 4.0, D[0], level=0),                       # 0: matched
           point(20.5, 20.5, 4.0, D[0], level=0, skip=1),               # 1: skipped
           point(40.5, 30.5, -5.0, D[6]),                               # 2: behind
           point(85.0, 30.5, 4.0, D[6]),                                # 3: right of the image
           point(40.5, 30.5, 4.0, D[6], dmin=2.0),                      # 4: nearer than dist_min
           point(40.5, 30.5, 4.0, D[6], flip_normal=True),              # 5: seen from behind
           point(40.5, 30.5, 4.0, D[6], level=4),                       # 6: level n_levels
           point(10.5, 50.5, 4.0, D[6], level=0),                       # 7: nothing within 2.5 pixels
           point(60.5, 40.5, 4.0, D[1], level=1),                       # 8: a candidate, but 60 > th_high
           point(60.5, 20.5, 4.0, D[2], level=1)]                       # 9: 10 > 0.8 * 11
    p = from_fuse(fc.craft(keys, pts), LOCAL, th_high=50)
    expect = {0: (0, 0, 5, 256, 0, (20.5, 20.5)), 1: (1, -1, 256, 256, -128, None), 2: (2, -1, 256, 256, -128, None),
              3: (3, -1, 256, 256, -128, (85.0, 30.5)), 4: (4, -1, 256, 256, -128, (40.5, 30.5)), 5: (5, -1, 256, 256, -128, (40.5, 30.5)),
              6: (6, -1, 256, 256, 4, (40.5, 30.5)), 7: (7, -1, 256, 256, 0, (10.5, 50.5)), 8: (8, 1, 60, 256, 1, (60.5, 40.5)),
              9: (9, 2, 10, 11, 1, (60.5, 20.5))}
    totals = dict(n_matches=1, n_before_filter=1, key_match=[0, -1, -1, -1, -1, -1, -1, -1])
    return p, expect, totals


def micro_expect(mode):
    return (_micro_last if mode == LAST else _micro_local)()[1:]


CHAIN = 40


def _chain():
    """CHAIN queries with one descriptor at one pixel over a cluster of CHAIN keypoints that lie i + 1 bits from it: query i ends on
    keypoint i, and a round of the conflict pass settles exactly one more query (CHAIN + 1 rounds)"""
    keys = [key(40.0 + 0.02 * i, 30.0, 0, flip(D[0], i + 1)) for i in range(CHAIN)] + FILLER
    pts = [point(40.4, 30.2, 4.0, D[0]) for _ in range(CHAIN)]
    return from_fuse(fc.craft(keys, pts), LAST, q_oct=[0] * CHAIN)


def _overwrite():
    """query 0 does not block (Observations() == 0): query 1 takes the same keypoint 0 and overwrites it; query 2 finds it blocked and
    takes keypoint 1.  Keypoint 2 was occupied before the call: query 3, which has its descriptor, takes keypoint 3 instead; query 4
    sees keypoint 2 only and leaves with state 5 and bestDist 256"""
    keys = [key(20, 20, 0, flip(D[0], 2)), key(21, 20, 0, flip(D[0], 7)), key(60, 40, 0, D[1]), key(61, 40, 0, flip(D[1], 9)), key(30, 50, 0, D[2])] + FILLER
    pts = [point(20.4, 20.2, 4.0, D[0]), point(20.4, 20.2, 4.0, D[0]), point(20.4, 20.2, 4.0, D[0]), point(60.4, 40.2, 4.0, D[1]),
           point(30.4, 50.2, 4.0, D[2])]
    occ = np.zeros(len(keys), dtype=np.uint8)
    occ[[2, 4]] = 1
    p = from_fuse(fc.craft(keys, pts), LAST, q_oct=[0] * 5, occupied=occ, q_blocks=[0, 1, 1, 1, 1])
    return p, dict(best_idx=[0, 0, 1, 3, -1], best_dist=[2, 2, 7, 9, 256], state=[0, 0, 0, 0, 5], key_match=[1, 2, -1, 3, -1] + [-1] * len(FILLER), n_matches=4)


def _drop_clears_kept():
    """query 0 (not blocking, bin 3) and query 1 (bin 0) both write keypoint 0; the bins hold 2, 1, 1 and 1 matches, bin 3 is dropped and
    clears keypoint 0 although query 1, which wrote it last, is kept"""
    keys = [key(20, 20, 0, flip(D[0], 2)), key(40, 20, 0, flip(D[1], 2)), key(60, 20, 0, flip(D[2], 2)), key(20, 40, 0, flip(D[3], 2))] + FILLER
    pts = [point(20.4, 20.2, 4.0, D[0]), point(20.4, 20.2, 4.0, D[0]), point(40.4, 20.2, 4.0, D[1]), point(60.4, 20.2, 4.0, D[2]), point(20.4, 40.2, 4.0, D[3])]
    angle = np.full(len(keys), 10.0, dtype=np.float32)
    q_angle = np.array([100, 10, 10, 40, 70], dtype=np.float32)
    p = from_fuse(fc.craft(keys, pts), LAST, q_oct=[0] * 5, angle=angle, q_angle=q_angle, q_blocks=[0, 1, 1, 1, 1])
    return p, dict(state=[6, 0, 0, 0, 0], best_idx=[0, 0, 1, 2, 3], bin=[3, 0, 0, 1, 2], key_match=[-2, 2, 3, 4] + [-1] * len(FILLER), n_matches=4,
                   n_before_filter=5, ind=[0, 1, 2])


def _ratio_blocked():
    """local-map mode.  Cluster A: query 0 takes keypoint 0; query 1 would fail the ratio test with it (10 > 0.8 * 11) and passes
    without it (11 against no second).  Cluster B: query 2 takes keypoint 2; query 3 would pass with it (5 against 20) and fails
    without it (20 > 0.8 * 21)"""
    keys = [key(20, 20, 1, flip(D[0], 10)), key(21, 20, 1, flip(D[0], 11, 100)),
            key(60, 40, 1, flip(D[1], 5)), key(61, 40, 1, flip(D[1], 20, 50)), key(60, 41, 1, flip(D[1], 21, 120))] + FILLER
    pts = [point(20.4, 20.2, 4.0, flip(D[0], 10), level=1), point(20.4, 20.2, 4.0, D[0], level=1),
           point(60.4, 40.2, 4.0, flip(D[1], 5), level=1), point(60.4, 40.2, 4.0, D[1], level=1)]
    p = from_fuse(fc.craft(keys, pts), LOCAL)
    return p, dict(state=[0, 0, 0, 9], best_idx=[0, 1, 2, 3], best_dist=[0, 11, 0, 20], best_dist2=[21, 256, 25, 21],
                   key_match=[0, 1, 2, -1, -1] + [-1] * len(FILLER), n_matches=3)


def _float32_product():
    """nn_ratio = 0.9f with distances 9 and 10 at one level: 0.9f * 10 is 9.0 in float32, so 9 > 9.0 is false and the query matches;
    in float64 the product is 8.9999998 and the query would fail"""
    keys = [key(20, 20, 1, flip(D[0], 9)), key(21, 20, 1, flip(D[0], 10, 100))] + FILLER
    p = from_fuse(fc.craft(keys, [point(20.4, 20.2, 4.0, D[0], level=1)]), LOCAL, nn_ratio=0.9)
    return p, dict(state=[0], best_idx=[0], best_dist=[9], best_dist2=[10], n_matches=1)


def _octave_edges():
    """last-frame mode: octave 0 (minLevel = -1) sees the octaves 0 and 1, the top octave 3 sees 2 and 3; the nearer descriptors lie
    outside the windows"""
    keys = [key(20, 20, 0, flip(D[0], 8)), key(21, 20, 1, flip(D[0], 6)), key(20, 21, 2, flip(D[0], 1)),
            key(60, 40, 3, flip(D[1], 8)), key(61, 40, 2, flip(D[1], 6)), key(60, 41, 1, flip(D[1], 1))] + FILLER
    pts = [point(20.4, 20.2, 4.0, D[0]), point(60.4, 40.2, 4.0, D[1])]
    p = from_fuse(fc.craft(keys, pts), LAST, q_oct=[0, 3])
    return p, dict(state=[0, 0], best_idx=[1, 4], best_dist=[6, 6])


def hand_expect():
    """name -> the hand-made answers of the small cases"""
    return {n: f()[1] for n, f in (("overwrite", _overwrite), ("drop_clears_kept", _drop_clears_kept), ("ratio_blocked", _ratio_blocked),
                                   ("float32_product", _float32_product), ("octave_edges", _octave_edges))}


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["micro_last"] = _micro_last()[0]
    c["micro_local"] = _micro_local()[0]
    c["chain_40"] = _chain()
    c["overwrite"] = _overwrite()[0]
    c["drop_clears_kept"] = _drop_clears_kept()[0]
    c["ratio_blocked"] = _ratio_blocked()[0]
    c["float32_product"] = _float32_product()[0]
    c["octave_edges"] = _octave_edges()[0]
    c["level_edges_local"] = from_fuse(fc._level_edges(), LOCAL)
    # the border cases of fuse_cases: clamped cell ranges, a radius larger than the image, the four early returns (a negative radius)
    c["border_local"] = from_fuse(fc._border(), LOCAL)
    c["border_last"] = from_fuse(fc._border(), LAST, q_oct=[0, 3, 0, 1, 0, 2])
    c["border_all_local"] = from_fuse(fc._border(), LOCAL, th=400.0)
    c["border_all_last"] = from_fuse(fc._border(), LAST, q_oct=[0, 3, 0, 1, 0, 2], th=1000.0)
    c["border_returns_local"] = from_fuse(fc._border_returns(), LOCAL, th=-8.0)
    c["border_returns_last"] = from_fuse(fc._border_returns(), LAST, q_oct=[0] * 5, th=-20.0)
    z = fc._z_zero()
    c["z_zero_local"] = from_fuse(z, LOCAL)
    c["z_zero_last"] = from_fuse(z, LAST, q_oct=[0] * z.n_pt)
    for mode, tag in ((LAST, "last"), (LOCAL, "local")):
        c["empty_q_" + tag] = synth.search_proj_scene(22, mode, n_keys=50, n_q=0)
        c["empty_keys_" + tag] = synth.search_proj_scene(23, mode, n_keys=0, n_q=40)
        c["synth_small_" + tag] = synth.search_proj_scene(32, mode, n_keys=200, n_q=120)
        c["synth_mid_" + tag] = synth.search_proj_scene(31, mode, n_keys=1000, n_q=600)
        # more matching queries than keypoints: most keypoints are wanted twice or more
        c["crowd_" + tag] = synth.search_proj_scene(41, mode, n_keys=120, n_q=400, twins=0.5)
        c["crowd2_" + tag] = synth.search_proj_scene(42, mode, n_keys=150, n_q=450, twins=0.5, non_blocking=0.25)
    for k, n in enumerate((255, 256, 257, 513)):
        c["queries_%d" % n] = synth.search_proj_scene(300 + n, (LAST, LOCAL)[k % 2], n_keys=200, n_q=n)
    c["no_orientation"] = c["synth_small_last"].copy(check_orientation=False)
    # the largest frame the entry point takes: the claim table fills the dynamic LDS
    c["max_keys"] = synth.search_proj_scene(51, LOCAL, n_keys=abi.SEARCH_PROJ_MAX_KEYS, n_q=96, twins=0.0, cols=128, rows=96)
    return c


@functools.lru_cache(maxsize=None)
def ref(name, dtype="float64", ignore_claims=False):
    return ref_mod.search_proj_ref(cases()[name], np.dtype(dtype), ignore_claims)


def check_against(what, got, want, uv_tol=UV_TOL, cos_tol=COS_TOL):
    """a library result against a yardstick result: every integer output equal for every query and every keypoint, uv and view_cos
    within their tolerances with the same non-finite entries, 1 <= rounds <= n_q + 1.  Returns the largest uv and view_cos
    differences"""
    assert got.status == 0, what
    for k in ("state", "best_idx", "best_dist", "best_dist2", "level", "bin", "key_match", "hist", "ind"):
        g, w = np.asarray(getattr(got, k)), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (what, k, bad[:8], g[bad[:8]], w[bad[:8]])
    assert (got.n_matches, got.n_before_filter) == (want["n_matches"], want["n_before_filter"]), what
    assert 1 <= got.rounds <= len(want["state"]) + 1, (what, got.rounds)
    du = ref_mod.real_difference(dict(uv=got.uv), want, "uv")
    dc = ref_mod.real_difference(dict(view_cos=got.view_cos), want, "view_cos")
    assert du <= uv_tol and dc <= cos_tol, (what, du, dc)
    return du, dc
