"""The cases of the vba_search_by_projection_kf tests: hand-made problems and synthetic ones (mc_slam_amd.synth.search_proj_kf_scene), the
smallest shapes at which the kernel can still go wrong.  cases() builds every problem once; ref(name, dtype) is the yardstick's answer
(tests/search_proj_kf_ref.py, the sequential loop), computed once and shared by the tests (treat both as read-only).

The hand-made problems use the frame of tests/fuse_cases.py: the identity pose, an 80 x 60 image with K = (50, 50, 40, 30), an 8 x 6
grid (cells of 10 pixels) and four levels of factor 1.2, with th = 3 (radii 3, 3.6, 4.32 and 5.184 pixels by level) and th_dist = 50
in both modes.  Apart from z_zero no case puts a quantity on a threshold: tests/test_search_proj_kf_ref.py asserts the margins."""
import functools

import numpy as np

from mc_slam_amd import abi, synth
import fuse_cases as fc
import search_proj_kf_ref as ref_mod
from fuse_cases import D, FILLER, flip, key, point

LOOP, RELOC = abi.SEARCH_PROJ_KF_LOOP, abi.SEARCH_PROJ_KF_RELOC
TAGS = ((LOOP, "loop"), (RELOC, "reloc"))

# the largest |uv| difference between the float64 and the longdouble yardstick over all cases (tests/test_search_proj_kf_ref.py prints
# it and asserts this bound on it); the tolerance is ten times that, rounded up to one digit
UV_LONGDOUBLE = 2e-13
UV_TOL = 2e-12


def from_fuse(f, mode, occupied=None, angle=None, q_angle=None, **kw):
    """the keyframe and the points of a vba_fuse problem as a problem of `mode`"""
    common = dict(mode=mode, Rcw=f.Rcw, tcw=f.tcw, Ow=f.Ow, K=f.K, bounds=f.bounds, desc=f.desc, uv=f.uv, oct=f.oct, scale=f.scale,
                  log_scale_factor=f.log_scale_factor, grid_cols=f.grid_cols, grid_rows=f.grid_rows, grid_inv_w=f.grid_inv_w, grid_inv_h=f.grid_inv_h,
                  cell_begin=f.cell_begin, cell_feat=f.cell_feat, occupied=np.zeros(f.n_keys, dtype=np.uint8) if occupied is None else occupied,
                  q_pos=f.pos, q_desc=f.pt_desc, q_skip=f.skip, q_dist_min=f.dist_min, q_dist_max=f.dist_max, q_pred_max=f.pred_max, th=3.0, th_dist=50)
    if mode == LOOP:
        common.update(q_normal=f.normal)
    else:
        common.update(check_orientation=angle is not None, angle=np.zeros(f.n_keys, dtype=np.float32) if angle is None else angle,
                      q_angle=np.zeros(f.n_pt, dtype=np.float32) if q_angle is None else q_angle)
    common.update(kw)
    return abi.SearchProjKfProblem(**common)


def _micro_loop():
    """one query per state of the loop mode, and a second way into state 8.  expect: query -> (state, best_idx, best_dist, level, uv or None)"""
    keys = [key(20, 20, 0, flip(D[0], 5)),           # 0: the match of query 0
            key(61, 41, 1, flip(D[1], 60)),          # 1: the only candidate of query 8, 60 bits off
            key(62, 21, 0, D[2])] + FILLER           # 2: in the area of query 9 with its exact descriptor, two levels below it
    pts = [point(20.5, 20.5, 4.0, D[0], level=0),                       # 0: matched
           point(20.5, 20.5, 4.0, D[0], level=0, skip=1),               # 1: skipped
           point(40.5, 30.5, -5.0, D[6]),                               # 2: behind
           point(85.0, 30.5, 4.0, D[6]),                                # 3: right of the image
           point(40.5, 30.5, 4.0, D[6], dmin=2.0),                      # 4: nearer than dist_min
           point(40.5, 30.5, 4.0, D[6], flip_normal=True),              # 5: seen from behind
           point(40.5, 30.5, 4.0, D[6], level=4),                       # 6: level n_levels
           point(10.5, 50.5, 4.0, D[6], level=0),                       # 7: nothing within 3 pixels
           point(60.5, 40.5, 4.0, D[1], level=1),                       # 8: a candidate, but 60 > th_dist
           point(60.5, 20.5, 4.0, D[2], level=2)]                       # 9: a keypoint in the area, none at its levels
    expect = {0: (0, 0, 5, 0, (20.5, 20.5)), 1: (1, -1, 256, -128, None), 2: (2, -1, 256, -128, None), 3: (3, -1, 256, -128, (85.0, 30.5)),
              4: (4, -1, 256, -128, (40.5, 30.5)), 5: (5, -1, 256, -128, (40.5, 30.5)), 6: (6, -1, 256, 4, (40.5, 30.5)),
              7: (7, -1, 256, 0, (10.5, 50.5)), 8: (8, 1, 60, 1, (60.5, 40.5)), 9: (8, -1, 256, 2, (60.5, 20.5))}
    totals = dict(n_matches=1, n_before_filter=1, hist=[0] * 30, ind=[-1, -1, -1], key_match=[0] + [-1] * (2 + len(FILLER)))
    return from_fuse(fc.craft(keys, pts), LOOP), expect, totals


def _micro_reloc():
    """one query per state of the reloc mode.  The matches fall into the bins 0, 0, 1, 2 and 3: ComputeThreeMaxima keeps 0, 1 and 2, the
    match of query 4 is dropped and its keypoint cleared.  expect: query -> (state, best_idx, best_dist, level, bin, uv or None)"""
    keys = [key(10, 10, 0, flip(D[0], 5)), key(30, 10, 0, flip(D[1], 4)), key(50, 10, 0, flip(D[2], 3)), key(70, 10, 0, flip(D[3], 2)),
            key(10, 30, 0, flip(D[4], 1)),
            key(30, 30, 1, flip(D[5], 60)),          # 5: the only candidate of query 10, 60 bits off
            key(50, 50, 3, D[6])]                    # 6: in the area of query 9 with its exact descriptor, outside its level window
    pts = [point(10.5, 10.5, 4.0, D[0]), point(30.5, 10.5, 4.0, D[1]), point(50.5, 10.5, 4.0, D[2]), point(70.5, 10.5, 4.0, D[3]),
           point(10.5, 30.5, 4.0, D[4]),
           point(10.5, 10.5, 4.0, D[0], skip=1),     # 5: skipped
           point(85.0, 30.5, 4.0, D[7]),             # 6: right of the image
           point(40.5, 30.5, 4.0, D[7], dmin=2.0),   # 7: nearer than dist_min
           point(40.5, 30.5, 4.0, D[7], level=4),    # 8: level n_levels
           point(50.5, 50.5, 4.0, D[6]),             # 9: the window -1 .. 1 holds no keypoint of its area
           point(30.5, 30.5, 4.0, D[5], level=1)]    # 10: a candidate, but 60 > th_dist
    angle = np.full(len(keys), 10.0, dtype=np.float32)
    q_angle = np.array([10, 10, 40, 70, 100, 10, 10, 10, 10, 10, 10], dtype=np.float32)
    expect = {0: (0, 0, 5, 0, 0, (10.5, 10.5)), 1: (0, 1, 4, 0, 0, (30.5, 10.5)), 2: (0, 2, 3, 0, 1, (50.5, 10.5)), 3: (0, 3, 2, 0, 2, (70.5, 10.5)),
              4: (7, 4, 1, 0, 3, (10.5, 30.5)), 5: (1, -1, 256, -128, 255, None), 6: (2, -1, 256, -128, 255, (85.0, 30.5)),
              7: (3, -1, 256, -128, 255, (40.5, 30.5)), 8: (4, -1, 256, 4, 255, (40.5, 30.5)), 9: (5, -1, 256, 0, 255, (50.5, 50.5)),
              10: (6, 5, 60, 1, 255, (30.5, 30.5))}
    totals = dict(n_matches=4, n_before_filter=5, hist=[2, 1, 1, 1] + [0] * 26, ind=[0, 1, 2], key_match=[0, 1, 2, 3, -2, -1, -1])
    return from_fuse(fc.craft(keys, pts), RELOC, angle=angle, q_angle=q_angle), expect, totals


def micro_expect(mode):
    return (_micro_loop if mode == LOOP else _micro_reloc)()[1:]


CHAIN = 40


def _chain(mode):
    """CHAIN queries with one descriptor at one pixel over a cluster of CHAIN keypoints that lie i + 1 bits from it: all prefer
    keypoint 0, then 1, and so on; query i ends on keypoint i, and a round of the conflict pass settles exactly one more query
    (CHAIN + 1 rounds)"""
    keys = [key(40.0 + 0.02 * i, 30.0, 0, flip(D[0], i + 1)) for i in range(CHAIN)] + FILLER
    pts = [point(40.4, 30.2, 4.0, D[0]) for _ in range(CHAIN)]
    return from_fuse(fc.craft(keys, pts), mode)


def _behind_reloc():
    """the mirror image of a matching point through the camera centre: z = -4, the same pixel, the same distance.  The reloc mode has
    no depth test: it matches.  Query 1 is the point in front, which finds keypoint 0 taken and takes keypoint 1"""
    keys = [key(20, 20, 0, flip(D[0], 5)), key(21, 20, 0, flip(D[0], 9))] + FILLER
    q = point(20.5, 20.5, 4.0, D[0])
    b = dict(q, pos=-q["pos"])
    return from_fuse(fc.craft(keys, [b, q]), RELOC), dict(state=[0, 0], best_idx=[0, 1], best_dist=[5, 9], level=[0, 0], n_matches=2,
                                                          key_match=[0, 1] + [-1] * len(FILLER))


def _levels(mode):
    """query 0 (level 0) over a keypoint of level 1, 3 bits off: a candidate at L + 1 is taken in reloc mode and skipped in loop mode.
    Query 1 (level 0) over a keypoint of level 3 with its exact descriptor: the area holds only other levels, which is an empty area
    in reloc mode (state 5) and a non-empty one without a candidate in loop mode (state 8, best_idx -1, best_dist 256)"""
    keys = [key(20, 20, 1, flip(D[0], 3)), key(60, 40, 3, D[1])] + FILLER
    pts = [point(20.4, 20.3, 4.0, D[0], level=0), point(60.4, 40.3, 4.0, D[1], level=0)]
    if mode == LOOP:
        want = dict(state=[8, 8], best_idx=[-1, -1], best_dist=[256, 256], level=[0, 0], n_matches=0)
    else:
        want = dict(state=[0, 5], best_idx=[0, -1], best_dist=[3, 256], level=[0, 0], n_matches=1)
    return from_fuse(fc.craft(keys, pts), mode), want


def _all_taken(mode):
    """both keypoints of the area held a point before the call: state 8 in loop mode and state 6 in reloc mode, with no candidate"""
    keys = [key(20, 20, 0, D[0]), key(21, 20, 0, flip(D[0], 2))] + FILLER
    occ = np.zeros(len(keys), dtype=np.uint8)
    occ[:2] = 1
    p = from_fuse(fc.craft(keys, [point(20.4, 20.3, 4.0, D[0])]), mode, occupied=occ)
    return p, dict(state=[8 if mode == LOOP else 6], best_idx=[-1], best_dist=[256], level=[0], n_matches=0, key_match=[-1] * len(keys))


def hand_expect():
    """name -> the hand-made answers of the small cases"""
    out = {"behind_reloc": _behind_reloc()[1]}
    for mode, tag in TAGS:
        out["levels_" + tag] = _levels(mode)[1]
        out["all_taken_" + tag] = _all_taken(mode)[1]
    return out


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["micro_loop"] = _micro_loop()[0]
    c["micro_reloc"] = _micro_reloc()[0]
    c["chain_40"] = _chain(LOOP)
    c["chain_40_reloc"] = _chain(RELOC)
    c["behind_reloc"] = _behind_reloc()[0]
    z = fc._z_zero()
    for mode, tag in TAGS:
        c["levels_" + tag] = _levels(mode)[0]
        c["all_taken_" + tag] = _all_taken(mode)[0]
        c["level_edges_" + tag] = from_fuse(fc._level_edges(), mode)
        c["tie_cells_" + tag] = from_fuse(fc._tie_cells(), mode)
        # the border cases of fuse_cases: clamped cell ranges (the CEIL of the last cell), a radius larger than the image, the four
        # early returns (a negative radius)
        c["border_" + tag] = from_fuse(fc._border(), mode)
        c["border_all_" + tag] = from_fuse(fc._border(), mode, th=1000.0)
        c["border_returns_" + tag] = from_fuse(fc._border_returns(), mode, th=-20.0)
        c["z_zero_" + tag] = from_fuse(z, mode)
        c["empty_q_" + tag] = synth.search_proj_kf_scene(22, mode, n_keys=50, n_q=0)
        c["empty_keys_" + tag] = synth.search_proj_kf_scene(23, mode, n_keys=0, n_q=40)
        c["synth_small_" + tag] = synth.search_proj_kf_scene(32, mode, n_keys=200, n_q=120)
        c["synth_mid_" + tag] = synth.search_proj_kf_scene(31, mode, n_keys=1000, n_q=600)
        # more matching queries than keypoints: most keypoints are wanted twice or more
        c["crowd_" + tag] = synth.search_proj_kf_scene(41, mode, n_keys=120, n_q=400, twins=0.5)
    for k, n in enumerate((255, 256, 257, 513)):
        c["queries_%d" % n] = synth.search_proj_kf_scene(300 + n, (LOOP, RELOC)[k % 2], n_keys=200, n_q=n)
    c["no_orientation"] = c["synth_small_reloc"].copy(check_orientation=False)
    # the largest target the entry point takes: the claim table fills the dynamic LDS
    c["max_keys"] = synth.search_proj_kf_scene(51, RELOC, n_keys=abi.SEARCH_PROJ_KF_MAX_KEYS, n_q=96, twins=0.0, cols=128, rows=96)
    return c


@functools.lru_cache(maxsize=None)
def ref(name, dtype="float64", ignore_claims=False):
    return ref_mod.search_proj_kf_ref(cases()[name], np.dtype(dtype), ignore_claims)


def check_against(what, got, want, uv_tol=UV_TOL):
    """a library result against a yardstick result: every integer output equal for every query and every keypoint, uv within its
    tolerance with the same non-finite entries, 1 <= rounds <= n_q + 1.  Returns the largest uv difference"""
    assert got.status == 0, what
    for k in ("state", "best_idx", "best_dist", "level", "bin", "key_match", "hist", "ind"):
        g, w = np.asarray(getattr(got, k)), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (what, k, bad[:8], g[bad[:8]], w[bad[:8]])
    assert (got.n_matches, got.n_before_filter) == (want["n_matches"], want["n_before_filter"]), what
    assert 1 <= got.rounds <= len(want["state"]) + 1, (what, got.rounds)
    du = ref_mod.real_difference(dict(uv=got.uv), want, "uv")
    assert du <= uv_tol, (what, du)
    return du
