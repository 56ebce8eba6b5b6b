"""The seeded cases of the vba_sim3_ransac tests in one place: (seed, n_pairs, fix_scale, outlier_frac, same_K, n_hyp, min_inliers).
n_pairs walks the edges of the 64-pair ballot chunks (63, 64, 65) and the smallest legal candidate (3); n_hyp walks 1, 5, 64, 257
(one more than the lanes that run Horn) and 300 (the reference's budget).  The seeds were picked so that every hypothesis of every
case satisfies the conditions tests/test_sim3_ransac_ref.py asserts (eigenvalue gap, gate margin); what each case is there for is
asserted there too (KINDS)."""
import functools

from mc_slam_amd import synth

CASES = [
    (4, 3, 0, 0.0, False, 1, 2),       # the smallest candidate: c = 3 > 2, a hit at 0
    (1, 3, 1, 0.0, True, 1, 3),        # n_pairs == min_inliers: c = 3 is no hit (strict >)
    (4, 25, 0, 0.0, False, 5, 20),     # hit at 3
    (4, 25, 1, 0.2, False, 5, 20),     # no hit
    (3, 63, 0, 0.3, False, 64, 20),    # a late hit (56)
    (4, 63, 0, 0.3, False, 64, 20),    # hit at 0
    (2, 64, 1, 0.4, False, 64, 20),    # hit at 1
    (6, 65, 0, 0.5, False, 64, 20),    # no hit with max c == min_inliers: the strict-> edge
    (5, 120, 1, 0.6, True, 64, 20),
    (1, 120, 0, 0.5, False, 257, 60),  # no hit over 257 hypotheses: the second round of phase A is consumed
    (3, 120, 0, 0.6, False, 300, 20),  # a late hit (242)
    (7, 400, 0, 0.6, False, 300, 20),
    (1, 400, 1, 0.3, False, 300, 20),  # hit at 0 of 300
]
IDS = ["s%d-n%d-f%d-o%g-k%d-h%d-m%d" % (c[0], c[1], c[2], c[3], int(c[4]), c[5], c[6]) for c in CASES]


@functools.lru_cache(maxsize=None)
def make(case):
    """the abi.Sim3RansacProblem of a case (shared between the tests: treat it as read-only)"""
    seed, n, fix_scale, outlier_frac, same_K, n_hyp, min_inliers = case
    p = synth.make_sim3_ransac(seed, n, fix_scale, outlier_frac, same_K=same_K)
    return p.copy(sample=synth.draw_triples(seed + 1000, n, n_hyp), min_inliers=min_inliers)


@functools.lru_cache(maxsize=None)
def reference(case, dtype_name="float64"):
    """the yardstick's answer for a case, computed once per dtype"""
    import numpy as np
    import sim3_ransac_ref as ref
    return ref.ransac(make(case), getattr(np, dtype_name))
