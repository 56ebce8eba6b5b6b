"""The seeded cases of the vba_triangulate tests in one place: (seed, n_matches, kind) of synth.make_triangulate.  n_matches walks
the wave and workgroup boundaries of the kernel (one lane per match, 256 lanes per workgroup): 0, 1, 63, 64, 65, 255, 256, 257 and
513 (three workgroups).  'far' is the pair about 50 m from the origin with parallaxes just inside the gate; 'forward' holds the
deliberately made matches of reasons 4 and 6.  The conditions the GPU comparison rests on (the smallest margin of every
comparison, how often every reason occurs) are asserted in tests/test_triangulate_ref.py."""
import functools

from mc_slam_amd import synth

CASES = [
    (1, 0, "std"),
    (2, 1, "std"),
    (3, 63, "std"),
    (4, 64, "forward"),
    (5, 65, "std"),
    (6, 255, "forward"),
    (7, 256, "std"),
    (8, 257, "far"),
    (9, 513, "std"),
    (10, 513, "forward"),
    (11, 257, "std"),
]
IDS = ["s%d-n%d-%s" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def make(case):
    """the abi.TriangulateProblem of a case (shared between the tests: treat it as read-only)"""
    seed, n, kind = case
    return synth.make_triangulate(seed, n, kind, same_K=(seed % 2 == 0))


@functools.lru_cache(maxsize=None)
def reference(case, dtype_name="float64"):
    """the yardstick's answer for a case, computed once per dtype"""
    import numpy as np
    import triangulate_ref as ref
    return ref.triangulate(make(case), getattr(np, dtype_name))
