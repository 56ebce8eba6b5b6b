"""The graphs of the pose-graph tests and the tolerances of the GPU comparison (tests/test_gpu_posegraph.py).

Every graph is the smallest at which one part of k_posegraph_opt can go wrong; all have a fixed vertex.

TOL_*: the GPU differs from the float64 yardstick (tests/posegraph_ref.py) the way the float64 yardstick differs from the same
yardstick run with dtype=np.longdouble -- rounding inside the delta = 1e-9 central differences.  tests/test_posegraph_ref.py
measures the largest such differences d_t (m), d_q, d_s (relative), d_chi (relative) over CASES (at its = 20, and at its = 3 for
SCHEDULE) and asserts 10 d <= TOL <= 100 d; each constant is ten times the measured d, rounded up to one digit (the ten covers the
sqrt(2) of two noisy sides and device transcendentals an ulp off libm).  Measured: d_t 8.5e-6, d_q 7.4e-8, d_s 2.2e-8, d_chi 1.6e-5.
"""
import functools

from mc_slam_amd import synth

TOL_T = 9e-5
TOL_Q = 8e-7
TOL_S = 3e-7
TOL_CHI = 2e-4

_BUILD = {
    # two vertices, the drifted and the true relative pose as two edges between them (with one edge alone the cost ends at
    # exactly 0 and every decision is rounding); one side fixed each
    "TWO_I": lambda: synth.make_posegraph(11, 2, span=1, loops=[(1, 0)], fixed_at=1),
    "TWO_J": lambda: synth.make_posegraph(11, 2, span=1, loops=[(1, 0)], fixed_at=0),
    # chain of 12, one loop edge (1, 11): one long envelope row, fill along the whole chain
    "ARROW": lambda: synth.make_posegraph(12, 12, span=1, loops=[(1, 11)], fixed_at=0),
    # the same with the fixed vertex in the middle: the free numbering skips a vertex
    "MID": lambda: synth.make_posegraph(12, 12, span=1, loops=[(1, 11)], fixed_at=5),
    # 70 vertices (more rows than a wave has lanes), a bundle of loop edges, a duplicated edge, an isolated vertex (pivots of lambda)
    "BAND": lambda: synth.make_posegraph(13, 70, span=3, loops=[(i, j) for i in (66, 67, 68, 69) for j in (2, 3, 4)], fixed_at=0,
                                         dup_edge=40, isolated=True),
    # two loops, one inside the other, fixed scale: nested envelopes, zero scale columns
    "NEST": lambda: synth.make_posegraph(14, 130, span=2, loops=[(129, 1), (90, 40)], fixed_at=0, fix_scale=True),
    # the whole path once: span 6, a loop of 8 edges, 500 map points
    "BIG": lambda: synth.make_posegraph(15, 150, span=6, loops=[(149 - k, k) for k in range(8)], fixed_at=0, n_pt=500),
    # a loop measurement that is wrong by 2.5 rad: the first step and its nine retries are all rejected (found by a search over
    # seeds, shapes and loop rotation errors up to 2.5 rad; nu doubles at every rejection, so the tenth retry runs at lambda =
    # 1e-16 * 2^45 = 3.5e-3 and in most graphs of the search that one is accepted -- not in this one)
    "REJECT": lambda: synth.make_posegraph(0, 6, span=1, loops=[(5, 0)], fixed_at=0, loop_rot_err=2.5),
}

CASES = ["TWO_I", "TWO_J", "ARROW", "MID", "BAND", "NEST", "BIG"]     # result parity at its = 20
SCHEDULE = ["ARROW", "MID", "BAND", "NEST"]                           # schedule parity at its = 3


@functools.lru_cache(maxsize=None)
def _built(name):
    return _BUILD[name]()


def case(name, **changes):
    """a private copy of the named graph (the cached original is never handed out)"""
    return _built(name).copy(**changes)
