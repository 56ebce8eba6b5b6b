"""The seeded cases of the vba_two_view_init tests in one place: (name, seed, arguments of synth.make_two_view).  n_matches walks the
wave and workgroup boundaries of the kernel (lanes stride over the matches in chunks of 64, a workgroup has 256 lanes): 8, 9, 63,
64, 65, 255, 256, 257, 300; n_hyp walks the sixteen-jobs-per-pass boundary of the fitting phase: 1, 15, 16, 17, 200, and 0.  Both
frames have more keypoints than matches (37 / 53 more).  What a case is there for stands beside it; that it does end that way,
and the margins the GPU comparison rests on, is asserted in tests/test_two_view_ref.py."""
import functools

from mc_slam_amd import synth

# expect: (ok, model, reason)
CASES = [
    ("general-300x200", 1, dict(n_matches=300, n_hyp=200, kind="general", far_frac=0.1), (1, 2, 0)),       # F; far points counted, not flagged
    ("plane-300x200", 1, dict(n_matches=300, n_hyp=200, kind="plane", baseline=1.0), (1, 1, 0)),           # H
    ("wrong30-300x200", 1, dict(n_matches=300, n_hyp=200, kind="general", outlier_frac=0.3), (1, 2, 0)),   # 30 % wrong matches
    ("rotation-257x16", 1, dict(n_matches=257, n_hyp=16, kind="rotation"), (0, 1, 3)),                     # pure rotation: :822 fails
    ("rotation-quiet-257x16", 3, dict(n_matches=257, n_hyp=16, kind="rotation", noise=0.002), (0, 1, 2)),  # pure rotation: d1 / d2 = 1
    ("short-256x15", 1, dict(n_matches=256, n_hyp=15, kind="general", baseline=0.08), (0, 2, 5)),          # short baseline: parallax
    ("shorter-256x15", 1, dict(n_matches=256, n_hyp=15, kind="general", baseline=0.04), (0, 1, 3)),        # shorter: H, :822 fails
    ("eight-8x1", 2, dict(n_matches=8, n_hyp=1, kind="general", min_triangulated=5), (0, 2, 4)),
    ("nine-9x1", 1, dict(n_matches=9, n_hyp=1, kind="general", min_triangulated=5, noise=0.05), (1, 2, 0)),  # nGood = 9: min(50, size - 1)
    ("general-63x15", 1, dict(n_matches=63, n_hyp=15, kind="general", min_triangulated=40), (1, 2, 0)),    # nGood = 57: element 50
    ("plane-64x16", 1, dict(n_matches=64, n_hyp=16, kind="plane", baseline=1.0, min_triangulated=40), (1, 1, 0)),
    ("wrong30-65x17", 1, dict(n_matches=65, n_hyp=17, kind="general", outlier_frac=0.3), (0, 2, 4)),       # maxGood < nMinGood
    ("far30-255x200", 1, dict(n_matches=255, n_hyp=200, kind="general", far_frac=0.3), (1, 2, 0)),         # 75 points with cos >= 0.99998
    ("nohyp-64x0", 1, dict(n_matches=64, n_hyp=0, kind="general"), (0, 2, 1)),                             # no hypothesis at all
]
IDS = [c[0] for c in CASES]
NAMES = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def make(name):
    """the abi.TwoViewProblem of a case (shared between the tests: treat it as read-only)"""
    _, seed, kw, _ = NAMES[name]
    return synth.make_two_view(seed, **kw)


@functools.lru_cache(maxsize=None)
def reference(name, dtype_name="float64", flip=False):
    """the yardstick's answer for a case, computed once per dtype and convention"""
    import numpy as np
    import two_view_ref as ref
    return ref.two_view(make(name), getattr(np, dtype_name), flip)
