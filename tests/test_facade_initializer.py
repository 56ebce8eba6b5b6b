"""Initializer::Initialize of the host facade (mc_slam_amd/host/Initializer.cpp) on a real MI355X, against tests/two_view_ref.py on
the sets the facade drew.  The module makes the only Initializers of its process: the first Initialize seeds rand() with 0, the
second continues the stream (DUtils::Random::SeedRandOnce), and so does the mirror of the draw in tests/facade_initializer_lib.py."""
import numpy as np
import pytest

import facade_initializer_lib as fi
import two_view_cases as cases
import two_view_ref as ref
from test_gpu_two_view import TOL

pytestmark = pytest.mark.gpu
F32 = 2.0 ** -24     # half a unit in the last place of a float32 of magnitude 1


@pytest.fixture(scope="module")
def runs():
    """two Initialize calls of one process, in order: a general scene (succeeds on F), then a short baseline (fails), then a plane
    through a second Initializer; with each the sets the mirror drew from the same stream"""
    pa, pb, pc = cases.make("general-300x200"), cases.make("short-256x15"), cases.make("plane-300x200")
    fi.seed_rand(0)
    mirror = [fi.draw_sets(p.n_matches) for p in (pa, pb, pc)]
    a = fi.Init(pa)
    out = [a.initialize(pa)]
    b = fi.Init(pb)
    out.append(b.initialize(pb))
    c = fi.Init(pc)
    out.append(c.initialize(pc))
    for i in (a, b, c):
        i.close()
    return (pa, pb, pc), mirror, out


def test_the_draw_continues_the_rand_stream(runs):
    ps, mirror, out = runs
    for p, m, o in zip(ps, mirror, out):
        assert np.array_equal(o["sets"], m)
        assert all(len(set(s)) == 8 for s in o["sets"].tolist()) and o["sets"].max() < p.n_matches
    assert not np.array_equal(mirror[0], mirror[2])     # same N = 300, later in the stream


def test_against_the_yardstick_on_the_facades_sets(runs):
    ps, _, out = runs
    rets = []
    for p, o in zip(ps, out):
        q = p.copy(sets=o["sets"])
        r = ref.two_view(q)
        small = {k: v for k, v in r["margins"].items() if not v >= 1e-9}
        assert not small and min(r["gap_h"].min(), r["gap_f"].min()) >= 1e-6, small      # the comparison below excuses nothing
        assert o["ret"] == r["ok"] and o["info"]["n_matches"] == p.n_matches
        for k in ("ok", "model", "reason", "best_hyp_h", "best_hyp_f", "n_inliers_h", "n_inliers_f", "n_rt", "best_rt"):
            assert o["info"][k] == r[k], k
        rets.append(o["ret"])
        if not r["ok"]:   # nothing was written
            assert (o["R21"] == 7).all() and (o["t21"] == 7).all() and (o["vP3D"] == 7).all() and (o["vbTriangulated"] == 7).all()
            continue
        assert np.array_equal(o["vbTriangulated"], r["triangulated"])
        dR = max(np.abs(o["R21"] - r["R21"]).max(), np.abs(o["t21"] - r["t21"]).max())
        nz = np.linalg.norm(r["x3d"], axis=1) > 0
        assert not o["vP3D"][~nz].any()
        dx = (np.linalg.norm(o["vP3D"][nz] - r["x3d"][nz], axis=1) / np.linalg.norm(r["x3d"][nz], axis=1)).max()
        print("R21 | t21 %.2e  vP3D %.2e (float32 results against the float64 yardstick)" % (dR, dx))
        assert dR <= TOL["pose"] + F32                   # float32 rounding of entries of magnitude <= 1
        assert dx <= TOL["x3d"] + np.sqrt(3) * F32       # float32 rounding of every coordinate, relative to |x|
    assert rets == [1, 0, 1]
