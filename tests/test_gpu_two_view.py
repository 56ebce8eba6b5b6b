"""vba_two_view_init (k_two_view) against tests/two_view_ref.py in float64, on a real MI355X.

The cases come from tests/two_view_cases.py; tests/test_two_view_ref.py asserts on the CPU that every 9-column A of every
hypothesis has a relative gap of at least 1e-6 between its two smallest singular values and that every comparison the yardstick
evaluates is at least 1e-9 away from its threshold, so every decision below is compared exactly: none is excused."""
import numpy as np
import pytest

import two_view_cases as cases
from test_two_view_ref import differences
from mc_slam_amd import abi, backend, synth

pytestmark = pytest.mark.gpu

# Ten times the largest float64-against-longdouble difference of the yardstick over all cases, rounded up to one digit
# (tests/test_two_view_ref.py::test_print_float64_against_longdouble prints hyp_score 1.066e-11, score 9.466e-13, rh 2.367e-13,
# HF 7.636e-13, parallax 1.337e-10, pose 1.801e-14, x3d 1.296e-12).  The kernel and the float64 yardstick are two FP64 evaluations
# of the same formulas (fused multiply-adds and other summation orders in the kernel), so each may differ from the exact value by
# about that much.  Scores are relative, H21 / F21 up to scale and sign, parallaxes in degrees, x3d relative to |x3d|.
TOL = dict(hyp_score=2e-10, score=1e-11, rh=3e-12, HF=8e-12, parallax=2e-9, pose=2e-13, x3d=2e-11)
EQUAL = ("status", "ok", "model", "reason", "best_hyp_h", "best_hyp_f", "n_inliers_h", "n_inliers_f", "n_rt", "best_rt")
FILL = 0xA5


@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0)
    yield b
    b.close()


def as_dict(g):
    return {k: getattr(g, k) for k in g.__dataclass_fields__}


def _same(a, b):
    """two results of the library, bit for bit"""
    for k in a.__dataclass_fields__:
        x, y = getattr(a, k), getattr(b, k)
        assert (x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else (x == y or (x != x and y != y)), k


@pytest.mark.parametrize("name", cases.IDS)
def test_against_the_yardstick(ba, name):
    p, r = cases.make(name), cases.reference(name)
    g = ba.two_view_init([p], fill=FILL)[0]
    assert ba.get_profile()["kernel_launches"] <= 2
    for k in EQUAL:
        assert getattr(g, k) == r[k], (k, getattr(g, k), r[k])
    assert np.array_equal(g.rt_good, r["rt_good"])
    assert np.array_equal(g.inlier_h, r["inlier_h"]) and np.array_equal(g.inlier_f, r["inlier_f"])
    got = as_dict(g)
    if not g.ok:   # R21, t21, x3d and triangulated are left untouched
        assert (g.x3d == float(FILL)).all() and (g.triangulated == FILL).all() and not g.R21.any() and not g.t21.any()
        got["x3d"] = got["triangulated"] = got["R21"] = got["t21"] = None
    else:
        assert np.array_equal(g.triangulated, r["triangulated"])
        untouched = np.ones(p.n_keys1, dtype=bool)
        untouched[p.match[r["rt"][r["best_rt"]]["state"] > 0, 0]] = False
        assert untouched.sum() > 30 and not g.x3d[untouched].any() and g.x3d[~untouched].all(axis=1).all()   # zeros exactly where no point was accepted
    d = differences(got, r)
    print(name, "GPU against the float64 yardstick:", {k: "%.2e" % v for k, v in d.items()})
    for k, v in d.items():
        assert v <= TOL[k], (k, v, TOL[k])


def _mixed_batch():
    """all cases: the n_hyp == 0 problem and the failing ones stand between the others"""
    return [cases.make(n) for n in cases.IDS]


def test_a_ragged_batch_equals_single_calls(ba):
    """bit for bit, whatever the position in the batch, in both orders"""
    batch = _mixed_batch()
    single = [ba.two_view_init([p], fill=FILL)[0] for p in batch]
    assert {s.reason for s in single} == {0, 1, 2, 3, 4, 5}
    for order in (list(range(len(batch))), list(reversed(range(len(batch))))):
        got = ba.two_view_init([batch[i] for i in order], fill=FILL)
        assert ba.get_profile()["kernel_launches"] <= 2
        for i, g in zip(order, got):
            _same(g, single[i])
    assert ba.two_view_init([]) == []


def test_without_score_arrays(ba):
    """hyp_score_* are optional: the rest of the answer is the same without them"""
    p = cases.make("general-63x15")
    a, b = ba.two_view_init([p])[0], ba.two_view_init([p], want_scores=False)[0]
    assert b.hyp_score_h is None and a.hyp_score_h.shape == (15,)
    b.hyp_score_h, b.hyp_score_f = a.hyp_score_h, a.hyp_score_f
    _same(a, b)
    assert a.score_h == a.hyp_score_h[a.best_hyp_h] and a.score_f == a.hyp_score_f[a.best_hyp_f]


def test_the_thresholds_are_the_callers(ba):
    p = cases.make("general-63x15")
    g = ba.two_view_init([p, p.copy(min_triangulated=60), p.copy(min_parallax=80.0), p.copy(sigma=0.01)])
    assert (g[0].ok, g[1].ok, g[1].reason, g[2].ok, g[2].reason) == (1, 0, 4, 0, 5)
    assert g[3].n_inliers_f < g[0].n_inliers_f and g[3].score_f < g[0].score_f


def test_refusals_and_pending_tickets(ba):
    p = cases.make("general-63x15")
    K0 = p.K.copy(); K0[1] = 0.0
    m = p.match.copy(); m[5, 0] = m[4, 0]
    m2 = p.match.copy(); m2[7, 1] = p.n_keys2
    s = p.sets.copy(); s[3, 2] = p.n_matches
    u = p.uv2.copy(); u[2, 1] = np.nan
    for bad, msg in ((p.copy(K=K0), "vba_two_view_init: pair 1: zero fx / fy"),
                     (p.copy(match=m), "vba_two_view_init: pair 1: match 5: repeated first index"),
                     (p.copy(match=m2), "vba_two_view_init: pair 1: match 7: index outside its frame"),
                     (p.copy(sets=s), "vba_two_view_init: pair 1: hypothesis 3: set index out of range"),
                     (p.copy(uv2=u), "vba_two_view_init: pair 1: keypoint 2 of frame 2: a pixel is not finite"),
                     (p.copy(match=p.match[:7]), "vba_two_view_init: pair 1: n_matches < 8 with n_hyp > 0"),
                     (p.copy(sigma=0.0), "vba_two_view_init: pair 1: zero sigma")):
        packed = ba.two_view_pack([p, bad], fill=FILL)
        rc = ba.lib.vba_two_view_init(ba.h, packed[0], packed[3], packed[4])
        assert rc == -1 and ba.lib.vba_last_error(ba.h).decode() == msg
        assert (packed[2][0].ih == FILL).all() and (packed[2][0].x == float(FILL)).all() and packed[2][0].s.model == 0   # before any launch
    w = synth.config_c3(seed=3, n_kf=6, n_pt=120, n_obs=500)
    t = ba.submit([w])
    packed = ba.two_view_pack([p], fill=FILL)
    rc = ba.lib.vba_two_view_init(ba.h, packed[0], packed[3], packed[4])
    err = ba.lib.vba_last_error(ba.h).decode()
    ba.wait(t)
    assert rc == -1 and "asynchronous batches pending" in err, (rc, err)
    assert (packed[2][0].ih == FILL).all()                      # nothing was written
    assert ba.two_view_init([p])[0].ok == 1
