"""vba_fuse (k_fuse) against tests/fuse_ref.py in float64, on a real MI355X.

The cases come from tests/fuse_cases.py; tests/test_fuse_ref.py asserts on the CPU that every floating-point comparison the yardstick
evaluates has a relative margin of at least 1e-9, that every floor and ceil argument lies as far from an integer, and that float64
and longdouble agree in every integer output.  So state, best_idx, best_dist, level and n_found are compared for equality and for
every point: none is excused.  uv is compared within fuse_cases.UV_TOL, ten times the float64-against-longdouble difference."""
import numpy as np
import pytest

import fuse_cases as cases
import fuse_ref as ref_mod
import triangulate_cases
from mc_slam_amd import backend, synth

pytestmark = pytest.mark.gpu
NAMES = list(cases.cases())


@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0)
    yield b
    b.close()


def _same(a, b):
    """two results of the library, bit for bit"""
    assert (a.status, a.n_found) == (b.status, b.n_found)
    for k in ("best_idx", "best_dist", "level", "uv", "state"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def test_against_the_yardstick(ba):
    """every case alone; prints the largest uv difference in front of the assertion on it"""
    worst = 0.0
    for name in NAMES:
        worst = max(worst, cases.check_against(name, ba.fuse([cases.cases()[name]])[0], cases.ref(name), tol=np.inf))
    print("largest |uv| difference GPU against the float64 yardstick: %.3e pixels (tolerance %.0e)" % (worst, cases.UV_TOL))
    assert worst <= cases.UV_TOL


def test_one_ragged_call_equals_single_calls(ba):
    """all cases in one call, bit for bit, whatever the position in the batch, in both orders; one launch per call"""
    ps = [cases.cases()[n] for n in NAMES]
    single = [ba.fuse([p])[0] for p in ps]
    for order in (list(range(len(ps))), list(reversed(range(len(ps))))):
        got = ba.fuse([ps[i] for i in order])
        assert ba.get_profile()["kernel_launches"] == 1
        for i, g in zip(order, got):
            _same(g, single[i])
            cases.check_against(NAMES[i], g, cases.ref(NAMES[i]))
    assert ba.fuse([]) == []
    assert sum(s.n_found for s in single) >= 500


def test_the_thresholds_are_the_callers(ba):
    """th_low = 0, chi2_reproj = 0, th = 0 or cos_view = 2 change only what the yardstick says"""
    p = cases.cases()["synth_small"]
    changed = [p.copy(th_low=0), p.copy(chi2_reproj=0.0), p.copy(th=0.0), p.copy(cos_view=2.0)]
    got = ba.fuse([p] + changed)
    assert got[0].n_found > 20
    for q, g in zip(changed, got[1:]):
        w = ref_mod.fuse_ref(q)
        assert w["margin"] >= 1e-9 and w["margin_r"] >= 1e-9
        cases.check_against("changed", g, w)
        assert g.n_found == 0
    assert set(got[3].state) <= {1, 2, 3, 4, 5, 6, 7} and set(got[4].state) <= {1, 2, 3, 4, 5}


def test_between_two_triangulate_calls(ba):
    """the call leaves the arena and the results of vba_triangulate on the same handle alone"""
    t = triangulate_cases.make(triangulate_cases.CASES[2])
    a = ba.triangulate([t])[0]
    cases.check_against("synth_small", ba.fuse([cases.cases()["synth_small"]])[0], cases.ref("synth_small"))
    b = ba.triangulate([t])[0]
    assert (a.status, a.n_accepted) == (b.status, b.n_accepted) and a.x3d.tobytes() == b.x3d.tobytes() and a.reason.tobytes() == b.reason.tobytes()


def test_refusals_and_pending_tickets(ba):
    p = cases.cases()["synth_small"]
    o = p.oct.copy(); o[4] = 8
    f = p.cell_feat.copy(); f[3] = f[0]
    b = p.cell_begin.copy(); b[-1] = p.n_keys + 1
    x = p.pos.copy(); x[7, 1] = np.inf
    for bad, msg in ((p.copy(oct=o), "vba_fuse: problem 1: keypoint 4: octave >= n_levels"),
                     (p.copy(cell_feat=f), "vba_fuse: problem 1: cell_feat entry 3: keypoint %d listed twice" % f[0]),
                     (p.copy(cell_begin=b), "vba_fuse: problem 1: cell_begin ends above n_keys"),
                     (p.copy(pos=x), "vba_fuse: problem 1: point 7: the position is not finite"),
                     (p.copy(th=np.nan), "vba_fuse: problem 1: a threshold is not finite"),
                     (p.copy(th_low=257), "vba_fuse: problem 1: th_low outside 0 .. 256")):
        packed = ba.fuse_pack([p, bad])
        assert ba.lib.vba_fuse(ba.h, packed[0], packed[3], packed[4]) != 0
        assert ba.lib.vba_last_error(ba.h).decode() == msg
        assert all((k.st == 255).all() and (k.bi == -7).all() and k.s.n_found == -7 for k in packed[2])     # nothing was written
    packed = ba.fuse_pack([p])
    for n, pp, rr in ((-1, packed[3], packed[4]), (1, None, packed[4]), (1, packed[3], None)):
        assert ba.lib.vba_fuse(ba.h, n, pp, rr) != 0
        assert ba.lib.vba_last_error(ba.h).decode() == "vba_fuse: bad arguments"
    w = synth.config_c3(seed=3, n_kf=6, n_pt=120, n_obs=500)
    t = ba.submit([w])
    rc = ba.lib.vba_fuse(ba.h, packed[0], packed[3], packed[4])
    err = ba.lib.vba_last_error(ba.h).decode()
    ba.wait(t)
    assert rc == -1 and "asynchronous batches pending" in err, (rc, err)
    assert (packed[2][0].st == 255).all() and (packed[2][0].uv == -7.0).all() and packed[2][0].s.n_found == -7     # nothing was written
    cases.check_against("synth_small", ba.fuse([p])[0], cases.ref("synth_small"))
