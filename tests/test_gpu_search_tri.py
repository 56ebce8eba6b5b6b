"""vba_search_triangulation (k_search_tri) against tests/search_tri_ref.py in float64, on a real MI355X.

The cases come from tests/search_tri_cases.py; tests/test_search_tri_ref.py asserts on the CPU that every floating-point comparison
the yardstick evaluates has a relative margin of at least 1e-9 and that float64 and longdouble agree in every output, so every
output below is compared for equality and for every keypoint: none is excused."""
import numpy as np
import pytest

import search_tri_cases as cases
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
    assert (a.status, a.n_matches, a.n_before_filter) == (b.status, b.n_matches, b.n_before_filter)
    for k in ("hist", "ind", "match12", "best_dist", "state", "pairs"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


@pytest.mark.parametrize("name", NAMES)
def test_against_the_yardstick(ba, name):
    cases.check_against(name, ba.search_triangulation([cases.cases()[name]])[0], cases.ref(name))


def test_one_ragged_call_equals_single_calls(ba):
    """all cases in one call, bit for bit, whatever the position in the batch, in both orders; one launch per call"""
    ps = [cases.cases()[n] for n in NAMES]
    single = [ba.search_triangulation([p])[0] for p in ps]
    for order in (list(range(len(ps))), list(reversed(range(len(ps))))):
        got = ba.search_triangulation([ps[i] for i in order])
        assert ba.get_profile()["kernel_launches"] == 1
        for i, g in zip(order, got):
            _same(g, single[i])
            cases.check_against(NAMES[i], g, cases.ref(NAMES[i]))
    assert ba.search_triangulation([]) == []
    assert sum(s.n_matches for s in single) > 500


def test_check_orientation_toggled(ba):
    """the toggled pair changes only what the yardstick says"""
    got = ba.search_triangulation([cases.toggled(cases.cases()[n]) for n in NAMES])
    for n, g in zip(NAMES, got):
        cases.check_against(n + " toggled", g, cases.ref(n, toggle=True))


def test_the_thresholds_are_the_callers(ba):
    p = cases.cases()["synth_mid"]
    g = ba.search_triangulation([p, p.copy(th_low=0), p.copy(chi2_epi=0.0), p.copy(epipole_r2=1e12), p.copy(level_sigma2_2=p.level_sigma2_2 * 0)])
    assert g[0].n_before_filter > 50
    for k in (1, 2, 3, 4):
        assert g[k].n_before_filter == 0 and set(g[k].state) <= {1, 2, 3}


def test_between_two_triangulate_calls(ba):
    """the call leaves the arena and the results of vba_triangulate on the same handle alone"""
    t = triangulate_cases.make(triangulate_cases.CASES[2])
    a = ba.triangulate([t])[0]
    cases.check_against("synth_small", ba.search_triangulation([cases.cases()["synth_small"]])[0], cases.ref("synth_small"))
    b = ba.triangulate([t])[0]
    assert (a.status, a.n_accepted) == (b.status, b.n_accepted) and a.x3d.tobytes() == b.x3d.tobytes() and a.reason.tobytes() == b.reason.tobytes()


def test_refusals_and_pending_tickets(ba):
    p = cases.cases()["synth_small"]
    o = p.oct2.copy(); o[4] = 8
    f = p.node_feat1.copy(); f[3] = f[0]
    for bad, msg in ((p.copy(oct2=o), "vba_search_triangulation: pair 1: keypoint 4 of keyframe 2: octave >= n_levels2"),
                     (p.copy(node_feat1=f), "vba_search_triangulation: pair 1: node_feat of keyframe 1 entry 3: keypoint %d listed twice" % f[0]),
                     (p.copy(epipole=np.array([np.nan, 0])), "vba_search_triangulation: pair 1: the epipole is not finite"),
                     (p.copy(th_low=300), "vba_search_triangulation: pair 1: th_low outside 0 .. 255")):
        with pytest.raises(RuntimeError, match=msg):
            ba.search_triangulation([p, bad])
    packed = ba.search_triangulation_pack([p])
    for n, pp, rr in ((-1, packed[3], packed[4]), (1, None, packed[4]), (1, packed[3], None)):
        assert ba.lib.vba_search_triangulation(ba.h, n, pp, rr) != 0
        assert ba.lib.vba_last_error(ba.h).decode() == "vba_search_triangulation: bad arguments"
    assert (packed[2][0].st == 255).all()
    w = synth.config_c3(seed=3, n_kf=6, n_pt=120, n_obs=500)
    t = ba.submit([w])
    rc = ba.lib.vba_search_triangulation(ba.h, packed[0], packed[3], packed[4])
    err = ba.lib.vba_last_error(ba.h).decode()
    ba.wait(t)
    assert rc == -1 and "asynchronous batches pending" in err, (rc, err)
    assert (packed[2][0].st == 255).all()                      # nothing was written
    cases.check_against("synth_small", ba.search_triangulation([p])[0], cases.ref("synth_small"))
