"""vba_search_by_sim3 (k_search_sim3) against tests/search_sim3_ref.py in float64, on a real MI355X.

The cases come from tests/search_sim3_cases.py; tests/test_search_sim3_ref.py asserts on the CPU that every floating-point comparison
the yardstick evaluates has a relative margin of at least 1e-9, that every floor and ceil argument lies as far from an integer, and
that float64 and longdouble agree in every output.  So match1 / 2, best_dist1 / 2, level1 / 2, state1 / 2, match12 and n_found are
compared for equality and for every keypoint: none is excused.  The entry point returns no floating-point value."""
import numpy as np
import pytest

import fuse_cases
import search_sim3_cases as cases
import search_sim3_ref as ref_mod
from mc_slam_amd import backend, synth

pytestmark = pytest.mark.gpu
NAMES = list(cases.cases())
ARRAYS = ref_mod.INT_KEYS[1:]


@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0)
    yield b
    b.close()


def _same(a, b):
    """two results of the library, bit for bit"""
    assert (a.status, a.n_found) == (b.status, b.n_found)
    for k in ARRAYS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def test_against_the_yardstick(ba):
    """every case alone"""
    for name in NAMES:
        cases.check_against(name, ba.search_by_sim3([cases.cases()[name]])[0], cases.ref(name))
        launches = ba.get_profile()["kernel_launches"]
        assert launches == (0 if name == "nothing_searchable" else 1), name   # a call without queries launches nothing and writes everything


def test_one_ragged_call_equals_single_calls(ba):
    """all cases in one call, bit for bit, whatever the position in the batch, in both orders; one launch per call"""
    ps = [cases.cases()[n] for n in NAMES]
    single = [ba.search_by_sim3([p])[0] for p in ps]
    for order in (list(range(len(ps))), list(reversed(range(len(ps))))):
        got = ba.search_by_sim3([ps[i] for i in order])
        assert ba.get_profile()["kernel_launches"] == 1
        for i, g in zip(order, got):
            _same(g, single[i])
            cases.check_against(NAMES[i], g, cases.ref(NAMES[i]))
    assert ba.search_by_sim3([]) == []
    assert sum(s.n_found for s in single) >= 500


def test_the_thresholds_are_the_callers(ba):
    """th_high = 0 and th = 0 change only what the yardstick says"""
    p = cases.cases()["synth_small"]
    changed = [p.copy(th_high=0), p.copy(th=0.0)]
    got = ba.search_by_sim3([p] + changed)
    assert got[0].n_found > 20
    for q, g in zip(changed, got[1:]):
        w = ref_mod.search_sim3_ref(q)
        assert w["margin"] >= 1e-9 and w["margin_r"] >= 1e-9
        cases.check_against("changed", g, w)
        assert g.n_found == 0
    assert 8 in set(got[1].state1) and 0 not in set(got[1].state1) and np.array_equal(got[1].level1, got[0].level1)
    assert set(got[2].state1) <= {1, 2, 3, 4, 5, 6, 7} and set(got[2].state2) <= {1, 2, 3, 4, 5, 6, 7}


def test_between_two_fuse_calls(ba):
    """the call leaves the arena and the results of vba_fuse on the same handle alone"""
    f = fuse_cases.cases()["synth_small"]
    a = ba.fuse([f])[0]
    cases.check_against("synth_small", ba.search_by_sim3([cases.cases()["synth_small"]])[0], cases.ref("synth_small"))
    b = ba.fuse([f])[0]
    assert (a.status, a.n_found) == (b.status, b.n_found)
    for k in ("best_idx", "best_dist", "level", "uv", "state"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    fuse_cases.check_against("fuse synth_small", b, fuse_cases.ref("synth_small"))


def test_refusals_and_pending_tickets(ba):
    p = cases.cases()["synth_small"]
    o = p.kf2.oct.copy(); o[4] = 6
    f = p.kf1.cell_feat.copy(); f[3] = f[0]
    b = p.kf2.cell_begin.copy(); b[-1] = p.kf2.n_keys + 1
    i = int(np.nonzero(p.kf1.has_pt)[0][2])
    x = p.kf1.pos.copy(); x[i, 1] = np.inf
    d = p.kf2.pred_max.copy(); d[int(np.nonzero(p.kf2.has_pt)[0][1])] = np.nan
    R = p.R12.copy(); R[1, 1] = np.nan
    for bad, msg in ((p.copy(kf2=dict(oct=o)), "pair 1: keyframe 2: keypoint 4: octave >= n_levels"),
                     (p.copy(kf1=dict(cell_feat=f)), "pair 1: keyframe 1: cell_feat entry 3: keypoint %d listed twice" % f[0]),
                     (p.copy(kf2=dict(cell_begin=b)), "pair 1: keyframe 2: cell_begin ends above n_keys"),
                     (p.copy(kf1=dict(pos=x)), "pair 1: keyframe 1: keypoint %d: the position is not finite" % i),
                     (p.copy(kf2=dict(pred_max=d)), "pair 1: keyframe 2: keypoint %d: a distance is not finite" % int(np.nonzero(p.kf2.has_pt)[0][1])),
                     (p.copy(s12=0.0), "pair 1: s12 is not finite or not positive"),
                     (p.copy(s12=np.inf), "pair 1: s12 is not finite or not positive"),
                     (p.copy(R12=R), "pair 1: the Sim3 is not finite"),
                     (p.copy(th=np.nan), "pair 1: a threshold is not finite"),
                     (p.copy(th_high=257), "pair 1: th_high outside 0 .. 256")):
        packed = ba.search_by_sim3_pack([p, bad])
        assert ba.lib.vba_search_by_sim3(ba.h, packed[0], packed[3], packed[4]) != 0
        assert ba.lib.vba_last_error(ba.h).decode() == "vba_search_by_sim3: " + msg
        assert all(k.untouched() for k in packed[2])                             # nothing was written
    packed = ba.search_by_sim3_pack([p])
    for n, pp, rr in ((-1, packed[3], packed[4]), (1, None, packed[4]), (1, packed[3], None)):
        assert ba.lib.vba_search_by_sim3(ba.h, n, pp, rr) != 0
        assert ba.lib.vba_last_error(ba.h).decode() == "vba_search_by_sim3: bad arguments"
    # a position that is not finite under a keypoint WITHOUT a usable point is never read
    j = int(np.nonzero(p.kf1.has_pt == 0)[0][0])
    y = p.kf1.pos.copy(); y[j] = np.nan
    cases.check_against("nan where has_pt is 0", ba.search_by_sim3([p.copy(kf1=dict(pos=y))])[0], cases.ref("synth_small"))
    w = synth.config_c3(seed=3, n_kf=6, n_pt=120, n_obs=500)
    t = ba.submit([w])
    rc = ba.lib.vba_search_by_sim3(ba.h, packed[0], packed[3], packed[4])
    err = ba.lib.vba_last_error(ba.h).decode()
    ba.wait(t)
    assert rc == -1 and "asynchronous batches pending" in err, (rc, err)
    assert packed[2][0].untouched()                                              # nothing was written
    cases.check_against("synth_small", ba.search_by_sim3([p])[0], cases.ref("synth_small"))
