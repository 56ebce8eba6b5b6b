"""vba_search_by_projection (k_search_proj) against tests/search_proj_ref.py, the sequential loop, in float64, on a real MI355X.

The cases come from tests/search_proj_cases.py; tests/test_search_proj_ref.py asserts on the CPU that every floating-point comparison
the yardstick evaluates has a relative margin of at least 1e-9, that every floor and ceil argument lies as far from an integer, and
that float64 and longdouble agree in every integer output.  So state, best_idx, best_dist, best_dist2, level, bin, key_match, hist,
ind, n_matches and n_before_filter are compared for equality, for every query and every keypoint: none is excused.  uv and view_cos
are compared within search_proj_cases.UV_TOL and COS_TOL, ten times the float64-against-longdouble difference."""
import numpy as np
import pytest

import fuse_cases
import search_proj_cases as cases
import search_proj_ref as ref_mod
from mc_slam_amd import abi, backend, synth

pytestmark = pytest.mark.gpu
NAMES = list(cases.cases())
REAL = ("uv", "view_cos")
INTS = ("best_idx", "best_dist", "best_dist2", "level", "bin", "state", "key_match", "hist", "ind")


@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0)
    yield b
    b.close()


def _same(a, b):
    """two results of the library, bit for bit"""
    assert (a.status, a.n_matches, a.n_before_filter, a.rounds) == (b.status, b.n_matches, b.n_before_filter, b.rounds)
    for k in INTS + REAL:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def test_against_the_yardstick(ba):
    """every case alone; prints the largest uv and view_cos differences and the rounds in front of the assertions on them"""
    worst_uv = worst_cos = 0.0
    rounds = {}
    for name in NAMES:
        got = ba.search_by_projection([cases.cases()[name]])[0]
        du, dc = cases.check_against(name, got, cases.ref(name), uv_tol=np.inf, cos_tol=np.inf)
        worst_uv, worst_cos = max(worst_uv, du), max(worst_cos, dc)
        rounds[name] = got.rounds
    print("largest |uv| difference GPU against the float64 yardstick: %.3e pixels (tolerance %.0e); |view_cos|: %.3e (tolerance %.0e)"
          % (worst_uv, cases.UV_TOL, worst_cos, cases.COS_TOL))
    print("rounds:", rounds)
    assert worst_uv <= cases.UV_TOL and worst_cos <= cases.COS_TOL
    assert rounds["chain_40"] <= cases.CHAIN + 1 and rounds["empty_q_last"] == 1 and rounds["empty_keys_local"] == 1
    assert max(rounds.values()) > 2            # the dependency was exercised


def test_one_ragged_call_equals_single_calls(ba):
    """all cases in one call, bit for bit, whatever the position in the batch, in both orders; one launch per call"""
    ps = [cases.cases()[n] for n in NAMES]
    single = [ba.search_by_projection([p])[0] for p in ps]
    for order in (list(range(len(ps))), list(reversed(range(len(ps))))):
        got = ba.search_by_projection([ps[i] for i in order])
        assert ba.get_profile()["kernel_launches"] == 1
        for i, g in zip(order, got):
            _same(g, single[i])
            cases.check_against(NAMES[i], g, cases.ref(NAMES[i]))
    assert ba.search_by_projection([]) == []
    assert sum(s.n_matches for s in single) >= 500


def test_the_thresholds_are_the_callers(ba):
    """th_high = 0, th = 0, cos_view = 2, nn_ratio = 0, a wider th, no orientation check: they change only what the yardstick says"""
    a, b = cases.cases()["crowd_last"], cases.cases()["crowd_local"]
    changed = [a.copy(th_high=0), a.copy(th=0.0), a.copy(th=30.0), a.copy(check_orientation=False), b.copy(th_high=0), b.copy(cos_view=2.0),
               b.copy(nn_ratio=0.0), b.copy(th=5.0), b.copy(nn_ratio=0.9)]
    got = ba.search_by_projection([a, b] + changed)
    assert got[0].n_matches > 20 and got[1].n_matches > 20
    for q, g in zip(changed, got[2:]):
        w = ref_mod.search_proj_ref(q)
        assert w["margin"] >= 1e-9 and w["margin_r"] >= 1e-9
        cases.check_against("changed", g, w)
    # a radius of 0 holds no keypoint; cos_view = 2 lets no point into the frustum; without the filter nothing is dropped
    assert got[3].n_matches == 0 and set(got[3].state) <= {1, 2, 3, 4} and set(got[7].state) <= {1, 2, 3, 4, 5}
    assert got[5].n_matches == got[0].n_before_filter > got[0].n_matches


def test_between_two_fuse_calls(ba):
    """the call leaves the arena and the results of vba_fuse on the same handle alone"""
    f = fuse_cases.cases()["synth_small"]
    x = ba.fuse([f])[0]
    cases.check_against("synth_small_local", ba.search_by_projection([cases.cases()["synth_small_local"]])[0], cases.ref("synth_small_local"))
    y = ba.fuse([f])[0]
    assert (x.status, x.n_found) == (y.status, y.n_found)
    for k in ("best_idx", "best_dist", "level", "uv", "state"):
        assert getattr(x, k).tobytes() == getattr(y, k).tobytes(), k
    fuse_cases.check_against("synth_small", y, fuse_cases.ref("synth_small"))


def test_refusals_and_pending_tickets(ba):
    fn, name = ba.lib.vba_search_by_projection, "vba_search_by_projection"
    p, m = cases.cases()["synth_small_last"], cases.cases()["synth_small_local"]
    o = p.q_oct.copy(); o[4] = 8
    f = p.cell_feat.copy(); f[3] = f[0]
    g = p.angle.copy(); g[6] = 360.0
    x = m.q_pos.copy(); x[7, 1] = np.inf
    big = synth.search_proj_scene(52, abi.SEARCH_PROJ_LOCAL_MAP, n_keys=abi.SEARCH_PROJ_MAX_KEYS + 1, n_q=4, twins=0.0)
    for good, bad, msg in ((p, p.copy(q_oct=o), "problem 1: query 4: octave >= n_levels"),
                           (p, p.copy(cell_feat=f), "problem 1: cell_feat entry 3: keypoint %d listed twice" % f[0]),
                           (p, p.copy(angle=g), "problem 1: keypoint 6: angle outside [0, 360)"),
                           (m, m.copy(q_pos=x), "problem 1: query 7: the position is not finite"),
                           (m, m.copy(th=np.nan), "problem 1: a threshold is not finite"),
                           (m, m.copy(th_high=257), "problem 1: th_high outside 0 .. 256"),
                           (m, m.copy(mode=2), "problem 1: unknown mode"),
                           (m, big, "problem 1: n_keys above 16384: the claim table of a frame lives in LDS")):
        packed = ba.search_by_projection_pack([good, bad])
        assert fn(ba.h, packed[0], packed[3], packed[4]) != 0
        assert ba.lib.vba_last_error(ba.h).decode() == name + ": " + msg
        assert all(k.untouched() for k in packed[2])     # nothing was written
    packed = ba.search_by_projection_pack([p])
    for n, pp, rr in ((-1, packed[3], packed[4]), (1, None, packed[4]), (1, packed[3], None)):
        assert fn(ba.h, n, pp, rr) != 0
        assert ba.lib.vba_last_error(ba.h).decode() == name + ": bad arguments"
    w = synth.config_c3(seed=3, n_kf=6, n_pt=120, n_obs=500)
    t = ba.submit([w])
    rc = fn(ba.h, packed[0], packed[3], packed[4])
    err = ba.lib.vba_last_error(ba.h).decode()
    ba.wait(t)
    assert rc == -1 and "asynchronous batches pending" in err, (rc, err)
    assert packed[2][0].untouched()     # nothing was written
    cases.check_against("synth_small_last", ba.search_by_projection([p])[0], cases.ref("synth_small_last"))
