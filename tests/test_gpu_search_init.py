"""vba_search_for_initialization (k_search_init) against tests/search_init_ref.py, the sequential loop, on a real MI355X.

The cases come from tests/search_init_cases.py.  Every decision is an integer one but the area, whose comparisons the yardstick keeps
at a relative margin of 1e-9 (tests/test_search_init_ref.py), so state, match12, best_idx, best_dist, best_dist2, bin, match21,
matched_dist, hist, ind, n_matches, n_before_filter and n_stolen are compared for equality, for every keypoint of both frames, none
excused, and prev_matched bit for bit."""
import numpy as np
import pytest

import fuse_cases
import search_init_cases as cases
import search_init_ref as ref_mod
import search_proj_cases
from mc_slam_amd import abi, backend, synth

pytestmark = pytest.mark.gpu
NAMES = list(cases.cases())
ARRAYS = ("match12", "best_idx", "best_dist", "best_dist2", "bin", "state", "prev_matched", "match21", "matched_dist", "hist", "ind")


@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0)
    yield b
    b.close()


def _same(a, b):
    """two results of the library, bit for bit"""
    assert (a.status, a.n_matches, a.n_before_filter, a.n_stolen, a.rounds) == (b.status, b.n_matches, b.n_before_filter, b.n_stolen, b.rounds)
    for k in ARRAYS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def test_against_the_yardstick(ba):
    """every case alone; prints the rounds in front of the assertions on them"""
    rounds = {}
    for name in NAMES:
        got = ba.search_for_initialization([cases.cases()[name]])[0]
        rounds[name] = got.rounds
        cases.check_against(name, got, cases.ref(name))
    print("rounds:", rounds)
    assert rounds["dep_chain_40"] == 41 and rounds["steal_chain_40"] == 2
    assert rounds["empty_keys1"] == 1 and rounds["empty_keys2"] == 1 and rounds["upper_levels_only"] == 1
    for name in NAMES:
        assert 1 <= rounds[name] <= cases.n_queries(cases.cases()[name]) + 1, name
    assert max(v for k, v in rounds.items() if k not in ("dep_chain_40", "steal_chain_40")) > 2     # the dependency was exercised elsewhere too


def test_one_ragged_call_equals_single_calls(ba):
    """all cases in one call, bit for bit, whatever the position in the batch, in both orders; one launch per call"""
    ps = [cases.cases()[n] for n in NAMES]
    single = [ba.search_for_initialization([p])[0] for p in ps]
    for order in (list(range(len(ps))), list(reversed(range(len(ps))))):
        got = ba.search_for_initialization([ps[i] for i in order])
        assert ba.get_profile()["kernel_launches"] == 1
        for i, g in zip(order, got):
            _same(g, single[i])
            cases.check_against(NAMES[i], g, cases.ref(NAMES[i]))
    assert ba.search_for_initialization([]) == []


def test_the_thresholds_are_the_callers(ba):
    """th_low = 0, windowSize 0 and negative, nn_ratio 1 and 0.1, the filter off: they change only what the yardstick says"""
    a, b = cases.cases()["crowd_0"], cases.cases()["stolen_in_hist"]
    changed = [a.copy(th_low=0), a.copy(window_size=0.0), a.copy(window_size=-30.0), a.copy(nn_ratio=1.0), a.copy(nn_ratio=0.1),
               a.copy(check_orientation=False), b.copy(check_orientation=False), b.copy(window_size=-5.0)]
    got = ba.search_for_initialization([a, b] + changed)
    assert got[0].n_matches > 20 and got[0].n_stolen > 0
    for q, g in zip(changed, got[2:]):
        cases.check_against("changed", g, ref_mod.search_init_ref(q))
    # a radius of 0 or below holds no keypoint; without the filter nothing is dropped
    for g in (got[3], got[4], got[9]):
        assert g.n_matches == 0 and set(g.state) <= {1, 2}
    assert got[7].n_matches == got[0].n_before_filter and got[8].n_matches == 9


def test_between_calls_of_the_siblings(ba):
    """the call leaves the arenas and the results of vba_search_by_projection and vba_fuse on the same handle alone"""
    f, u = search_proj_cases.cases()["synth_small_local"], fuse_cases.cases()["synth_small"]
    x, xf = ba.search_by_projection([f])[0], ba.fuse([u])[0]
    cases.check_against("crowd_1", ba.search_for_initialization([cases.cases()["crowd_1"]])[0], cases.ref("crowd_1"))
    y, yf = ba.search_by_projection([f])[0], ba.fuse([u])[0]
    assert (x.status, x.n_matches, x.rounds) == (y.status, y.n_matches, y.rounds)
    for k in ("best_idx", "best_dist", "best_dist2", "level", "view_cos", "uv", "bin", "state", "key_match"):
        assert getattr(x, k).tobytes() == getattr(y, k).tobytes(), k
    for k in ("best_idx", "best_dist", "level", "uv", "state"):
        assert getattr(xf, k).tobytes() == getattr(yf, k).tobytes(), k
    search_proj_cases.check_against("synth_small_local", y, search_proj_cases.ref("synth_small_local"))
    fuse_cases.check_against("synth_small", yf, fuse_cases.ref("synth_small"))


def test_refusals_and_pending_tickets(ba):
    fn, name = ba.lib.vba_search_for_initialization, "vba_search_for_initialization"
    p = cases.cases()["crowd_2"]
    f = p.cell_feat.copy(); f[3] = f[0]
    g = p.angle2.copy(); g[6] = 360.0
    m = p.prev_matched.copy(); m[4, 1] = np.nan
    u = p.uv2.copy(); u[5, 0] = np.inf
    cb = p.cell_begin.copy(); cb[0] = 1
    big = synth.search_init_scene(52, 4, abi.SEARCH_INIT_MAX_KEYS + 1, size=(80, 60), cols=8, rows=6, window_size=5.0, twins=0.0)
    for bad, msg in ((p.copy(cell_feat=f), "pair 1: cell_feat entry 3: keypoint %d listed twice" % f[0]),
                     (p.copy(angle2=g), "pair 1: keypoint 6 of frame 2: angle outside [0, 360)"),
                     (p.copy(prev_matched=m), "pair 1: keypoint 4 of frame 1: prev_matched is not finite"),
                     (p.copy(uv2=u), "pair 1: keypoint 5 of frame 2: a pixel is not finite"),
                     (p.copy(cell_begin=cb), "pair 1: cell_begin does not start at 0"),
                     (p.copy(nn_ratio=np.nan), "pair 1: a threshold is not finite"),
                     (p.copy(window_size=np.inf), "pair 1: a threshold is not finite"),
                     (p.copy(th_low=256), "pair 1: th_low outside 0 .. 255"),
                     (p.copy(grid_cols=0), "pair 1: grid size outside 1 .. 65536 cells"),
                     (p.copy(angle1=None), "pair 1: NULL array with n_keys1 > 0"),
                     (big, "pair 1: n_keys2 above 16384: the claimer lists of frame 2 live in LDS")):
        packed = ba.search_for_initialization_pack([p, bad])
        assert fn(ba.h, packed[0], packed[3], packed[4]) != 0
        assert ba.lib.vba_last_error(ba.h).decode() == name + ": " + msg
        assert all(k.untouched() for k in packed[2])     # nothing was written
    packed = ba.search_for_initialization_pack([p])
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
    cases.check_against("crowd_2", ba.search_for_initialization([p])[0], cases.ref("crowd_2"))
