"""vba_search_by_bow (k_search_bow) against tests/search_bow_ref.py, the sequential loop, on a real MI355X.

The cases come from tests/search_bow_cases.py.  Every output is an integer (float32 appears in the ratio product and in the bin only,
both restated in np.float32), so state, match12, best_idx, best_dist, best_dist2, bin, match21, hist, ind, n_matches and
n_before_filter are compared for equality, for every keypoint of both sides: none is excused."""
import numpy as np
import pytest

import search_bow_cases as cases
import search_bow_ref as ref_mod
import search_proj_cases
from mc_slam_amd import abi, backend, synth

pytestmark = pytest.mark.gpu
NAMES = list(cases.cases())


@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0)
    yield b
    b.close()


def _same(a, b):
    """two results of the library, bit for bit"""
    assert (a.status, a.n_matches, a.n_before_filter, a.rounds) == (b.status, b.n_matches, b.n_before_filter, b.rounds)
    for k in cases.INTS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def test_against_the_yardstick(ba):
    """every case alone; prints the rounds in front of the assertions on them"""
    rounds = {}
    for name in NAMES:
        got = ba.search_by_bow([cases.cases()[name]])[0]
        cases.check_against(name, got, cases.ref(name))
        rounds[name] = got.rounds
    print("rounds:", rounds)
    assert 30 <= rounds["chain_40"] <= cases.CHAIN + 1 and 2 <= rounds["chain_8x5"] <= 6          # the node-local bound
    assert rounds["empty_keys1"] == 1 and rounds["empty_keys2"] == 1 and rounds["no_shared_node"] == 1
    assert max(rounds["crowd_frame"], rounds["crowd_kf"]) > 2                                    # the dependency was exercised


def test_one_ragged_call_equals_single_calls(ba):
    """all cases in one call, bit for bit, whatever the position in the batch, in both orders; one launch per call"""
    ps = [cases.cases()[n] for n in NAMES]
    single = [ba.search_by_bow([p])[0] for p in ps]
    for order in (list(range(len(ps))), list(reversed(range(len(ps))))):
        got = ba.search_by_bow([ps[i] for i in order])
        assert ba.get_profile()["kernel_launches"] == 1
        for i, g in zip(order, got):
            _same(g, single[i])
            cases.check_against(NAMES[i], g, cases.ref(NAMES[i]))
    assert ba.search_by_bow([]) == []
    assert single[NAMES.index("realistic_frame")].n_matches + single[NAMES.index("realistic_kf")].n_matches >= 500


def test_the_thresholds_are_the_callers(ba):
    """th_low = 0, nn_ratio = 0, nn_ratio = 1, a lower th_low, no orientation check: they change only what the yardstick says"""
    a, b = cases.cases()["crowd_frame"], cases.cases()["crowd_kf"]
    changed = [a.copy(th_low=0), a.copy(nn_ratio=0.0), a.copy(nn_ratio=1.0), a.copy(check_orientation=False), b.copy(th_low=0), b.copy(nn_ratio=0.0),
               b.copy(nn_ratio=1.0), b.copy(th_low=20), b.copy(nn_ratio=0.7)]
    got = ba.search_by_bow([a, b] + changed)
    assert got[0].n_matches > 20 and got[1].n_matches > 20
    for q, g in zip(changed, got[2:]):
        cases.check_against("changed", g, ref_mod.search_bow_ref(q))
    # nothing is below 0 * bestDist2; nothing passes `< 0`; without the filter nothing is dropped
    assert got[3].n_matches == 0 and set(got[3].state) <= {1, 2, 3, 4} and got[7].n_matches == 0 and got[6].n_matches == 0 and set(got[6].state) <= {1, 2, 3}
    assert got[5].n_matches == got[0].n_before_filter >= got[0].n_matches


def test_between_two_search_by_projection_calls(ba):
    """the call leaves the arena and the results of vba_search_by_projection on the same handle alone"""
    f = search_proj_cases.cases()["synth_small_local"]
    x = ba.search_by_projection([f])[0]
    cases.check_against("synth_small_kf", ba.search_by_bow([cases.cases()["synth_small_kf"]])[0], cases.ref("synth_small_kf"))
    y = ba.search_by_projection([f])[0]
    assert (x.status, x.n_matches, x.rounds) == (y.status, y.n_matches, y.rounds)
    for k in ("best_idx", "best_dist", "best_dist2", "level", "view_cos", "uv", "bin", "state", "key_match"):
        assert getattr(x, k).tobytes() == getattr(y, k).tobytes(), k
    search_proj_cases.check_against("synth_small_local", y, search_proj_cases.ref("synth_small_local"))


def test_refusals_and_pending_tickets(ba):
    fn, name = ba.lib.vba_search_by_bow, "vba_search_by_bow"
    p, m = cases.cases()["synth_small_frame"], cases.cases()["synth_small_kf"]
    i = p.node_id2.copy(); i[2] = i[1]
    f = p.node_feat2.copy(); f[3] = f[0]
    g = p.angle1.copy(); g[6] = 360.0
    x = m.node_feat1.copy(); x[7] = m.n_keys1
    big = synth.search_bow_scene(52, abi.SEARCH_BOW_KF_FRAME, n_keys1=4, n_keys2=abi.SEARCH_BOW_MAX_KEYS + 1, n_nodes=3, twins=0.0)
    for good, bad, msg in ((p, p.copy(node_id2=i), "pair 1: node_id of keyframe 2 is not strictly ascending at node 2"),
                           (p, p.copy(node_feat2=f), "pair 1: node_feat of keyframe 2 entry 3: keypoint %d listed twice" % f[0]),
                           (p, p.copy(angle1=g), "pair 1: keypoint 6 of keyframe 1: angle outside [0, 360)"),
                           (m, m.copy(node_feat1=x), "pair 1: node_feat of keyframe 1 entry 7: keypoint index out of range"),
                           (m, m.copy(nn_ratio=np.nan), "pair 1: nn_ratio is not finite"),
                           (m, m.copy(th_low=256), "pair 1: th_low outside 0 .. 255"),
                           (m, m.copy(mode=2), "pair 1: unknown mode"),
                           (m, m.copy(good_mp2=None), "pair 1: NULL array with n_keys2 > 0"),
                           (m, big, "pair 1: n_keys2 above 16384: the claim table of side 2 lives in LDS")):
        packed = ba.search_by_bow_pack([good, bad])
        assert fn(ba.h, packed[0], packed[3], packed[4]) != 0
        assert ba.lib.vba_last_error(ba.h).decode() == name + ": " + msg
        assert all(k.untouched() for k in packed[2])     # nothing was written
    packed = ba.search_by_bow_pack([p])
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
    cases.check_against("synth_small_frame", ba.search_by_bow([p])[0], cases.ref("synth_small_frame"))
