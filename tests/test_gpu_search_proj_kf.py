"""vba_search_by_projection_kf (k_search_proj_kf) against tests/search_proj_kf_ref.py, the sequential loop, in float64, on a real MI355X.

The cases come from tests/search_proj_kf_cases.py; tests/test_search_proj_kf_ref.py asserts on the CPU that every floating-point
comparison the yardstick evaluates has a relative margin of at least 1e-9, that every floor and ceil argument lies as far from an
integer, and that float64 and longdouble agree in every integer output.  So state, best_idx, best_dist, level, bin, key_match, hist,
ind, n_matches and n_before_filter are compared for equality, for every query and every keypoint: none is excused.  uv is compared
within search_proj_kf_cases.UV_TOL, ten times the float64-against-longdouble difference."""
import numpy as np
import pytest

import fuse_cases
import search_proj_cases
import search_proj_kf_cases as cases
import search_proj_kf_ref as ref_mod
from mc_slam_amd import abi, backend, synth

pytestmark = pytest.mark.gpu
NAMES = list(cases.cases())
INTS = ("best_idx", "best_dist", "level", "bin", "state", "key_match", "hist", "ind")


@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0)
    yield b
    b.close()


def _same(a, b, keys=INTS + ("uv",), scalars=("status", "n_matches", "n_before_filter", "rounds")):
    """two results of the library, bit for bit"""
    assert [getattr(a, k) for k in scalars] == [getattr(b, k) for k in scalars]
    for k in keys:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def test_against_the_yardstick(ba):
    """every case alone; prints the largest uv difference and the rounds in front of the assertions on them"""
    worst_uv = 0.0
    rounds = {}
    for name in NAMES:
        got = ba.search_by_projection_kf([cases.cases()[name]])[0]
        worst_uv = max(worst_uv, cases.check_against(name, got, cases.ref(name), uv_tol=np.inf))
        rounds[name] = got.rounds
    print("largest |uv| difference GPU against the float64 yardstick: %.3e pixels (tolerance %.0e)" % (worst_uv, cases.UV_TOL))
    print("rounds:", rounds)
    assert worst_uv <= cases.UV_TOL
    assert rounds["chain_40"] == cases.CHAIN + 1 and rounds["chain_40_reloc"] == cases.CHAIN + 1
    assert rounds["empty_q_loop"] == 1 and rounds["empty_keys_reloc"] == 1
    assert max(v for k, v in rounds.items() if not k.startswith("chain_40")) > 2      # the dependency was exercised elsewhere too


def test_one_ragged_call_equals_single_calls(ba):
    """all cases in one call, both modes mixed, bit for bit, whatever the position in the batch, in both orders; one launch per call"""
    ps = [cases.cases()[n] for n in NAMES]
    single = [ba.search_by_projection_kf([p])[0] for p in ps]
    for order in (list(range(len(ps))), list(reversed(range(len(ps))))):
        got = ba.search_by_projection_kf([ps[i] for i in order])
        assert ba.get_profile()["kernel_launches"] == 1
        for i, g in zip(order, got):
            _same(g, single[i])
            cases.check_against(NAMES[i], g, cases.ref(NAMES[i]))
    assert ba.search_by_projection_kf([]) == []
    assert sum(s.n_matches for s in single) >= 500


def test_the_thresholds_are_the_callers(ba):
    """th_dist = 0, th = 0, cos_view = 2, a wider th, the relocalisation pair (3, 64), the filter off: they change only what the
    yardstick says"""
    a, b = cases.cases()["crowd_loop"], cases.cases()["crowd_reloc"]
    changed = [a.copy(th_dist=0), a.copy(th=0.0), a.copy(cos_view=2.0), a.copy(th=30.0), b.copy(th_dist=0), b.copy(th=0.0), b.copy(th=30.0),
               b.copy(th=3.0, th_dist=64), b.copy(check_orientation=False)]
    got = ba.search_by_projection_kf([a, b] + changed)
    assert got[0].n_matches > 20 and got[1].n_matches > 20
    for q, g in zip(changed, got[2:]):
        w = ref_mod.search_proj_kf_ref(q)
        assert w["margin"] >= 1e-9 and w["margin_r"] >= 1e-9
        cases.check_against("changed", g, w)
    # a radius of 0 holds no keypoint; cos_view = 2 lets no point past the viewing-angle gate; without the filter nothing is dropped
    assert got[3].n_matches == 0 and set(got[3].state) <= {1, 2, 3, 4, 5, 6, 7} and got[7].n_matches == 0 and set(got[7].state) <= {1, 2, 3, 4, 5}
    assert got[4].n_matches == 0 and set(got[4].state) <= {1, 2, 3, 4, 5}
    assert got[10].n_matches == got[1].n_before_filter > got[1].n_matches


def test_between_fuse_and_search_by_projection_calls(ba):
    """the call leaves the arenas and the results of vba_fuse and vba_search_by_projection on the same handle alone"""
    f = fuse_cases.cases()["synth_small"]
    s = search_proj_cases.cases()["synth_small_local"]
    x, sx = ba.fuse([f])[0], ba.search_by_projection([s])[0]
    for name in ("synth_small_loop", "synth_small_reloc"):
        cases.check_against(name, ba.search_by_projection_kf([cases.cases()[name]])[0], cases.ref(name))
    y, sy = ba.fuse([f])[0], ba.search_by_projection([s])[0]
    _same(x, y, keys=("best_idx", "best_dist", "level", "uv", "state"), scalars=("status", "n_found"))
    _same(sx, sy, keys=("best_idx", "best_dist", "best_dist2", "level", "view_cos", "uv", "bin", "state", "key_match", "hist", "ind"))
    fuse_cases.check_against("synth_small", y, fuse_cases.ref("synth_small"))
    search_proj_cases.check_against("synth_small_local", sy, search_proj_cases.ref("synth_small_local"))


def test_refusals_and_pending_tickets(ba):
    fn, name = ba.lib.vba_search_by_projection_kf, "vba_search_by_projection_kf"
    p, m = cases.cases()["synth_small_reloc"], cases.cases()["synth_small_loop"]
    o = p.oct.copy(); o[4] = 8
    f = p.cell_feat.copy(); f[3] = f[0]
    g = p.angle.copy(); g[6] = 360.0
    h = p.q_angle.copy(); h[5] = -1.0
    x = m.q_pos.copy(); x[7, 1] = np.inf
    nr = m.q_normal.copy(); nr[2, 0] = np.nan
    big = synth.search_proj_kf_scene(52, cases.LOOP, n_keys=abi.SEARCH_PROJ_KF_MAX_KEYS + 1, n_q=4, twins=0.0)
    for good, bad, msg in ((p, p.copy(oct=o), "problem 1: keypoint 4: octave >= n_levels"),
                           (p, p.copy(cell_feat=f), "problem 1: cell_feat entry 3: keypoint %d listed twice" % f[0]),
                           (p, p.copy(angle=g), "problem 1: keypoint 6: angle outside [0, 360)"),
                           (p, p.copy(q_angle=h), "problem 1: query 5: angle outside [0, 360)"),
                           (m, m.copy(q_pos=x), "problem 1: query 7: the position is not finite"),
                           (m, m.copy(q_normal=nr), "problem 1: query 2: the normal is not finite"),
                           (m, m.copy(th=np.nan), "problem 1: a threshold is not finite"),
                           (m, m.copy(cos_view=np.inf), "problem 1: a threshold is not finite"),
                           (m, m.copy(th_dist=257), "problem 1: th_dist outside 0 .. 256"),
                           (p, p.copy(th_dist=-1), "problem 1: th_dist outside 0 .. 256"),
                           (m, m.copy(mode=2), "problem 1: unknown mode"),
                           (m, big, "problem 1: n_keys above 16384: the claim table of a target lives in LDS")):
        packed = ba.search_by_projection_kf_pack([good, bad])
        assert fn(ba.h, packed[0], packed[3], packed[4]) != 0
        assert ba.lib.vba_last_error(ba.h).decode() == name + ": " + msg
        assert all(k.untouched() for k in packed[2])     # nothing was written
    packed = ba.search_by_projection_kf_pack([p])
    for n, pp, rr in ((-1, packed[3], packed[4]), (1, None, packed[4]), (1, packed[3], None)):
        assert fn(ba.h, n, pp, rr) != 0
        assert ba.lib.vba_last_error(ba.h).decode() == name + ": bad arguments"
    # a reloc problem without the filter needs no angles, a loop problem none either
    q = p.copy(check_orientation=False, angle=None, q_angle=None)
    cases.check_against("no angles", ba.search_by_projection_kf([q])[0], ref_mod.search_proj_kf_ref(q))
    w = synth.config_c3(seed=3, n_kf=6, n_pt=120, n_obs=500)
    t = ba.submit([w])
    rc = fn(ba.h, packed[0], packed[3], packed[4])
    err = ba.lib.vba_last_error(ba.h).decode()
    ba.wait(t)
    assert rc == -1 and "asynchronous batches pending" in err, (rc, err)
    assert packed[2][0].untouched()     # nothing was written
    cases.check_against("synth_small_reloc", ba.search_by_projection_kf([p])[0], cases.ref("synth_small_reloc"))
