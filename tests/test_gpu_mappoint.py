"""vba_mappoint_update (k_mappoint_update) against tests/mappoint_ref.py on a real MI355X.

The cases come from tests/mappoint_cases.py; tests/test_mappoint_ref.py asserts on the CPU that the yardstick agrees with a brute-force
sort and that float64 and longdouble agree in every integer output.  So best_obs, best_median, n_desc, desc, both states and the counts
are compared for equality and for every point: none is excused.  normal, dist_max and dist_min are compared within
mappoint_cases.NORMAL_TOL (absolute) and DIST_TOL (relative), ten times the float64-against-longdouble difference."""
import numpy as np
import pytest

import fuse_cases
import fuse_ref
import mappoint_cases as cases
import mappoint_ref as ref_mod
import triangulate_cases
from mc_slam_amd import abi, backend, synth

pytestmark = pytest.mark.gpu
NAMES = list(cases.cases())
ARRAYS = ("best_obs", "best_median", "n_desc", "desc", "normal", "dist_max", "dist_min", "desc_state", "normal_state")


@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0)
    yield b
    b.close()


def _same(a, b):
    """two results of the library, bit for bit"""
    assert (a.status, a.n_desc_done, a.n_normal_done) == (b.status, b.n_desc_done, b.n_normal_done)
    for k in ARRAYS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def test_against_the_yardstick(ba):
    """every case alone; prints the largest differences in front of the assertion on them"""
    worst_n = worst_d = 0.0
    for name in NAMES:
        got = ba.mappoint_update([cases.cases()[name]])[0]
        dn, dd = cases.check_against(name, got, cases.ref(name), normal_tol=np.inf, dist_tol=np.inf)
        worst_n, worst_d = max(worst_n, dn), max(worst_d, dd)
    print("largest difference GPU against the float64 yardstick: normal %.3e (tolerance %.0e), distances %.3e relative (tolerance %.0e)"
          % (worst_n, cases.NORMAL_TOL, worst_d, cases.DIST_TOL))
    assert worst_n <= cases.NORMAL_TOL and worst_d <= cases.DIST_TOL


def test_one_ragged_call_equals_single_calls(ba):
    """all cases in one call, bit for bit, whatever the position in the batch, in both orders; one launch per call"""
    ps = [cases.cases()[n] for n in NAMES]
    single = [ba.mappoint_update([p])[0] for p in ps]
    for order in (list(range(len(ps))), list(reversed(range(len(ps))))):
        got = ba.mappoint_update([ps[i] for i in order])
        assert ba.get_profile()["kernel_launches"] == 1
        for i, g in zip(order, got):
            _same(g, single[i])
            cases.check_against(NAMES[i], g, cases.ref(NAMES[i]))
    assert ba.mappoint_update([]) == []
    # a call without device work launches nothing and still answers
    got = ba.mappoint_update([cases.cases()["n_pt_0"], cases.cases()["all_bad"].copy(what=np.ones(2, dtype=np.uint8))])
    assert ba.get_profile()["kernel_launches"] == 0 and got[1].desc_state.tolist() == [3, 3] and got[1].normal_state.tolist() == [1, 1]


def test_a_points_answer_does_not_depend_on_its_neighbours(ba):
    """the points of the ragged case one by one (every 7th), each as a problem of its own over the same keyframe table"""
    p = cases.cases()["ragged_300"]
    whole = ba.mappoint_update([p])[0]
    idx = list(range(0, p.n_pt, 7)) + [int(i) for i in np.nonzero(np.diff(p.obs_begin) > 256)[0]]
    subs = []
    for i in idx:
        b, e = p.obs_begin[i], p.obs_begin[i + 1]
        subs.append(abi.MapPointProblem(kf_center=p.kf_center, kf_bad=p.kf_bad, what=p.what[i:i + 1], obs_begin=[0, e - b], obs_kf=p.obs_kf[b:e],
                                        obs_desc=p.obs_desc[b:e], pos=p.pos[i:i + 1], ref_kf=p.ref_kf[i:i + 1], ref_scale=p.ref_scale[i:i + 1],
                                        ref_top_scale=p.ref_top_scale[i:i + 1]))
    for i, g in zip(idx, ba.mappoint_update(subs)):
        for k in ARRAYS:
            assert getattr(g, k)[0].tobytes() == getattr(whole, k)[i].tobytes(), (i, k)


def test_refusals_and_pending_tickets(ba):
    fn, name = ba.lib.vba_mappoint_update, "vba_mappoint_update"
    p = cases.cases()["bad_kf"]

    def edit(field, i, v):
        a = getattr(p, field).copy()
        a.reshape(-1)[i] = v
        return p.copy(**{field: a})

    legal = cases.over_cap()
    b = legal.obs_begin.copy(); b[2:] -= 1                                       # the long list at exactly 1024: legal
    legal = legal.copy(obs_begin=b, obs_kf=legal.obs_kf[:-1], obs_desc=legal.obs_desc[:-1])
    assert np.diff(legal.obs_begin).max() == abi.MAPPOINT_MAX_OBS
    cases.check_against("cap", ba.mappoint_update([legal])[0], ref_mod.mappoint_ref(legal))
    for bad, msg in ((cases.over_cap(), "problem 1: point 1: more than 1024 observations: a point's descriptors live in LDS"),
                     (edit("obs_begin", 0, 1), "problem 1: obs_begin does not start at 0"),
                     (edit("obs_begin", 2, 5), "problem 1: obs_begin decreases at point 1"),
                     (edit("obs_kf", 3, 10), "problem 1: point 0: observation 3: obs_kf out of range"),
                     (edit("obs_kf", 9, -1), "problem 1: point 1: observation 0: obs_kf out of range"),
                     (edit("ref_kf", 2, 10), "problem 1: point 2: ref_kf out of range"),
                     (edit("kf_center", 7, np.inf), "problem 1: keyframe 2: centre is not finite"),
                     (edit("pos", 4, np.nan), "problem 1: point 1: position is not finite"),
                     (edit("ref_scale", 3, np.inf), "problem 1: point 3: a scale is not finite"),
                     (edit("ref_top_scale", 0, 0.0), "problem 1: point 0: a scale is <= 0"),
                     (edit("ref_scale", 4, -1.2), "problem 1: point 4: a scale is <= 0"),
                     (edit("what", 1, 4), "problem 1: point 1: what has a bit outside the two parts"),
                     (p.copy(obs_desc=None), "problem 1: NULL array that the descriptor part needs"),
                     (p.copy(pos=None), "problem 1: NULL array that the normal part needs")):
        packed = ba.mappoint_update_pack([p, bad])
        assert fn(ba.h, packed[0], packed[3], packed[4]) != 0
        assert ba.lib.vba_last_error(ba.h).decode() == name + ": " + msg
        assert all(k.untouched() for k in packed[2])     # nothing was written
    # what a part does not read is not checked: an out-of-range ref_kf and a NULL pos without a normal part, NULL descriptors without
    # a descriptor part
    w1, w2 = np.ones(p.n_pt, dtype=np.uint8), np.full(p.n_pt, 2, dtype=np.uint8)
    got = ba.mappoint_update([edit("ref_kf", 2, 10).copy(what=w1, pos=None, ref_scale=None), p.copy(what=w2, obs_desc=None)])
    want = ref_mod.mappoint_ref(p.copy(what=w1)), ref_mod.mappoint_ref(p.copy(what=w2))
    cases.check_against("desc only", got[0], want[0])
    cases.check_against("normal only", got[1], want[1])
    packed = ba.mappoint_update_pack([p])
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
    cases.check_against("bad_kf", ba.mappoint_update([p])[0], cases.ref("bad_kf"))


def test_between_calls_of_a_sibling(ba):
    """the call leaves the arena and the result of vba_triangulate on the same handle alone"""
    t = triangulate_cases.make(triangulate_cases.CASES[4])
    x = ba.triangulate([t])[0]
    cases.check_against("ties", ba.mappoint_update([cases.cases()["ties"]])[0], cases.ref("ties"))
    y = ba.triangulate([t])[0]
    assert x.status == y.status and x.x3d.tobytes() == y.x3d.tobytes() and x.reason.tobytes() == y.reason.tobytes()


def test_refreshed_points_feed_vba_fuse(ba):
    """the points of a fuse scene refreshed from synthetic observations (noisy copies of their descriptors seen from a few keyframes
    around the scene's), then desc, normal, 0.8f * dist_min and 1.2f * dist_max, float32 as MapPoint's getters return them, as the
    inputs of vba_fuse: what fuse_ref says for the yardstick-refreshed attributes"""
    s = synth.fuse_scene(61, n_keys=200, n_pt=80)
    r = np.random.default_rng(62)
    n_kf = 7
    lists = [np.sort(r.choice(n_kf, int(r.integers(2, 7)), replace=False)) for _ in range(s.n_pt)]
    descs = [np.stack([cases.noisy(r, s.pt_desc[i], int(r.integers(0, 6))) for _ in l]) for i, l in enumerate(lists)]
    m = cases.build(63, lists, n_kf, descs=descs, pos=s.pos)
    key = s.truth["key"]                                                          # the reference keyframe saw a match at its keypoint's octave
    m = m.copy(kf_center=cases.f32(s.Ow + r.normal(size=(n_kf, 3)) * 0.3),
               ref_scale=cases.SCALE[np.where(key >= 0, s.oct[np.maximum(key, 0)], 0)].astype(np.float64))
    got, want = ba.mappoint_update([m])[0], ref_mod.mappoint_ref(m)
    cases.check_against("chain", got, want)
    assert got.n_desc_done == got.n_normal_done == s.n_pt
    f = np.float32

    def refreshed(desc, normal, dmax, dmin):
        mx = dmax.astype(f)
        return s.copy(pt_desc=desc, normal=normal.astype(f).astype(np.float64), pred_max=mx.astype(np.float64),
                      dist_max=(f(1.2) * mx).astype(np.float64), dist_min=(f(0.8) * dmin.astype(f)).astype(np.float64))

    a = refreshed(got.desc, got.normal, got.dist_max, got.dist_min)
    b = refreshed(want["desc"], want["normal"], want["dist_max"], want["dist_min"])
    w = fuse_ref.fuse_ref(b, np.dtype("float64"))
    fuse_cases.check_against("chain", ba.fuse([a])[0], w)
    assert w["n_found"] > 40
