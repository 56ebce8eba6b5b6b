"""vba_triangulate (k_triangulate) against tests/triangulate_ref.py in float64, on a real MI355X.

The cases come from tests/triangulate_cases.py; tests/test_triangulate_ref.py asserts on the CPU, for every match of every case,
that every comparison the yardstick evaluates has a margin of at least 1e-9, so every reason below is compared exactly and for
every match: none is excused."""
import numpy as np
import pytest

import triangulate_cases as cases
from mc_slam_amd import abi, backend, synth

pytestmark = pytest.mark.gpu

# Ten times the largest float64-against-longdouble difference of the yardstick's points over all matches of all cases, relative to
# the point's distance from Ow1, rounded up to one digit (tests/test_triangulate_ref.py::test_print_float64_against_longdouble
# prints 9.053e-14).  The kernel and the float64 yardstick are two FP64 evaluations of the same formulas (fused multiply-adds in
# the kernel), so each may differ from the exact value by about that much.
TOL = 1e-12


@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0)
    yield b
    b.close()


def _same(a, b):
    """two results of the library, bit for bit"""
    assert (a.status, a.n_accepted) == (b.status, b.n_accepted)
    assert a.x3d.tobytes() == b.x3d.tobytes() and a.reason.tobytes() == b.reason.tobytes()


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_against_the_yardstick(ba, case):
    p = cases.make(case)
    r = cases.reference(case)
    g = ba.triangulate([p])[0]
    assert g.status == 0 and g.reason.shape == (p.n_matches,)
    assert np.array_equal(g.reason, r["reason"]), [(i, g.reason[i], r["reason"][i]) for i in np.nonzero(g.reason != r["reason"])[0][:10]]
    assert g.n_accepted == r["n_accepted"] == int((g.reason == 0).sum())
    ok = (r["reason"] == 0) | (r["reason"] >= 3)
    assert not g.x3d[~ok].any()                                # zeros for reasons 1 and 2
    if ok.any():
        d = np.linalg.norm(g.x3d[ok] - r["x3d"][ok], axis=1) / np.linalg.norm(r["x3d"][ok] - p.Ow1, axis=1)
        print(cases.IDS[cases.CASES.index(case)], "points %d  largest |dx| / |x - Ow1| %.2e" % (ok.sum(), d.max()))
        assert d.max() <= TOL, (int(np.argmax(d)), d.max())


def _mixed_batch():
    some = [cases.make(cases.CASES[k]) for k in (2, 3, 6, 7, 8, 9)]
    empty = cases.make(cases.CASES[0])
    one = cases.make(cases.CASES[1])
    levels = synth.make_triangulate(31, 70, "std", n_levels=3)             # another table length between the others
    return [some[3], empty, some[0], one, empty, some[5], levels, some[1], some[2], some[4], empty]


def test_a_batch_equals_single_calls(ba):
    """bit for bit, whatever the position in the batch, in both orders, with empty pairs mixed in"""
    batch = _mixed_batch()
    single = [ba.triangulate([p])[0] for p in batch]
    for order in (list(range(len(batch))), list(reversed(range(len(batch))))):
        got = ba.triangulate([batch[i] for i in order])
        for i, g in zip(order, got):
            _same(g, single[i])
    e = single[1]
    assert (e.status, e.n_accepted) == (0, 0) and e.reason.shape == (0,)
    assert sum(s.n_accepted for s in single) > 100


def test_one_launch_per_call(ba):
    ba.triangulate(_mixed_batch())
    assert ba.get_profile()["kernel_launches"] == 1
    ba.triangulate([cases.make(cases.CASES[9])])               # three workgroups, one launch
    assert ba.get_profile()["kernel_launches"] == 1
    assert ba.triangulate([]) == []
    assert ba.triangulate([cases.make(cases.CASES[0])])[0].n_accepted == 0     # no match at all: nothing to launch
    assert ba.get_profile()["kernel_launches"] == 0


def test_the_thresholds_are_the_callers(ba):
    """cos_max, chi2_th and ratio_factor are read from the problem, and the level tables of each keyframe are its own"""
    p = cases.make(cases.CASES[8])
    g = ba.triangulate([p, p.copy(cos_max=2.0), p.copy(chi2_th=0.0), p.copy(ratio_factor=1.0), p.copy(level_sigma2_2=p.level_sigma2_2 * 0)])
    assert (g[1].reason != 1).all() and (g[0].reason == 1).any()
    assert set(g[2].reason) <= {1, 3, 4, 5}
    m = g[0].reason == 0
    assert set(g[3].reason[m]) == {8}                          # ratioDist < ratioOctave or > ratioOctave: one of them always holds
    assert set(g[4].reason[m]) == {6}


def test_refusals_and_pending_tickets(ba):
    p = cases.make(cases.CASES[2])
    K0 = p.K1.copy(); K0[0] = 0.0
    o = p.oct2.copy(); o[4] = 8
    for bad, msg in ((p.copy(oct2=o), "vba_triangulate: pair 1: match 4: octave >= n_levels"),
                     (p.copy(K1=K0), "vba_triangulate: pair 1: zero fx / fy"),
                     (p.copy(tcw2=np.array([0, np.nan, 0])), "vba_triangulate: pair 1: a pose is not finite"),
                     (p.copy(scale_1=-p.scale_1), "vba_triangulate: pair 1: level 0: scale <= 0")):
        with pytest.raises(RuntimeError, match=msg):
            ba.triangulate([p, bad])
    w = synth.config_c3(seed=3, n_kf=6, n_pt=120, n_obs=500)
    t = ba.submit([w])
    packed = ba.triangulate_pack([p])
    rc = ba.lib.vba_triangulate(ba.h, packed[0], packed[3], packed[4])
    err = ba.lib.vba_last_error(ba.h).decode()
    ba.wait(t)
    assert rc == -1 and "asynchronous batches pending" in err, (rc, err)
    assert (packed[2][0].r == 255).all()                       # nothing was written
    assert np.array_equal(ba.triangulate([p])[0].reason, cases.reference(cases.CASES[2])["reason"])
