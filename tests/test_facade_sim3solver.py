"""The Sim3Solver of the host facade (mc_slam_amd/host/Sim3Solver.h): on the CPU the constructor's products, SetRansacParameters and
the draw against their NumPy mirror (tests/facade_sim3solver_lib.py); on the GPU iterate(5) until bNoMore or a hit, and find(),
against tests/sim3_ransac_ref.py driven by the same triples."""
import numpy as np
import pytest

import facade_sim3_lib
import facade_sim3solver_lib as fl
import sim3_ransac_ref as ref
from mc_slam_amd import synth
from mc_slam_amd.synth import quat_to_rot


def _pair(seed, n, fix_scale, outlier_frac, specials=True):
    p = synth.make_sim3_ransac(seed, n, fix_scale, outlier_frac)
    pair = facade_sim3_lib.Sim3Pair(fl.as_sim3_problem(p, p.truth["S12"]), seed=seed, specials=specials)
    return p, pair


@pytest.fixture(scope="module")
def built():
    p, pair = _pair(11, 90, 0, 0.4)
    yield p, pair
    pair.close()


def test_constructor_against_the_mirror(built):
    p, pair = built
    want, rows = fl.ransac_problem(pair, 0)
    s = fl.Solver(pair, 0)
    try:
        a, i = s.arrays(), s.info()
        assert i["N"] == p.n_pairs == want.n_pairs and i["mN1"] == len(pair.matches) and i["N"] < i["mN1"]   # the specials are filtered
        assert np.array_equal(a["indices1"], rows)
        assert np.array_equal(a["p1c"], want.p1c) and np.array_equal(a["p2c"], want.p2c)
        assert np.array_equal(a["gate1"], want.max_err1) and np.array_equal(a["gate2"], want.max_err2)
        assert set(a["gate1"]) <= {9.0, 13.0, 19.0, 27.0}              # 9.210 sigma2 in a size_t
        assert np.array_equal(a["K1"], want.K1) and np.array_equal(a["K2"], want.K2)
        # the float32 points are the generator's to float32 rounding of the pose chain
        assert np.abs(a["p1c"] - p.p1c).max() < 1e-4
    finally:
        s.close()


@pytest.mark.parametrize("prob,min_inliers,max_its", [(0.99, 6, 300), (0.99, 20, 300), (0.99, 20, 50), (0.999, 45, 300), (0.5, 89, 300), (0.99, 90, 300),
                                                        (0.99, 91, 300), (0.99, 1, 300)])
def test_set_ransac_parameters(built, prob, min_inliers, max_its):
    _, pair = built
    s = fl.Solver(pair, 1)
    try:
        assert s.info()["max_its"] == fl.max_iterations(90)            # the constructor's defaults: 0.99, 6, 300
        s.set_ransac(prob, min_inliers, max_its)
        i = s.info()
        assert i["min_inliers"] == min_inliers and i["iterations"] == 0
        assert i["max_its"] == fl.max_iterations(90, prob, min_inliers, max_its), (i, prob, min_inliers, max_its)
    finally:
        s.close()
    assert fl.max_iterations(90, 0.99, 90, 300) == 1 and fl.max_iterations(90, 0.99, 20, 300) == 300 and fl.max_iterations(90, 0.99, 45, 300) == 35


def test_draw_against_the_mirror():
    L = fl.lib()
    for n, seed in ((90, 5), (4, 6), (3, 7)):
        p, pair = _pair(20 + n, n, 1, 0.0, specials=False)
        s = fl.Solver(pair, 1)
        try:
            L.fc_srand(seed)
            got = s.draw(200)
            L.fc_srand(seed)
            want = fl.draw(n, 200)
            assert np.array_equal(got, want)
            assert got.min() >= 0 and got.max() < n
            dup = sum(len(set(r)) < 3 for r in got.tolist())
            print("n", n, "triples with a repeated pair:", dup, "of 200")
            if n <= 4:
                assert dup > 0                                          # the [idx] / [randi] removal as it stands
        finally:
            s.close()
            pair.close()


def test_too_few_pairs_end_at_once():
    """N < mRansacMinInliers: bNoMore and no backend call (:145-149), so this runs without a device"""
    p, pair = _pair(3, 12, 0, 0.0, specials=False)
    s = fl.Solver(pair, 0)
    try:
        s.set_ransac(0.99, 20, 300)
        r = s.iterate(5)
        assert not r["found"] and r["no_more"] and r["n_inliers"] == 0 and not r["inliers"].any() and len(r["triples"]) == 0
    finally:
        s.close()
        pair.close()


def _drive(s, rows, want, min_inliers, step):
    """iterate(step) until bNoMore or a hit, the yardstick beside it on the same triples; returns the last answer"""
    best, bestS, done = 0, np.zeros(8), 0
    budget = s.info()["max_its"]
    while True:
        r = s.iterate(step, max_hyp=max(step, 300) if step > 0 else 300)
        q = want.copy(sample=r["triples"], min_inliers=min_inliers, best_inliers=best, best_S12=bestS)
        y = ref.ransac(q)
        assert len(r["triples"]) == (min(step, budget - done) if step > 0 else budget)
        assert (y["gap"] >= 1e-4).all() and (y["margin"] >= 1e-6).all()     # the condition of an exact comparison (a seed that fails it is replaced)
        done += y["its_done"]
        best, bestS = y["best_inliers"], y["best_S12"]
        i = s.info()
        assert (i["iterations"], i["best_inliers"]) == (done, best)
        assert r["found"] == (y["hit"] >= 0) and r["n_inliers"] == y["n_inliers"]
        if y["hit"] >= 0:
            inl = np.zeros(len(r["inliers"]), dtype=bool)
            inl[rows[y["inlier"].astype(bool)]] = True
            assert np.array_equal(r["inliers"], inl)
            S = y["S12"]
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = S[7] * quat_to_rot(S[3:7]), S[:3]
            assert np.array_equal(r["T12"], np.float32(T)) or np.abs(r["T12"] - T).max() < 1e-6
        else:
            assert not r["inliers"].any()
        assert r["no_more"] == (y["hit"] < 0 and done >= budget)
        if best > 0 or y["best_hyp"] >= 0:
            R, t, sc = s.estimate()
            assert np.abs(R - quat_to_rot(bestS[3:7])).max() < 1e-6 and np.abs(t - bestS[:3]).max() < 1e-6 and abs(sc - bestS[7]) < 1e-6
        if r["found"] or r["no_more"]:
            return r, done


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,fix_scale,outlier_frac,min_inliers,rseed", [(11, 90, 0, 0.4, 20, 1), (12, 70, 1, 0.5, 20, 2), (13, 40, 0, 0.3, 35, 3)])
def test_iterate_against_the_yardstick(seed, n, fix_scale, outlier_frac, min_inliers, rseed):
    p, pair = _pair(seed, n, fix_scale, outlier_frac)
    want, rows = fl.ransac_problem(pair, fix_scale)
    s = fl.Solver(pair, fix_scale)
    try:
        s.set_ransac(0.99, min_inliers, 300)
        fl.lib().fc_srand(rseed)
        r, done = _drive(s, rows, want, min_inliers, 5)
        print("seed", seed, "found", r["found"], "after", done, "hypotheses of", s.info()["max_its"], "inliers", r["n_inliers"])
    finally:
        s.close()
        pair.close()


@pytest.mark.gpu
def test_find_against_the_yardstick():
    p, pair = _pair(11, 90, 0, 0.4)
    want, rows = fl.ransac_problem(pair, 0)
    s = fl.Solver(pair, 0)
    try:
        s.set_ransac(0.99, 20, 300)
        fl.lib().fc_srand(9)
        r, done = _drive(s, rows, want, 20, -1)
        assert r["found"] and done < 300
    finally:
        s.close()
        pair.close()
