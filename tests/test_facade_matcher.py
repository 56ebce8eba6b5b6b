"""ORBmatcher::SearchForTriangulation, LocalMapping::ComputeF12 and the CreateNewMapPoints overload that calls the matcher itself
(mc_slam_amd/host/ORBmatcher.cpp, LocalMapping.cpp) on the mock map of tests/test_facade_newpoints.py, against the yardstick
tests/search_tri_ref.py fed with the facade's float32 F12 and epipole."""
import numpy as np
import pytest

import facade_matcher_lib
import search_tri_ref as ref
from mc_slam_amd import synth


@pytest.fixture()
def scene():
    s = facade_matcher_lib.MatcherScene()
    yield s
    s.close()


def test_compute_f12_against_float64(scene):
    """ComputeF12 holds float32 values of an FP64 product: an entry is off by at most 2^-24 of itself, so by at most 2^-24 of the
    matrix norm; ten times that is asserted, the measured spread printed (CPU only)"""
    worst = 0.0
    for k2 in (2, 4):
        F, e = scene.f12(1, k2)
        (R1, t1), (R2, t2) = scene.pose[1], scene.pose[k2]
        K1, K2 = scene.K[1].astype(np.float32).astype(np.float64), scene.K[k2].astype(np.float32).astype(np.float64)
        want = synth.compute_f12(R1, t1, K1, R2, t2, K2)
        worst = max(worst, np.abs(F - want).max() / np.linalg.norm(want))
        C2 = R2 @ (-R1.T @ t1) + t2
        assert np.allclose(e, [K2[0] * C2[0] / C2[2] + K2[2], K2[1] * C2[1] / C2[2] + K2[3]], rtol=1e-3)
    print("ComputeF12 against float64: largest |dF| / |F| %.3e" % worst)
    assert worst <= 10 * 2.0 ** -24


def test_only_stereo_is_refused(scene):
    assert scene.search(1, 2, True, only_stereo=True)[0] == -1


@pytest.mark.gpu
@pytest.mark.parametrize("check_orientation", [False, True])
def test_search_for_triangulation_equals_the_yardstick(scene, check_orientation):
    for k2 in (2, 4):
        r = ref.search_tri_ref(scene.problem(1, k2, check_orientation))
        assert r["margin"] >= 1e-9 and r["n_matches"] >= 30
        n, pairs = scene.search(1, k2, check_orientation)
        assert n == r["n_matches"] and np.array_equal(pairs, r["pairs"])


@pytest.mark.gpu
def test_new_overload_equals_the_existing_one_with_the_yardsticks_matches():
    a, b = facade_matcher_lib.MatcherScene(), facade_matcher_lib.MatcherScene()
    try:
        n_a, ids_a = a.create_matched([2, 3, 4])
        ids_b = []
        for k2 in (2, 3, 4):                                   # neighbour by neighbour: the matcher of 4 sees the points made from 2
            b.matches[k2] = ref.search_tri_ref(b.problem(1, k2, False))["pairs"].astype(np.int64).reshape(-1, 2)
            if len(b.matches[k2]) == 0:
                b.matches[k2] = np.zeros((0, 2), dtype=np.int64)
                continue
            n, _, ids = b.create([k2])
            assert n >= 0
            ids_b += ids.tolist()
        assert n_a == len(ids_a) == len(ids_b) and n_a >= 20
        assert a.L.fc_map_n_points(a.m) == b.L.fc_map_n_points(b.m) == n_a
        for ia, ib in zip(ids_a, ids_b):
            Pa, ra, na, oa = a.point(ia)
            Pb, rb, nb, ob = b.point(ib)
            assert Pa.tobytes() == Pb.tobytes() and (ra, na, oa) == (rb, nb, ob)
    finally:
        a.close(); b.close()
