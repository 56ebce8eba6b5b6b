"""ORBmatcher::SearchForInitialization and the MonocularInitialization slice of Tracking of the host facade
(mc_slam_amd/host/ORBmatcherInit.cpp, Tracking.cpp): the refusals on the CPU; on a real MI355X the matcher against
tests/search_init_ref.py on a mock pair, the slice on both sides of its two gates, and one chained run in which the slice's matches
reach Initializer::Initialize, against a direct vba_two_view_init call on the same matches."""
import functools

import numpy as np
import pytest

import facade_search_init_lib as fs
import search_init_ref as ref_mod
import two_view_cases
from mc_slam_amd import abi, backend, synth

FLAGS = ("ok", "model", "reason", "best_hyp_h", "best_hyp_f", "n_inliers_h", "n_inliers_f", "n_rt", "best_rt")


def pair(seed, n1, n2, **kw):
    """a mock pair as Tracking::MonocularInitialization meets it: 640 x 480, the 64 x 48 grid, ORBmatcher(0.9, true), window 100"""
    return synth.search_init_scene(seed, n_keys1=n1, n_keys2=n2, window_size=100.0, th_low=50, nn_ratio=0.9, check_orientation=True, **kw)


@functools.lru_cache(maxsize=None)
def with_matches(target):
    """a pair of 400 x 400 keypoints without twins and crowding for which the yardstick returns exactly `target` matches: matched
    keypoints of frame 1 are lifted to octave 1 (they leave at the level gate) until the count is reached"""
    p = pair(77, 400, 400, level0=1.0, matched=0.6, twins=0.0, crowd=0.0, angle_outliers=0.0)
    for _ in range(60):
        r = ref_mod.search_init_ref(p)
        if r["n_matches"] == target:
            return p, r
        assert r["n_matches"] > target
        kept = np.nonzero(r["state"] == 0)[0]
        o = p.oct1.copy()
        o[kept[:max(1, (r["n_matches"] - target) // 2)]] = 1      # in halves: the filter's 10 % rule can let a small bin back in
        p = p.copy(oct1=o)
    raise AssertionError("no pair with %d matches" % target)


def test_refusals(capfd):
    """refused in front of any backend work, so without a GPU: the message on std::cerr, -1, vnMatches12 and vbPrevMatched untouched"""
    p = pair(3, 30, 40)
    for change, msg in ((lambda f1, f2: f1.set_uright(4, 1.0), "frame 1 has a stereo keypoint (the backend is monocular)"),
                        (lambda f1, f2: f2.set_uright(7, 0.0), "frame 2 has a stereo keypoint (the backend is monocular)"),
                        (None, "vbPrevMatched has not one entry per keypoint of frame 1")):
        f1, f2 = fs.frames(p)
        prev = p.prev_matched if change else p.prev_matched[:-1]
        if change:
            change(f1, f2)
        capfd.readouterr()
        r = fs.search(f1, f2, prev)
        err = capfd.readouterr().err
        f1.close(); f2.close()
        assert r["ret"] == -1 and err.strip() == "ORBmatcher::SearchForInitialization: " + msg
        assert len(r["matches12"]) == 0 and r["prev_matched"].tobytes() == np.ascontiguousarray(prev).tobytes()
    # the slice passes a refusal on and drops its initializer
    f1, f2 = fs.frames(pair(4, 120, 120))
    f2.set_uright(0, 2.0)
    r = fs.monocular_initialization(f1, f2, pair(4, 120, 120).prev_matched)
    f1.close(); f2.close()
    assert (r["ret"], r["alive"]) == (-1, 0) and (r["matches12"] == 5).all()


@pytest.mark.gpu
def test_matcher_against_the_yardstick():
    """vnMatches12, vbPrevMatched and the return value on a 150-keypoint mock pair, with the reference's default window and with 100"""
    p = pair(11, 150, 150)
    for q, args in ((p, dict(window=100)), (p.copy(window_size=10.0, nn_ratio=0.6, check_orientation=False), dict(window=10, nnratio=0.6, check_ori=False))):
        want = ref_mod.search_init_ref(q)
        assert want["margin"] >= 1e-9 and want["margin_r"] >= 1e-9
        f1, f2 = fs.frames(q)
        got = fs.search(f1, f2, q.prev_matched, **args)
        f1.close(); f2.close()
        assert got["ret"] == want["n_matches"] and np.array_equal(got["matches12"], want["match12"])
        assert got["prev_matched"].tobytes() == want["prev_matched"].tobytes()
    assert ref_mod.search_init_ref(p)["n_matches"] > 20 and ref_mod.search_init_ref(p)["n_stolen"] > 0


@pytest.mark.gpu
def test_slice_on_both_sides_of_the_keypoint_gate():
    """100 keypoints in the current frame: no matcher call, the initializer goes, mvIniMatches is filled with -1; 101: the matcher runs"""
    for n2, called in ((100, False), (101, True)):
        p = pair(21, 130, n2)
        f1, f2 = fs.frames(p)
        r = fs.monocular_initialization(f1, f2, p.prev_matched)
        f1.close(); f2.close()
        if not called:
            assert (r["ret"], r["alive"]) == (-2, 0) and (r["matches12"] == -1).all() and r["prev_matched"].tobytes() == p.prev_matched.tobytes()
            continue
        want = ref_mod.search_init_ref(p)
        assert r["ret"] == want["n_matches"] < 100 and r["alive"] == 0
        assert np.array_equal(r["matches12"], want["match12"]) and r["prev_matched"].tobytes() == want["prev_matched"].tobytes()


@pytest.mark.gpu
def test_slice_on_both_sides_of_the_match_gate():
    """99 matches: the initializer is deleted; 100: it stays.  The matches are the yardstick's either way"""
    for target, alive in ((99, 0), (100, 1)):
        p, want = with_matches(target)
        f1, f2 = fs.frames(p)
        r = fs.monocular_initialization(f1, f2, p.prev_matched)
        f1.close(); f2.close()
        assert (r["ret"], r["alive"], r["init_ret"]) == (target, alive, -1)
        assert np.array_equal(r["matches12"], want["match12"]) and r["prev_matched"].tobytes() == want["prev_matched"].tobytes()


@pytest.mark.gpu
def test_the_slices_matches_reach_initialize():
    """a two-view scene with descriptors: the slice matches its 300 keypoints, Initialize runs on mvIniMatches, and its flags are those
    of a direct vba_two_view_init call on the same matches and the sets the facade drew"""
    t = two_view_cases.make("general-300x200")
    r = np.random.default_rng(5)
    n1, n2 = t.n_keys1, t.n_keys2
    uv1, uv2 = t.uv1.astype(np.float32), t.uv2.astype(np.float32)
    d2 = r.integers(0, 256, (n2, 32), dtype=np.uint8)
    d1 = r.integers(0, 256, (n1, 32), dtype=np.uint8)
    prev = uv1.copy()
    for i1, i2 in t.match:
        bits = np.unpackbits(d2[i2])
        bits[r.permutation(256)[:int(r.integers(0, 12))]] ^= 1
        d1[i1] = np.packbits(bits)
        prev[i1] = uv2[i2] + np.float32(0.25)                     # the last matched position, as an earlier frame left it
    lo, hi = np.floor(uv2.min(axis=0)) - 1, np.ceil(uv2.max(axis=0)) + 1
    bounds = (lo[0], hi[0], lo[1], hi[1])
    K = tuple(float(k) for k in t.K)
    f1 = fs.FrameH(uv1, np.zeros(n1), np.zeros(n1), d1, bounds, 64, 48, K)
    f2 = fs.FrameH(uv2, np.zeros(n2), np.zeros(n2), d2, bounds, 64, 48, K)
    o = fs.monocular_initialization(f1, f2, prev, do_initialize=True)
    f1.close(); f2.close()
    m = o["matches12"]
    assert o["ret"] == int((m >= 0).sum()) >= 100 and o["alive"] == 1 and o["init_ret"] in (0, 1)
    assert {(int(a), int(b)) for a, b in t.match} <= {(i, int(k)) for i, k in enumerate(m) if k >= 0}     # every true match was found
    idx = np.nonzero(m >= 0)[0]
    q = abi.TwoViewProblem(uv1=uv1.astype(np.float64), uv2=uv2.astype(np.float64), match=np.stack([idx, m[idx]], axis=1), sets=o["sets"], K=np.asarray(K, dtype=np.float32),
                           sigma=1.0, min_parallax=1.0, min_triangulated=50)
    ba = backend.LocalBA(0)
    d = ba.two_view_init([q])[0]
    ba.close()
    assert o["info"]["n_matches"] == len(idx) and o["init_ret"] == d.ok
    for k in FLAGS:
        assert o["info"][k] == getattr(d, k), k
    if d.ok:
        assert np.array_equal(o["vbTriangulated"], d.triangulated) and np.array_equal(o["R21"], d.R21.astype(np.float32))
        assert np.array_equal(o["vP3D"], d.x3d.astype(np.float32))
