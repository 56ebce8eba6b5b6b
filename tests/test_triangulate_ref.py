"""CPU checks of the vba_triangulate yardstick (tests/triangulate_ref.py) and of the conditions the GPU comparison rests on, for
every case of tests/triangulate_cases.py and EVERY match of it (no match is excused: the share left out is zero)."""
import numpy as np
import pytest

import triangulate_cases as cases
import triangulate_ref as ref
from mc_slam_amd import abi, synth

MARGIN_MIN = 1e-9   # of every comparison the yardstick evaluates: ~ 1e7 ulp, no rounding difference between two FP64 routes flips one
CODES = (0, 1, 3, 4, 5, 6, 8)   # 2 and 7 are unreachable behind the parallax and depth tests


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_hestenes_against_numpy_svd(case):
    """the float64 Hestenes vector of the smallest singular value against np.linalg.svd: the singular values to 1e-13 of the largest,
    the vector (up to sign) to 1e-13 scaled by the relative gap to the next singular value, which is what determines it"""
    p = cases.make(case)
    if p.n_matches == 0:
        return
    _, _, A = ref.build_A(p, np.float64)
    sig2, V = ref.hestenes4(A, np.float64)
    v = ref.smallest(sig2, V)
    U_, w, Vt = np.linalg.svd(A)
    assert (np.abs(np.sort(np.sqrt(sig2), axis=1)[:, ::-1] - w) <= 1e-13 * w[:, :1]).all()
    u = Vt[:, 3, :]
    sgn = np.sign(np.einsum("ni,ni->n", v, u))
    gap = (w[:, 2] - w[:, 3]) / w[:, 0]
    assert (np.abs(v - sgn[:, None] * u).max(axis=1) * gap <= 1e-13).all()
    assert (np.abs(np.linalg.norm(v, axis=1) - 1) <= 1e-14).all()
    # the columns of V are orthonormal
    assert np.abs(np.einsum("nij,nik->njk", V, V) - np.eye(4)).max() <= 1e-14


def test_noise_free_points_are_recovered():
    """exact pixels (in float64, not rounded through float32) of known points: the triangulated point is the point"""
    p = synth.make_triangulate(21, 200, "std")
    X = p.truth["Xw"]
    C1, C2 = -p.Rcw1.T @ p.tcw1, -p.Rcw2.T @ p.tcw2
    pix = lambda K, R, t: (lambda Y: np.stack([K[0] * Y[:, 0] / Y[:, 2] + K[2], K[1] * Y[:, 1] / Y[:, 2] + K[3]], axis=1))(X @ R.T + t)
    q = p.copy(uv1=pix(p.K1, p.Rcw1, p.tcw1), uv2=pix(p.K2, p.Rcw2, p.tcw2), oct1=np.zeros(200, dtype=np.uint8), oct2=np.zeros(200, dtype=np.uint8),
               Ow1=C1, Ow2=C2)
    r = ref.triangulate(q)
    ok = r["reason"] != 1                                      # the deep points fail the parallax gate and have no point
    assert ok.sum() >= 100 and set(r["reason"][ok]) <= {0, 8}
    d = np.linalg.norm(r["x3d"][ok] - X[ok], axis=1) / np.linalg.norm(X[ok] - C1, axis=1)
    # the float32 rotation is orthonormal to 1e-7 only, which bends the rays by as much: depth error ~ 1e-7 / parallax
    assert d.max() <= 1e-4, d.max()
    assert not r["x3d"][~ok].any()


def _hand_made():
    """two cameras 0.4 m apart looking down +z (keyframe 2 to the right), levels 1.2^l; one match per reason"""
    scale, sigma2 = synth.level_tables()
    K = np.array([400.0, 400.0, 320.0, 240.0])
    I = np.eye(3)
    base = dict(Rcw1=I, tcw1=np.zeros(3), Ow1=np.zeros(3), K1=K, Rcw2=I, tcw2=[-0.4, 0, 0], Ow2=[0.4, 0, 0], K2=K, level_sigma2_1=sigma2, scale_1=scale,
                level_sigma2_2=sigma2, scale_2=scale)
    pix = lambda X, C: [K[0] * (X[0] - C[0]) / X[2] + K[2], K[1] * X[1] / X[2] + K[3]]
    X = np.array([0.3, -0.2, 4.0])
    a, b = pix(X, [0, 0, 0]), pix(X, [0.4, 0, 0])
    rows = {
        0: (a, b, 0, 0),
        1: (pix([0.3, -0.2, 400.0], [0, 0, 0]), pix([0.3, -0.2, 400.0], [0.4, 0, 0]), 0, 0),     # parallax 0.001 rad
        3: (b, a, 0, 0),                                     # the pixels swapped: the rays meet behind both cameras
        5: (a, [b[0], b[1] + 8.0], 0, 3),                    # 8 pixels off the epipolar line, split evenly: 16 > 5.991 in keyframe 1 ...
        6: (a, [b[0], b[1] + 8.0], 3, 0),                    # ... and the other way round 16 < 5.991 * 2.99 there: only keyframe 2 objects
        8: (a, b, 0, 6),                                     # the same distance seen five octaves apart
    }
    # reason 4: keyframe 2 stands IN FRONT of keyframe 1 and the point lies between them
    fwd = dict(base, tcw2=[0, 0, -0.4], Ow2=[0, 0, 0.4])
    Xb = np.array([0.12, 0.0, 0.2])
    rows4 = ([K[0] * Xb[0] / Xb[2] + K[2], K[3]], [K[0] * Xb[0] / (Xb[2] - 0.4) + K[2], K[3]], 0, 0)
    mk = lambda kw, r: abi.TriangulateProblem(uv1=[r[0]], uv2=[r[1]], oct1=[r[2]], oct2=[r[3]], **kw)
    out = {code: mk(base, r) for code, r in rows.items()}
    out[4] = mk(fwd, rows4)
    return out, X, Xb


def test_one_hand_made_match_per_reason():
    problems, X, Xb = _hand_made()
    assert sorted(problems) == sorted(CODES)
    for code, p in problems.items():
        for dtype in (np.float32, np.float64, np.longdouble):
            r = ref.triangulate(p, dtype)
            assert r["reason"][0] == code, (code, dtype, r["reason"][0])
            assert r["n_accepted"] == int(code == 0)
    assert np.abs(ref.triangulate(problems[0])["x3d"][0] - X).max() <= 1e-12
    assert np.abs(ref.triangulate(problems[8])["x3d"][0] - X).max() <= 1e-12      # the point that failed is handed out
    assert np.abs(ref.triangulate(problems[4])["x3d"][0] - Xb).max() <= 1e-12
    assert not ref.triangulate(problems[1])["x3d"].any()
    r3 = ref.triangulate(problems[3])
    assert r3["x3d"][0, 2] < 0 and np.isinf(r3["margins"][0, ref.MARGINS.index("z2")])     # :1433 is never reached


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_every_margin_of_every_match(case):
    r = cases.reference(case)
    if case[1] == 0:
        assert r["reason"].shape == (0,) and r["n_accepted"] == 0
        return
    m = r["margins"]
    assert np.isfinite(m[:, 0]).all()                         # the first comparison is evaluated for every match
    print("case", case, "smallest margin %.2e" % r["margin"].min(), dict(zip(ref.MARGINS, ["%.1e" % v for v in m.min(axis=0)])))
    assert (m >= MARGIN_MIN).all(), (np.unravel_index(np.argmin(m), m.shape), m.min())
    assert not np.isnan(m).any()


def test_the_cases_cover_what_they_are_there_for():
    tot = np.zeros(9, dtype=int)
    for case in cases.CASES:
        tot += np.bincount(cases.reference(case)["reason"], minlength=9)
    print("reasons over all cases:", dict(enumerate(tot.tolist())))
    for code in CODES:
        assert tot[code] >= 5, (code, tot)
    assert sorted({c[1] for c in cases.CASES}) == [0, 1, 63, 64, 65, 255, 256, 257, 513]
    far = [c for c in cases.CASES if c[2] == "far"]
    assert len(far) == 1
    p, r = cases.make(far[0]), cases.reference(far[0])
    assert abs(np.linalg.norm(p.Ow1) - 50.0) < 1e-3
    inside = r["reason"] != 1
    assert inside.sum() >= 100 and (r["cos"][inside] > 0.9990).all()            # just inside the gate of 0.9998
    # reasons 4 and 6 come from the deliberately made matches
    fw = [c for c in cases.CASES if c[2] == "forward"]
    k4 = sum(int((cases.reference(c)["reason"][cases.make(c).truth["kind"] == 4] == 4).sum()) for c in fw)
    k6 = sum(int((cases.reference(c)["reason"][cases.make(c).truth["kind"] == 5] == 6).sum()) for c in fw)
    assert k4 >= 5 and k6 >= 5


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_float64_and_longdouble_decide_alike(case):
    r, rl = cases.reference(case), cases.reference(case, "longdouble")
    assert np.array_equal(r["reason"], rl["reason"]) and r["n_accepted"] == rl["n_accepted"]


def _has_point(reason):
    return (reason == 0) | (reason >= 3)


def test_print_float64_against_longdouble():
    """the figure the tolerance of tests/test_gpu_triangulate.py derives from (printed, -s shows it): the largest difference of the
    points between the float64 and the longdouble yardstick over all matches of all cases, relative to the point's distance from Ow1"""
    worst = 0.0
    for case in cases.CASES:
        p, r, rl = cases.make(case), cases.reference(case), cases.reference(case, "longdouble")
        ok = _has_point(r["reason"])
        if ok.any():
            d = np.linalg.norm((r["x3d"][ok] - rl["x3d"][ok]).astype(np.float64), axis=1) / np.linalg.norm(r["x3d"][ok] - p.Ow1, axis=1)
            worst = max(worst, float(d.max()))
    print("float64 against longdouble over all matches of all cases: |dx| / |x - Ow1| %.3e" % worst)
    assert np.isfinite(worst) and worst > 0


def test_print_float32_deviation():
    """how many decisions change when the yardstick computes as the reference does, in float32, and how far its points lie from the
    float64 ones (printed for DESIGN.md section 8, row f-8; not asserted: it is the size of a recorded deviation, not a requirement)"""
    n_d = n_tot = 0
    worst = 0.0
    for case in cases.CASES:
        p, r, r32 = cases.make(case), cases.reference(case), cases.reference(case, "float32")
        n_d += int((r["reason"] != r32["reason"]).sum())
        n_tot += len(r["reason"])
        ok = _has_point(r["reason"]) & _has_point(r32["reason"])
        if ok.any():
            d = np.linalg.norm(r["x3d"][ok] - r32["x3d"][ok].astype(np.float64), axis=1) / np.linalg.norm(r["x3d"][ok] - p.Ow1, axis=1)
            worst = max(worst, float(d.max()))
    print("float32 against float64: %d of %d decisions differ; largest |dx| / |x - Ow1| of the points %.3e" % (n_d, n_tot, worst))
