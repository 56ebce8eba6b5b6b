"""The cases of vba_mappoint_update, seeded, each the smallest shape at which k_mappoint_update can still go wrong: N at 1 .. 4 (the
lower median of an even N), around the wave (63, 64, 65), around the border between a wave item and a workgroup item (255, 256, 257)
and at the cap (1024); identical and complementary descriptors; rows with equal smallest median; bad keyframes at the head, in the
middle and at the tail of a list; every exit of both parts; the four values of `what` in one problem; and a ragged problem with both
item kinds.  Positions, centres and scale factors are float32 values (widened), so the float32 mode of the yardstick reads the same
inputs.  Shared by tests/test_mappoint_ref.py, test_host_mappoint.py, test_gpu_mappoint.py and scripts/mappoint_bench.py."""
import functools

import numpy as np

import mappoint_ref as ref_mod
from mc_slam_amd import abi

# the largest differences between the float64 and the longdouble yardstick over all cases (tests/test_mappoint_ref.py prints them and
# asserts these bounds on them): normal absolute, the two distances relative; the tolerances are ten times that, rounded up to one digit
NORMAL_LONGDOUBLE = 1.3e-15
NORMAL_TOL = 2e-14
DIST_LONGDOUBLE = 2.6e-16
DIST_TOL = 3e-15
# the largest difference between the float64 answer narrowed to float32 and the float32 mode (the reference's own arithmetic): normal
# in units of the float32 spacing at 1, the distances in units of their own spacing (measured; tests/test_mappoint_ref.py asserts twice these)
NORMAL_F32_ULPS = 5.0
DIST_F32_ULPS = 1.0

SCALE = np.float32(1.2) ** np.arange(8, dtype=np.float32)      # mvScaleFactors of 8 levels, float32


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def noisy(r, proto, flips):
    """a copy of the 256-bit prototype with `flips` random bits turned"""
    bits = np.unpackbits(proto)
    bits[r.permutation(256)[:flips]] ^= 1
    return np.packbits(bits)


def build(seed, lists, n_kf, what=3, kf_bad=(), descs=None, ref="first", pos=None):
    """a problem of len(lists) points; lists[i]: the observing keyframes of point i (ascending); descs[i]: its [n,32] descriptors
    (default: noisy copies of a prototype); ref: "first" (the first observer), "outside" (a keyframe that is no observer, where one
    exists) or an array"""
    r = np.random.default_rng(seed)
    n = len(lists)
    center = f32(r.uniform(-4.0, 4.0, (n_kf, 3)))
    bad = np.zeros(n_kf, dtype=np.uint8)
    bad[list(kf_bad)] = 1
    p = f32(r.uniform(-2.0, 2.0, (n, 3)) + [0.0, 0.0, 9.0]) if pos is None else f32(pos)
    begin = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    obs_kf = np.concatenate([np.asarray(l, dtype=np.int32) for l in lists] + [np.zeros(0, dtype=np.int32)])
    d = []
    for i, l in enumerate(lists):
        if descs is not None and descs[i] is not None:
            d.append(np.asarray(descs[i], dtype=np.uint8).reshape(len(l), 32))
            continue
        proto = r.integers(0, 256, 32, dtype=np.uint8)
        d.append(np.stack([noisy(r, proto, int(r.integers(0, 60))) for _ in l]) if len(l) else np.zeros((0, 32), dtype=np.uint8))
    if isinstance(ref, str):
        rk = np.zeros(n, dtype=np.int32)
        for i, l in enumerate(lists):
            out = np.setdiff1d(np.arange(n_kf), l)
            rk[i] = out[0] if (ref == "outside" and len(out)) else (l[0] if len(l) else 0)
    else:
        rk = np.asarray(ref, dtype=np.int32)
    lev = r.integers(0, 8, n)
    return abi.MapPointProblem(kf_center=center, kf_bad=bad, what=np.broadcast_to(np.asarray(what, dtype=np.uint8), (n,)).copy(), obs_begin=begin,
                               obs_kf=obs_kf, obs_desc=np.concatenate(d + [np.zeros((0, 32), dtype=np.uint8)]), pos=p, ref_kf=rk,
                               ref_scale=SCALE[lev].astype(np.float64), ref_top_scale=np.full(n, float(SCALE[7])))


def single(seed, n):
    """two points of N = n over n + 2 keyframes, one over a subset that skips keyframe 0"""
    return build(seed, [np.arange(n), np.arange(2, n + 2)], n + 2)


def long_tail(r, n, mean=8.0, cap=abi.MAPPOINT_MAX_OBS):
    """observation counts as a map has them: 2 to a few dozen for most points, hundreds for a few (a Pareto draw around `mean`)"""
    return np.minimum(2 + np.floor(r.pareto(1.6, n) * (mean - 2) * 0.6).astype(int), cap)


def ragged(seed, n_pt, n_kf=1100, force=(300, 700), mean=8.0, what=None, bad_frac=0.03):
    r = np.random.default_rng(seed)
    cnt = np.minimum(long_tail(r, n_pt, mean), n_kf)
    cnt[:len(force)] = force
    cnt = cnt[r.permutation(n_pt)]
    lists = [np.sort(r.choice(n_kf, c, replace=False)) for c in cnt]
    w = r.integers(0, 4, n_pt) if what is None else what
    return build(seed + 1, lists, n_kf, what=w, kf_bad=np.nonzero(r.random(n_kf) < bad_frac)[0], ref="first")


def over_cap():
    """one list of 1025 observations between two legal points: refused"""
    return build(90, [np.arange(3), np.arange(abi.MAPPOINT_MAX_OBS + 1), np.arange(2)], abi.MAPPOINT_MAX_OBS + 1)


@functools.lru_cache(maxsize=None)
def cases():
    r = np.random.default_rng(17)
    c = r.integers(0, 256, 32, dtype=np.uint8)
    far = lambda k: noisy(np.random.default_rng(100 + k), c, 100 + 10 * k)      # outliers, mutually far
    flip = lambda lo, hi: np.packbits(np.unpackbits(c) ^ np.isin(np.arange(256), np.arange(lo, hi)).astype(np.uint8))
    out = {}
    for n in (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1024):
        out["n%d" % n] = single(200 + n, n)
    out["identical"] = build(31, [np.arange(7)], 7, descs=[np.tile(c, (7, 1))])
    # (d, ~d): distance 256, the lower median of N = 2 is the 0 of the diagonal; (d, ~d, ~d): row 0 has median 256, rows 1 and 2 have 0
    out["complementary"] = build(32, [np.arange(2), np.arange(3)], 3, descs=[np.stack([c, ~c]), np.stack([c, ~c, ~c])])
    # equal smallest medians: the rows 0 and 3 (the earliest is the first row), 2, 3 and 4 (in the middle), the last two of four, and
    # three rows that tie at 10
    out["ties"] = build(33, [np.arange(5), np.arange(5), np.arange(4), np.arange(3)], 5,
                        descs=[np.stack([c, far(0), far(1), c, c]), np.stack([far(0), far(1), c, c, c]), np.stack([far(0), far(1), c, c]),
                               np.stack([c, flip(0, 10), flip(0, 20)])])
    # bad keyframes 0, 4 and 8 of nine: at the head, in the middle and at the tail of the first list, and other places of the others
    out["bad_kf"] = build(34, [np.arange(9), np.arange(1, 9), np.array([0, 4, 8, 9]), np.array([0, 1]), np.array([3, 4])], 10, kf_bad=(0, 4, 8))
    out["all_bad"] = build(35, [np.arange(4), np.array([1, 3])], 4, kf_bad=(0, 1, 2, 3))
    out["no_obs"] = build(36, [np.arange(3), np.zeros(0, dtype=int), np.arange(2)], 3)
    out["what_mixed"] = build(37, [np.arange(1 + i % 5) for i in range(12)], 6, what=np.arange(12) % 4, ref="outside")
    out["n_pt_0"] = build(38, [], 4)
    out["n_kf_1"] = build(39, [np.arange(1), np.arange(1), np.zeros(0, dtype=int)], 1)
    p = build(40, [np.arange(5), np.arange(2, 6), np.arange(300)], 300)
    pos = p.pos.copy()
    pos[0], pos[2] = p.kf_center[3], p.kf_center[299]                             # points 0 and 2 lie in an observer's centre
    out["at_centre"] = p.copy(pos=pos)
    out["ref_outside"] = build(41, [np.arange(1, 6), np.arange(2, 4)], 8, ref="outside")
    out["ragged_300"] = ragged(50, 300)
    return out


@functools.lru_cache(maxsize=None)
def ref(name, mode="float64"):
    return ref_mod.mappoint_ref(cases()[name], mode)


INTS = ("best_obs", "best_median", "n_desc", "desc", "desc_state", "normal_state")


def check_against(what, got, want, normal_tol=NORMAL_TOL, dist_tol=DIST_TOL):
    """a library result against a float64 yardstick result: every integer output, both states and the counts equal for every point,
    normal within normal_tol (absolute) and the two distances within dist_tol (relative).  Returns the two largest differences"""
    assert (got.status, got.n_desc_done, got.n_normal_done) == (0, want["n_desc_done"], want["n_normal_done"]), what
    for k in INTS:
        assert np.array_equal(getattr(got, k), want[k]), (what, k)
    dn = float(np.abs(got.normal - want["normal"]).max(initial=0))
    dd = 0.0
    for k in ("dist_max", "dist_min"):
        g, w = getattr(got, k), want[k]
        assert np.array_equal(g == 0, w == 0), (what, k)
        m = w != 0
        dd = max(dd, float((np.abs(g[m] - w[m]) / w[m]).max(initial=0)))
    assert dn <= normal_tol and dd <= dist_tol, (what, dn, dd)
    return dn, dd
