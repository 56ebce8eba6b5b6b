"""The host half of vba_sim3_ransac (mc_slam_amd/csrc/vba_host_sim3_ransac.h, vba_host_arena.h: refusals, arena offsets, packing,
write-back) under AddressSanitizer + UBSan (CPU only).  The harness (tests/host_sim3_ransac_check.cpp) packs into heap blocks of
exactly the arena's sizes; every expected offset below is restated from the sizes alone, and the packed regions are compared with
the interleaving done in NumPy through an order-sensitive checksum."""
import numpy as np
import pytest

from mc_slam_amd import synth
import host_check_lib as hc
from host_check_lib import checksum, up

DESC = np.dtype([("i", "<i4", 6), ("pair0", "<i8"), ("hyp0", "<i8"), ("K1", "<f8", 4), ("K2", "<f8", 4)])
OUT, HYP = 160, 32 * 8


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return hc.build(tmp_path_factory, "host_sim3_ransac_check", pthread=True)


def _write(path, items):
    """items: (problem, dict of n_pairs / n_hyp / nulls / want overrides)"""
    with open(path, "wb") as f:
        f.write(np.array([len(items)], dtype="<i4").tobytes())
        for p, o in items:
            f.write(np.array([o.get("n_pairs", p.n_pairs), p.n_pairs, o.get("n_hyp", p.n_hyp), p.n_hyp, p.fix_scale, o.get("min_inliers", p.min_inliers),
                              o.get("best_inliers", p.best_inliers), o.get("nulls", 0), o.get("want", 1)], dtype="<i4").tobytes())
            f.write(np.concatenate([p.K1, p.K2, p.best_S12]).astype("<f8").tobytes())
            for a in (p.p1c, p.p2c, p.max_err1, p.max_err2):
                f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(p.sample, dtype="<i4").tobytes())


def _batch(shapes, seed0):
    out = []
    for k, (n, nh) in enumerate(shapes):
        p = synth.make_sim3_ransac(seed0 + k, n, k % 2, 0.2)
        out.append(p.copy(sample=synth.draw_triples(seed0 + k, n, nh) if nh else np.zeros((0, 3), dtype=np.int32), min_inliers=5 + k % 7,
                          best_inliers=k % 3, best_S12=np.arange(8.0) + k))
    return out


SHAPES = [[(0, 0)], [(3, 1)], [(7, 5), (0, 0), (33, 0)], [(64, 64), (65, 3)], [(3 + k % 5, k % 4) for k in range(300)]]   # 300: the threaded path


@pytest.mark.parametrize("want", [1, 0])
def test_offsets_packing_and_write_back(checker, tmp_path, want):
    batches = [_batch(s, 100 * k) for k, s in enumerate(SHAPES)]
    files = []
    for k, ps in enumerate(batches):
        files.append(str(tmp_path / ("b%d.rs" % k)))
        _write(files[-1], [(p, dict(want=want)) for p in ps])
    for ps, line in zip(batches, hc.run(checker, files, len(files))):
        f = hc.fields(line)
        n, n_tot, h_tot = len(ps), sum(p.n_pairs for p in ps), sum(p.n_hyp for p in ps)
        assert (f["n_tot"], f["h_tot"], f["want"]) == (n_tot, h_tot, want)
        # the arena, restated from the sizes: four upload regions, three back regions, one device-only region
        o, offs = 0, []
        for b in (DESC.itemsize * n, (6 * n_tot + 6) * 8, (2 * n_tot + 2) * 8, (3 * h_tot + 3) * 4, OUT * n, n_tot + 1, (h_tot + 1) * 4, (h_tot + 1) * HYP):
            offs.append(o)
            o += up(b)
        assert [f[k] for k in ("desc", "p", "gate", "sample", "out", "flag", "cnt", "hyp")] == offs
        hc.assert_bound(f, [(k, k) for k in ("desc", "out", "p", "gate", "sample", "hyp", "cnt", "flag")])   # RansacBatch reads every region where it is
        assert f["upload"] == offs[4] and f["back"] == offs[7] - offs[4] and f["total"] == o
        assert f["download"] == (f["back"] if want else offs[6] - offs[4])
        # the packed regions
        d = np.zeros(n, dtype=DESC)
        po = ho = 0
        for k, p in enumerate(ps):
            d[k]["i"] = [p.n_pairs, p.fix_scale, p.min_inliers, p.n_hyp, p.best_inliers, 0]
            d[k]["pair0"], d[k]["hyp0"], d[k]["K1"], d[k]["K2"] = po, ho, p.K1, p.K2
            po += p.n_pairs; ho += p.n_hyp
        assert DESC.itemsize == 104
        assert f["sum_desc"] == checksum(d)
        assert f["sum_p"] == checksum(*[np.hstack([p.p1c, p.p2c]) for p in ps])
        assert f["sum_gate"] == checksum(*[np.stack([p.max_err1, p.max_err2], axis=1) for p in ps])
        assert f["sum_sample"] == checksum(np.concatenate([p.sample.ravel() for p in ps]).astype("<i4"))
        # the write-back of the synthetic result
        hyp = [p.n_hyp > 0 for p in ps]
        hit = [h and k % 2 == 0 for k, h in enumerate(hyp)]
        best = [h and k % 3 == 0 for k, h in enumerate(hyp)]
        assert f["got_its"] == sum(range(n)) and f["got_best"] == sum(3 * k + 1 for k in range(n))
        assert f["got_S7"] == sum((k + 7) if hit[k] else -1 for k in range(n))                       # S12 untouched without a hit
        assert f["got_bestS7"] == sum((100 + k + 7) if best[k] else (7 + k) for k in range(n))     # best_S12 kept without a new best
        assert f["got_keep"] == sum(1 for b in best if not b)
        flags = np.arange(n_tot) & 1
        po, want_flag = 0, 0
        for k, p in enumerate(ps):
            want_flag += int(flags[po:po + p.n_pairs].sum()) if hit[k] else 7 * p.n_pairs          # inlier untouched without a hit
            po += p.n_pairs
        assert f["got_flag"] == want_flag
        assert f["got_cnt"] == (sum(range(h_tot)) if want else 0)


REFUSALS = [
    (dict(n_pairs=-1), "problem 1: negative n_pairs"),
    (dict(n_hyp=-2), "problem 1: negative n_hyp"),
    (dict(min_inliers=-1), "problem 1: negative min_inliers"),
    (dict(best_inliers=-5), "problem 1: negative best_inliers"),
    (dict(nulls=1), "problem 1: NULL array with n_pairs > 0"),
    (dict(nulls=2), "problem 1: NULL array with n_pairs > 0"),
    (dict(nulls=4), "problem 1: NULL problem or result"),
    (dict(nulls=16), "problem 1: NULL problem or result"),
    (dict(nulls=8), "problem 1: NULL sample with n_hyp > 0"),
    (dict(small=True), "problem 1: n_pairs < 3 with n_hyp > 0"),
    (dict(sample=(4, 2, 9)), "problem 1: hypothesis 4: sample index out of range"),
    (dict(sample=(0, 0, -1)), "problem 1: hypothesis 0: sample index out of range"),
    (dict(K=np.inf), "problem 1: K1 / K2 is not finite"),
    (dict(point=(5, np.nan)), "problem 1: pair 5: a point is not finite"),
    (dict(gate=(8, np.inf)), "problem 1: pair 8: a gate is not finite"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m.split(": ", 1)[1].replace(" ", "_") + str(k) for k, (_, m) in enumerate(REFUSALS)])
def test_refusals(checker, tmp_path, change, message):
    good, bad = _batch([(9, 6), (9, 6)], 40)
    o = {k: v for k, v in change.items() if k in ("n_pairs", "n_hyp", "min_inliers", "best_inliers", "nulls")}
    if "small" in change:
        bad = synth.make_sim3_ransac(1, 2, 0, 0.0).copy(sample=np.zeros((1, 3), dtype=np.int32))
    if "sample" in change:
        h, j, v = change["sample"]
        s = bad.sample.copy(); s[h, j] = v
        bad = bad.copy(sample=s)
    if "K" in change:
        bad = bad.copy(K2=np.array([1.0, change["K"], 1.0, 1.0]))
    if "point" in change:
        a = bad.p2c.copy(); a[change["point"][0], 1] = change["point"][1]
        bad = bad.copy(p2c=a)
    if "gate" in change:
        a = bad.max_err1.copy(); a[change["gate"][0]] = change["gate"][1]
        bad = bad.copy(max_err1=a)
    path = str(tmp_path / "r.rs")
    _write(path, [(good, {}), (bad, o)])
    assert hc.run(checker, [path], 1) == ["error " + message]


def test_legal_edges(checker, tmp_path):
    """n_hyp == 0, n_pairs < min_inliers, no pairs at all, hyp_inliers == NULL beside a caller that wants the counts"""
    a, b, c = _batch([(5, 0), (4, 3), (0, 0)], 7)
    path = str(tmp_path / "e.rs")
    _write(path, [(a, dict(want=0)), (b, dict(min_inliers=50)), (c, dict(want=0))])
    f = hc.fields(hc.run(checker, [path], 1)[0])
    assert f["want"] == 1 and f["download"] == f["back"] and f["got_cnt"] == 0 + 1 + 2
