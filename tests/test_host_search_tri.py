"""The host half of vba_search_triangulation (mc_slam_amd/csrc/vba_host_search_tri.h, vba_host_arena.h: refusals, arena offsets, the
node join with its query list, the interleaved keypoint records, write-back with vMatchedPairs) under AddressSanitizer + UBSan
(CPU only).  The harness (tests/host_search_tri_check.cpp) packs into heap blocks of exactly the arena's sizes; every expected
offset below is restated from the sizes alone, the packed regions are compared with records built in NumPy through an
order-sensitive checksum, and the query list with the yardstick's node join (tests/search_tri_ref.py)."""
import numpy as np
import pytest

from mc_slam_amd import synth
import search_tri_cases as cases_mod
import search_tri_ref as ref_mod
import host_check_lib as hc
from host_check_lib import checksum, up

DESC = np.dtype([("off", "<i8", 4), ("i", "<i4", 6), ("c", "<f8", 13)])
KEY = np.dtype([("d", "u1", 32), ("u", "<f8"), ("v", "<f8"), ("angle", "<f4"), ("oct", "u1"), ("role", "u1"), ("pad", "u1", 10)])
OUT_BYTES = 144


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return hc.build(tmp_path_factory, "host_search_tri_check", pthread=True)


def consts(p):
    return np.concatenate([p.F12.ravel(), p.epipole, [p.chi2_epi, p.epipole_r2]])


def _write(path, items):
    """items: (problem, dict of n_keys1 / n_keys2 / n_nodes1 / n_nodes2 / n_levels2 / nulls overrides)"""
    with open(path, "wb") as f:
        f.write(np.array([len(items)], dtype="<i4").tobytes())
        for p, o in items:
            f.write(np.array([o.get("n_keys1", p.n_keys1), p.n_keys1, o.get("n_keys2", p.n_keys2), p.n_keys2, o.get("n_nodes1", len(p.node_id1)), len(p.node_id1),
                              len(p.node_feat1), o.get("n_nodes2", len(p.node_id2)), len(p.node_id2), len(p.node_feat2), o.get("n_levels2", p.n_levels2), p.n_levels2, p.th_low, int(p.check_orientation),
                              o.get("nulls", 0)], dtype="<i4").tobytes())
            f.write(consts(p).astype("<f8").tobytes())
            for s in "12":
                g = lambda k: getattr(p, k + s)
                f.write(g("desc").tobytes()); f.write(g("has_mp").tobytes()); f.write(g("uv").astype("<f8").tobytes()); f.write(g("angle").astype("<f4").tobytes())
                f.write(g("node_id").astype("<u4").tobytes()); f.write(g("node_begin").astype("<i4").tobytes()); f.write(g("node_feat").astype("<i4").tobytes())
            f.write(p.oct2.tobytes())
            f.write(p.level_sigma2_2.astype("<f8").tobytes()); f.write(p.scale_2.astype("<f8").tobytes())


def keys1(p, queries):
    k = np.zeros(p.n_keys1, dtype=KEY)
    k["d"], k["u"], k["v"] = p.desc1, p.uv1[:, 0], p.uv1[:, 1]
    k["angle"] = p.angle1 if p.check_orientation else 0
    k["role"] = np.where(p.has_mp1 != 0, 1, 2)
    k["role"][[q[0] for q in queries]] = 0
    return k


def keys2(p):
    k = np.zeros(p.n_keys2, dtype=KEY)
    k["d"], k["u"], k["v"], k["oct"], k["role"] = p.desc2, p.uv2[:, 0], p.uv2[:, 1], p.oct2, p.has_mp2 != 0
    k["angle"] = p.angle2 if p.check_orientation else 0
    return k


def _batches():
    C = cases_mod.cases()
    many = [synth.synth_match_pair(500 + k, n_true=(k * 7) % 5 * (k % 3), n_distract1=k % 4, n_distract2=(k + 1) % 3, n_nodes=1 + k % 3,
                                   n_levels=1 + k % 8, check_orientation=bool(k % 2)) for k in range(300)]   # the threaded path, a third without true pairs
    return [[C["empty1"]], [C["micro"]], [C["jumps"], C["empty2"], C["big_node"], C["no_shared"], C["synth_3_levels"]], list(C.values()), many]


def test_offsets_join_packing_and_write_back(checker, tmp_path):
    batches = _batches()
    files = []
    for k, ps in enumerate(batches):
        files.append(str(tmp_path / ("b%d.st" % k)))
        _write(files[-1], [(p, {}) for p in ps])
    for ps, line in zip(batches, hc.run(checker, files, len(files))):
        f = hc.fields(line)
        n = len(ps)
        k1, k2 = sum(p.n_keys1 for p in ps), sum(p.n_keys2 for p in ps)
        ft, lv = sum(len(p.node_feat2) for p in ps), sum(2 * p.n_levels2 for p in ps)
        assert (f["k1"], f["k2"], f["feat_tot"], f["lev_tot"]) == (k1, k2, ft, lv)
        # the arena, restated from the sizes: six upload regions, four back regions, nothing device-only
        o, offs = 0, []
        for b in (DESC.itemsize * n, 64 * (k1 + 1), 64 * (k2 + 1), 16 * (k1 + 1), 4 * (ft + 1), 8 * (lv + 1), OUT_BYTES * n, 4 * (k1 + 1), k1 + 1, k1 + 1):
            offs.append(o)
            o += up(b)
        assert [f[k] for k in ("desc", "key1", "key2", "query", "feat", "lev", "out", "match12", "best_dist", "state")] == offs
        hc.assert_bound(f, [(k, k) for k in ("desc", "key1", "key2", "query", "feat", "lev", "out", "match12", "best_dist", "state")])   # StBatch reads every region where it is
        assert f["upload"] == offs[6] and f["back"] == o - offs[6] and f["total"] == o
        # the join against the yardstick's, and the packed regions
        joins = [ref_mod.node_join(p) for p in ps]
        q = [np.array([(a, b, e, 0) for a, b, e in j], dtype="<i4").reshape(-1, 4) for j in joins]
        assert f["n_q"] == sum(len(j) for j in joins) and f["sum_query"] == checksum(*q)
        assert DESC.itemsize == 160 and KEY.itemsize == 64
        d = np.zeros(n, dtype=DESC)
        o1 = o2 = of = ol = 0
        for k, p in enumerate(ps):
            d[k]["off"] = [o1, o2, of, ol]
            d[k]["i"] = [p.n_keys1, p.n_keys2, len(joins[k]), p.n_levels2, p.th_low, int(p.check_orientation)]
            d[k]["c"] = consts(p)
            o1 += p.n_keys1; o2 += p.n_keys2; of += len(p.node_feat2); ol += 2 * p.n_levels2
        assert f["sum_desc"] == checksum(d)
        assert f["sum_key1"] == checksum(*[keys1(p, j) for p, j in zip(ps, joins)])
        assert f["sum_key2"] == checksum(*[keys2(p) for p in ps])
        assert f["sum_feat"] == checksum(*[p.node_feat2 for p in ps])
        assert f["sum_lev"] == checksum(*[np.concatenate([p.level_sigma2_2, p.scale_2]) for p in ps])
        # the write-back of the synthetic result (see the harness)
        i = np.arange(k1)
        m12 = i % 5 - 1
        got_n = got_pairs = got_hist = got_ind = 0
        o1 = 0
        for k, p in enumerate(ps):
            m = m12[o1:o1 + p.n_keys1]
            sel = np.nonzero(m >= 0)[0]
            got_n += len(sel) * (k + 1) + 2 * k
            got_pairs += int((3 * sel + m[sel]).sum())
            got_hist += 30 * k + sum(range(30))
            got_ind += 2 * k
            o1 += p.n_keys1
        assert (f["got_n"], f["got_status"], f["got_pairs"], f["got_hist"], f["got_ind"]) == (got_n, 0, got_pairs, got_hist, got_ind)
        assert (f["got_m12"], f["got_bd"], f["got_st"]) == (int(m12.sum()), int((i % 251).sum()), int((i % 5).sum()))


def _with(p, **kw):
    """a copy of p with single entries of its arrays replaced: name=(index, value)"""
    ch = {}
    for k, (i, v) in kw.items():
        a = getattr(p, k).copy()
        a.reshape(-1)[i] = v
        ch[k] = a
    return p.copy(**ch)


REFUSALS = [
    (dict(n_keys1=-1), "pair 1: negative n_keys"),
    (dict(n_keys2=-2), "pair 1: negative n_keys"),
    (dict(nulls=4), "pair 1: NULL problem or result"),
    (dict(nulls=16), "pair 1: NULL problem or result"),
    (dict(nulls=1024), "pair 1: NULL array with n_keys1 > 0"),
    (dict(nulls=2), "pair 1: NULL array with n_keys1 > 0"),
    (dict(nulls=32), "pair 1: NULL array with n_keys1 > 0"),
    (dict(nulls=1), "pair 1: NULL array with n_keys2 > 0"),
    (dict(nulls=2048), "pair 1: NULL array with n_keys2 > 0"),
    (dict(nulls=64), "pair 1: NULL angles with check_orientation"),
    (dict(nulls=8), "pair 1: NULL level table"),
    (dict(n_nodes1=-1), "pair 1: negative n_nodes of keyframe 1"),
    (dict(n_nodes2=-4), "pair 1: negative n_nodes of keyframe 2"),
    (dict(nulls=128), "pair 1: NULL node_begin of keyframe 1"),
    (dict(nulls=256), "pair 1: NULL node_id of keyframe 2"),
    (dict(nulls=512), "pair 1: NULL node_feat of keyframe 2"),
    (dict(n_levels2=0), "pair 1: n_levels2 outside 1 .. 64"),
    (dict(n_levels2=65), "pair 1: n_levels2 outside 1 .. 64"),
    (dict(copy=dict(th_low=256)), "pair 1: th_low outside 0 .. 255"),
    (dict(copy=dict(th_low=-1)), "pair 1: th_low outside 0 .. 255"),
    (dict(edit=dict(oct2=(6, 8))), "pair 1: keypoint 6 of keyframe 2: octave >= n_levels2"),
    (dict(edit=dict(uv1=(11, np.nan))), "pair 1: keypoint 5 of keyframe 1: a pixel is not finite"),
    (dict(edit=dict(uv2=(0, np.inf))), "pair 1: keypoint 0 of keyframe 2: a pixel is not finite"),
    (dict(edit=dict(F12=(4, np.nan))), "pair 1: F12 is not finite"),
    (dict(edit=dict(epipole=(1, -np.inf))), "pair 1: the epipole is not finite"),
    (dict(copy=dict(chi2_epi=np.nan)), "pair 1: a threshold is not finite"),
    (dict(copy=dict(epipole_r2=np.inf)), "pair 1: a threshold is not finite"),
    (dict(edit=dict(level_sigma2_2=(7, np.nan))), "pair 1: a level table is not finite"),
    (dict(edit=dict(scale_2=(0, np.inf))), "pair 1: a level table is not finite"),
    (dict(edit=dict(node_id1=(2, 5))), "pair 1: node_id of keyframe 1 is not strictly ascending at node 2"),
    (dict(edit=dict(node_id2=(3, 0))), "pair 1: node_id of keyframe 2 is not strictly ascending at node 3"),
    (dict(edit=dict(node_begin1=(0, 1))), "pair 1: node_begin of keyframe 1 does not start at 0"),
    (dict(edit=dict(node_begin2=(2, 0))), "pair 1: node_begin of keyframe 2 decreases at node 1"),
    (dict(edit=dict(node_feat1=(4, 80))), "pair 1: node_feat of keyframe 1 entry 4: keypoint index out of range"),
    (dict(edit=dict(node_feat2=(0, -1))), "pair 1: node_feat of keyframe 2 entry 0: keypoint index out of range"),
    (dict(dup=1), "pair 1: node_feat of keyframe 1 entry 9: keypoint K listed twice"),
    (dict(dup=2), "pair 1: node_feat of keyframe 2 entry 9: keypoint K listed twice"),
    (dict(edit=dict(angle1=(3, 360.0))), "pair 1: keypoint 3 of keyframe 1: angle outside [0, 360)"),
    (dict(edit=dict(angle2=(7, -0.5))), "pair 1: keypoint 7 of keyframe 2: angle outside [0, 360)"),
    (dict(edit=dict(angle2=(7, np.nan))), "pair 1: keypoint 7 of keyframe 2: angle outside [0, 360)"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m.split(": ", 1)[1].replace(" ", "_").replace("/", "") + str(k) for k, (_, m) in enumerate(REFUSALS)])
def test_refusals(checker, tmp_path, change, message):
    good, bad = synth.synth_match_pair(40), synth.synth_match_pair(41)
    o = {k: v for k, v in change.items() if k in ("n_keys1", "n_keys2", "n_nodes1", "n_nodes2", "n_levels2", "nulls")}
    if "edit" in change:
        bad = _with(bad, **change["edit"])
    if "copy" in change:
        bad = bad.copy(**change["copy"])
    if "dup" in change:
        name = "node_feat%d" % change["dup"]
        a = getattr(bad, name).copy()
        a[9] = a[2]
        message = message.replace("K", str(a[2]))
        bad = bad.copy(**{name: a})
    path = str(tmp_path / "r.st")
    _write(path, [(good, {}), (bad, o)])
    assert hc.run(checker, [path], 1) == ["error " + message]


def test_legal_edges(checker, tmp_path):
    """angles are not read without check_orientation (NULL and out of range are fine); a pair without keypoints needs no arrays;
    64 levels and octave 63 are legal; th_low 0 and 255 are legal"""
    a = synth.synth_match_pair(7, check_orientation=False)
    a = _with(a, angle1=(0, 720.0)).copy(th_low=255)
    e = cases_mod.cases()["empty1"]
    s = 1.01 ** np.arange(64)
    b = synth.synth_match_pair(8).copy(level_sigma2_2=s * s, scale_2=s, th_low=0)
    b = _with(b, oct2=(5, 63))
    path = str(tmp_path / "e.st")
    _write(path, [(a, dict(nulls=64)), (e, dict(nulls=2 | 32 | 1024)), (b, {})])
    f = hc.fields(hc.run(checker, [path], 1)[0])
    assert (f["k1"], f["lev_tot"]) == (a.n_keys1 + b.n_keys1, 16 + 16 + 128)
