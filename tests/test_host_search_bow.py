"""The host half of vba_search_by_bow (mc_slam_amd/csrc/vba_host_search_bow.h, vba_host_arena.h: refusals, arena offsets, the node join
with its query order, ranks and candidate ranges, the packed records, and the write-back with match21, histogram, maxima and drop)
under AddressSanitizer + UBSan (CPU only, a stand-alone program, nothing preloaded).  The harness (tests/host_search_bow_check.cpp)
packs into heap blocks of exactly the arena's sizes; every expected offset below is restated from the sizes alone, the packed regions
are compared with records built in NumPy through an order-sensitive checksum, and the write-back of a synthetic device result is
restated here in Python."""
import numpy as np
import pytest

from mc_slam_amd import abi, synth
import search_bow_cases as cases_mod
import search_bow_ref as ref_mod
import host_check_lib as hc
from host_check_lib import checksum, up

DESC = np.dtype([("off", "<i8", 3), ("i", "<i4", 5), ("nn_ratio", "<f4")])
QUERY = np.dtype([("idx1", "<i4"), ("c_begin", "<i4"), ("c_end", "<i4"), ("rank", "<i4")])
KF_FRAME, KF_KF = abi.SEARCH_BOW_KF_FRAME, abi.SEARCH_BOW_KF_KF


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return hc.build(tmp_path_factory, "host_search_bow_check", pthread=True)


def _or(a, n, dtype):
    return np.zeros(n, dtype=dtype) if a is None else a.astype(dtype)


def _write(path, items):
    """items: (pair, dict of mode / n_keys1 / n_keys2 / n_nodes1 / n_nodes2 / nulls overrides)"""
    with open(path, "wb") as f:
        f.write(np.array([len(items)], dtype="<i4").tobytes())
        for p, o in items:
            n1, n2 = p.n_keys1, p.n_keys2
            f.write(np.array([o.get("mode", p.mode), int(p.check_orientation), p.th_low, o.get("n_keys1", n1), n1, o.get("n_keys2", n2), n2,
                              o.get("n_nodes1", p.n_nodes1), p.n_nodes1, o.get("n_nodes2", p.n_nodes2), p.n_nodes2, len(p.node_feat1), len(p.node_feat2),
                              o.get("nulls", 0)], dtype="<i4").tobytes())
            f.write(np.array([p.nn_ratio], dtype="<f4").tobytes())
            f.write(p.desc1.tobytes()); f.write(p.desc2.tobytes()); f.write(p.good_mp1.tobytes()); f.write(_or(p.good_mp2, n2, "u1").tobytes())
            f.write(_or(p.angle1, n1, "<f4").tobytes()); f.write(_or(p.angle2, n2, "<f4").tobytes())
            f.write(p.node_id1.astype("<u4").tobytes()); f.write(p.node_begin1.astype("<i4").tobytes()); f.write(p.node_feat1.astype("<i4").tobytes())
            f.write(p.node_id2.astype("<u4").tobytes()); f.write(p.node_begin2.astype("<i4").tobytes()); f.write(p.node_feat2.astype("<i4").tobytes())


def join(p):
    """the node join restated: the query records in walk order, the roles, the largest number of queries in one node"""
    q, most = [], 0
    role = np.where(p.good_mp1 != 0, 2, 1).astype("u1")
    for a, b in ref_mod.shared_nodes(p):
        rank = 0
        for idx1 in p.node_feat1[p.node_begin1[a]:p.node_begin1[a + 1]]:
            if role[idx1] == 1:
                continue
            role[idx1] = 0
            q.append((idx1, p.node_begin2[b], p.node_begin2[b + 1], rank))
            rank += 1
        most = max(most, rank)
    return np.array(q, dtype=QUERY), role, most


def _batches():
    C = cases_mod.cases()
    r = np.random.default_rng(3)
    many = [synth.search_bow_scene(700 + k, k % 2, n_keys1=(k * 5) % 23, n_keys2=(k * 7) % 19 * (k % 3 > 0), n_nodes=1 + k % 4,
                                   check_orientation=bool(k % 4 < 2), th_low=int(r.integers(0, 256))) for k in range(300)]   # the threaded path
    small = [n for n in C if n != "max_keys"]
    return [[C["micro"]], [C["empty_keys1"]], [C["states"], C["one_sided_nodes"]],
            [C["queries_257"], C["empty_keys2"], C["queries_513"], C["no_shared_node"], C["queries_256"], C["orientation_drop"], C["bad_mp2_kf"]],
            [C[n] for n in small], many]


def replay(ps):
    """the write-back of the harness's synthetic device result, restated: the sums the harness prints"""
    s = dict.fromkeys(("match", "before", "rounds", "m12", "bi", "bd", "bd2", "st", "bin", "m21", "hist", "ind"), 0)
    i0 = 0
    for k, p in enumerate(ps):
        n1, n2 = p.n_keys1, p.n_keys2
        role = join(p)[1]
        i = np.arange(i0, i0 + n1)
        i0 += n1
        isq = role == 0
        bi = np.where(isq, (5 * i) % n2 if n2 else -1, -1)
        bd = np.where(isq, i % 257, 256)
        bd2 = np.where(isq, (3 * i) % 257, 256)
        st = np.where(isq, np.where((i % 3 == 0) & (n2 > 0), 0, 3 + i % 2), role)
        m12, m21 = np.full(n1, -1), np.full(n2, -1)
        bins = np.full(n1, 255)
        hist = np.zeros(30, dtype=int)
        n = 0
        for j in range(n1):
            if st[j] == 0:
                m12[j] = bi[j]
                m21[bi[j]] = j
                n += 1
                if p.check_orientation:
                    bins[j] = ref_mod.rot_bin(p.angle1[j], p.angle2[bi[j]])
                    hist[bins[j]] += 1
        before, ind = n, (-1, -1, -1)
        if p.check_orientation:
            ind = ref_mod.three_maxima(hist)
            for j in range(n1):
                if bins[j] != 255 and bins[j] not in ind:
                    m21[m12[j]], m12[j], st[j] = -2, -1, 5
                    n -= 1
        j = np.arange(n1)
        s["match"] += n * (k + 1); s["before"] += before * (k + 1); s["rounds"] += (k + 1) * (k + 1)
        s["hist"] += int((hist * (np.arange(30) + 1)).sum()) * (k + 1); s["ind"] += sum(v * (b + 1) for b, v in enumerate(ind)) * (k + 1)
        s["m12"] += int((m12 * (j % 13 + 1)).sum()); s["bi"] += int(bi.sum()); s["bd"] += int(bd.sum()); s["bd2"] += int(bd2.sum())
        s["st"] += int((st * (j % 5 + 1)).sum()); s["bin"] += int((bins * (j % 7 + 1)).sum()); s["m21"] += int((m21 * (np.arange(n2) % 11 + 1)).sum())
    return s


def test_offsets_join_packing_and_write_back(checker, tmp_path):
    batches = _batches()
    files = []
    for k, ps in enumerate(batches):
        files.append(str(tmp_path / ("b%d.sb" % k)))
        _write(files[-1], [(p, {}) for p in ps])
    dropped = ranked = 0
    for ps, line in zip(batches, hc.run(checker, files, len(files))):
        f = hc.fields(line)
        n = len(ps)
        k1, k2, ft = sum(p.n_keys1 for p in ps), sum(p.n_keys2 for p in ps), sum(len(p.node_feat2) for p in ps)
        mk = max(p.n_keys2 for p in ps)
        assert (f["k1"], f["k2"], f["feat_tot"], f["max_keys2"], f["lds"], f["grid"]) == (k1, k2, ft, mk, 4 * (mk + 1), n)
        # the arena, restated from the sizes: seven upload regions, five back regions, one that stays on the device
        assert DESC.itemsize == 48 and QUERY.itemsize == 16
        o, offs = 0, []
        for b in (48 * n, 32 * (k1 + 1), 32 * (k2 + 1), k1 + 1, k2 + 1, 16 * (k1 + 1), 4 * (ft + 1),
                  4 * (n + 1), 4 * (k1 + 1), 2 * (k1 + 1), 2 * (k1 + 1), k1 + 1, 4 * (k1 + 1)):
            offs.append(o)
            o += up(b)
        names = ("desc", "key1", "key2", "role", "blocked", "query", "feat", "rounds", "best_idx", "best_dist", "best_dist2", "state", "prev")
        assert [f[k] for k in names] == offs
        hc.assert_bound(f, [(k, k) for k in names])
        assert f["upload"] == offs[7] and f["back"] == offs[12] - offs[7] and f["total"] == o
        # the join and the records
        d = np.zeros(n, dtype=DESC)
        joins = [join(p) for p in ps]
        o1 = o2 = of = 0
        for k, (p, (q, role, most)) in enumerate(zip(ps, joins)):
            d[k]["off"] = [o1, o2, of]
            d[k]["i"] = [p.n_keys1, p.n_keys2, len(q), most, p.th_low - 1 if p.kf_kf else p.th_low]
            d[k]["nn_ratio"] = p.nn_ratio
            o1 += p.n_keys1; o2 += p.n_keys2; of += len(p.node_feat2)
            ranked += int(most > 1)
            assert most == ref_mod.queries(p)[1] and [int(x) for x in q["idx1"]] == [a for a, _, _ in ref_mod.queries(p)[0]]
        assert f["n_q"] == sum(len(q) for q, _, _ in joins)
        assert f["sum_desc"] == checksum(d)
        assert f["sum_key1"] == checksum(*[p.desc1 for p in ps]) and f["sum_key2"] == checksum(*[p.desc2 for p in ps])
        assert f["sum_role"] == checksum(*[role for _, role, _ in joins])
        assert f["sum_blocked"] == checksum(*[((p.good_mp2 == 0) if p.kf_kf else np.zeros(p.n_keys2, dtype=bool)).astype("u1") for p in ps])
        assert f["sum_query"] == checksum(*[q for q, _, _ in joins])
        assert f["sum_feat"] == checksum(*[p.node_feat2 for p in ps])
        # the write-back on the synthetic result of the harness
        s = replay(ps)
        assert (f["got_match"], f["got_before"], f["got_status"], f["got_rounds"]) == (s["match"], s["before"], 0, s["rounds"])
        assert (f["got_m12"], f["got_bi"], f["got_bd"], f["got_bd2"]) == (s["m12"], s["bi"], s["bd"], s["bd2"])
        assert (f["got_st"], f["got_bin"], f["got_m21"], f["got_hist"], f["got_ind"]) == (s["st"], s["bin"], s["m21"], s["hist"], s["ind"])
        dropped += s["before"] - s["match"]
    assert dropped > 50 and ranked > 20            # the drop of the orientation filter ran; nodes held several queries


def test_join_by_hand(checker, tmp_path):
    """one_sided_nodes: the two shared nodes 5 and 9 yield the queries (keypoint 1, candidates [2, 3), rank 0) and (keypoint 4, [3, 4),
    rank 0); states: node 5 yields keypoints 0, 3, 4 with the ranks 0, 1, 2 over the candidates [0, 3), keypoint 1 has role 1,
    keypoints 2 and 5 the roles 2 and 1"""
    C = cases_mod.cases()
    q, role, most = join(C["one_sided_nodes"])
    assert q.tolist() == [(1, 2, 3, 0), (4, 3, 4, 0)] and role.tolist() == [2, 0, 2, 2, 0, 2] and most == 1
    q, role, most = join(C["states"])
    assert q.tolist() == [(0, 0, 3, 0), (3, 0, 3, 1), (4, 0, 3, 2)] and role.tolist() == [0, 1, 2, 0, 0, 1] and most == 3
    path = str(tmp_path / "j.sb")
    _write(path, [(C["one_sided_nodes"], {}), (C["states"], {})])
    f = hc.fields(hc.run(checker, [path], 1)[0])
    assert f["n_q"] == 5 and f["sum_query"] == checksum(np.array([(1, 2, 3, 0), (4, 3, 4, 0), (0, 0, 3, 0), (3, 0, 3, 1), (4, 0, 3, 2)], dtype=QUERY))


def test_write_back_by_hand(checker, tmp_path):
    """three queries (the keypoints 0, 1 and 3 of side 1; keypoint 2 sits in a node side 2 does not list) against three keypoints: the
    synthetic result matches the keypoints 0 and 3 (multiples of 3), both on 5 i mod 3 = 0: the later one is what match21 keeps.
    Their angles put them into the bins 3 and 0; with two bins filled both are kept"""
    p = cases_mod.pair(KF_FRAME, [(1, 0, 1), (2, 0, 1), (3, 0, 1), (4, 0, 1)], [(1, 0, 1), (2, 0, 1), (4, 0, 1)], angle1=[100, 0, 0, 10], angle2=[10, 10, 10])
    path = str(tmp_path / "h.sb")
    _write(path, [(p, {})])
    f = hc.fields(hc.run(checker, [path], 1)[0])
    # match12 = [0, -1, -1, 0] with the weights 1 .. 4; match21 = [3, -1, -1] with the weights 1 .. 3; states 0, 4, 2, 0
    assert (f["n_q"], f["got_match"], f["got_before"], f["got_m12"], f["got_m21"], f["got_hist"]) == (3, 2, 2, 0 - 2 - 3 + 0, 3 - 2 - 3, 1 + 4)
    assert f["got_st"] == 0 * 1 + 4 * 2 + 2 * 3 + 0 * 4 and f["got_ind"] == 0 * 1 + 3 * 2 - 1 * 3 and f["got_bin"] == 3 * 1 + 255 * 2 + 255 * 3 + 0 * 4


def _with(p, **kw):
    """a copy of p with single entries of its arrays replaced: name=(index, value)"""
    ch = {}
    for k, (i, v) in kw.items():
        a = getattr(p, k).copy()
        a.reshape(-1)[i] = v
        ch[k] = a
    return p.copy(**ch)


# (mode, change, message)
REFUSALS = [
    (KF_FRAME, dict(n_keys1=-1), "negative n_keys"),
    (KF_KF, dict(n_keys2=-2), "negative n_keys"),
    (KF_FRAME, dict(mode=2), "unknown mode"),
    (KF_KF, dict(mode=-1), "unknown mode"),
    (KF_FRAME, dict(nulls=4), "NULL problem or result"),
    (KF_KF, dict(nulls=16), "NULL problem or result"),
    (KF_FRAME, dict(nulls=1), "NULL array with n_keys1 > 0"),
    (KF_KF, dict(nulls=256), "NULL array with n_keys1 > 0"),
    (KF_FRAME, dict(nulls=2), "NULL array with n_keys1 > 0"),
    (KF_KF, dict(nulls=32), "NULL array with n_keys1 > 0"),
    (KF_FRAME, dict(nulls=2048), "NULL array with n_keys1 > 0"),
    (KF_FRAME, dict(nulls=32768), "NULL array with n_keys1 > 0"),
    (KF_FRAME, dict(nulls=8), "NULL array with n_keys2 > 0"),
    (KF_KF, dict(nulls=512), "NULL array with n_keys2 > 0"),
    (KF_KF, dict(nulls=1024), "NULL array with n_keys2 > 0"),
    (KF_FRAME, dict(nulls=4096), "NULL angles with check_orientation"),
    (KF_KF, dict(nulls=8192), "NULL angles with check_orientation"),
    (KF_FRAME, dict(copy=dict(th_low=256)), "th_low outside 0 .. 255"),
    (KF_KF, dict(copy=dict(th_low=-1)), "th_low outside 0 .. 255"),
    (KF_FRAME, dict(copy=dict(nn_ratio=np.nan)), "nn_ratio is not finite"),
    (KF_KF, dict(copy=dict(nn_ratio=np.inf)), "nn_ratio is not finite"),
    (KF_FRAME, dict(edit=dict(angle1=(3, 360.0))), "keypoint 3 of keyframe 1: angle outside [0, 360)"),
    (KF_KF, dict(edit=dict(angle2=(2, np.nan))), "keypoint 2 of keyframe 2: angle outside [0, 360)"),
    (KF_KF, dict(edit=dict(angle1=(4, -1.0))), "keypoint 4 of keyframe 1: angle outside [0, 360)"),
    (KF_FRAME, dict(n_nodes1=-1), "negative n_nodes of keyframe 1"),
    (KF_FRAME, dict(nulls=64), "NULL node_begin of keyframe 1"),
    (KF_KF, dict(nulls=16384), "NULL node_id of keyframe 2"),
    (KF_KF, dict(nulls=128), "NULL node_feat of keyframe 2"),
    (KF_FRAME, dict(edit=dict(node_begin2=(0, 1))), "node_begin of keyframe 2 does not start at 0"),
    (KF_KF, dict(edit=dict(node_id1=(2, 0))), "node_id of keyframe 1 is not strictly ascending at node 2"),
    (KF_FRAME, dict(same_id=1), "node_id of keyframe 2 is not strictly ascending at node 1"),
    (KF_KF, dict(edit=dict(node_begin1=(2, -1))), "node_begin of keyframe 1 decreases at node 1"),
    (KF_FRAME, dict(edit=dict(node_feat1=(4, 40))), "node_feat of keyframe 1 entry 4: keypoint index out of range"),
    (KF_KF, dict(edit=dict(node_feat2=(0, -1))), "node_feat of keyframe 2 entry 0: keypoint index out of range"),
    (KF_KF, dict(dup=1), "node_feat of keyframe 2 entry 9: keypoint K listed twice"),
    (KF_FRAME, dict(big=1), "n_keys2 above 16384: the claim table of side 2 lives in LDS"),
]


@pytest.mark.parametrize("mode,change,message", REFUSALS, ids=[m.replace(" ", "_").replace("/", "").replace(":", "") + str(k) for k, (_, _, m) in enumerate(REFUSALS)])
def test_refusals(checker, tmp_path, mode, change, message):
    good, bad = synth.search_bow_scene(40, mode, n_keys1=40, n_keys2=40, n_nodes=4), synth.search_bow_scene(41, mode, n_keys1=40, n_keys2=40, n_nodes=4)
    assert len(bad.node_feat2) > 10 and bad.n_nodes1 > 3 and bad.n_nodes2 > 3
    o = {k: v for k, v in change.items() if k in ("mode", "n_keys1", "n_keys2", "n_nodes1", "n_nodes2", "nulls")}
    if "edit" in change:
        bad = _with(bad, **change["edit"])
    if "copy" in change:
        bad = bad.copy(**change["copy"])
    if "same_id" in change:
        a = bad.node_id2.copy()
        a[1] = a[0]
        bad = bad.copy(node_id2=a)
    if "dup" in change:
        a = bad.node_feat2.copy()
        a[9] = a[2]
        message = message.replace("K", str(a[2]))
        bad = bad.copy(node_feat2=a)
    if "big" in change:
        bad = synth.search_bow_scene(42, mode, n_keys1=3, n_keys2=abi.SEARCH_BOW_MAX_KEYS + 1, n_nodes=4, twins=0.0)
    path = str(tmp_path / "r.sb")
    _write(path, [(good, {}), (bad, o)])
    assert hc.run(checker, [path], 1) == ["error pair 1: " + message]


def test_legal_edges(checker, tmp_path):
    """a pair without keypoints on side 1 needs no arrays of side 1 and no per-keypoint results, one without keypoints on side 2 no
    arrays of side 2 and no match21; good_mp2 is NULL in KF_FRAME mode (the harness passes it so); without check_orientation no
    angles are needed and none is checked; th_low 0 and 255 are legal; a side 2 of exactly 16384 keypoints is legal; a pair without
    a shared node is legal"""
    C = cases_mod.cases()
    e1 = C["empty_keys1"]
    e2 = C["empty_keys2"].copy(th_low=255)
    b = synth.search_bow_scene(8, KF_KF, n_keys1=30, n_keys2=10, n_nodes=3, check_orientation=False, th_low=0)
    m = C["max_keys"]
    path = str(tmp_path / "e.sb")
    _write(path, [(e1, dict(nulls=1 | 2 | 32 | 256 | 2048 | 4096 | 32768)), (e2, dict(nulls=8 | 512 | 1024 | 8192)), (b, dict(nulls=4096 | 8192)),
                  (C["no_shared_node"], {}), (m, {})])
    f = hc.fields(hc.run(checker, [path], 1)[0])
    assert (f["k1"], f["k2"], f["grid"], f["max_keys2"], f["lds"]) == (0 + 40 + 30 + 2 + 96, 40 + 0 + 10 + 2 + 16384, 5, 16384, 65540)
    assert f["got_status"] == 0
