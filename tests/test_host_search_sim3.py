"""The host half of vba_search_by_sim3 (mc_slam_amd/csrc/vba_host_search_sim3.h, vba_host_arena.h: refusals, arena offsets, the tile
table, the two direction descriptors of a pair, the keypoint records, the compacted query records, the grid copies, the write-back
with the agreement loop) under AddressSanitizer + UBSan (CPU only).  The harness (tests/host_search_sim3_check.cpp) is a stand-alone
program and packs into heap blocks of exactly the arena's sizes; every expected offset below is restated from the sizes alone and
the packed regions are compared with records built in NumPy through an order-sensitive checksum."""
import numpy as np
import pytest

from mc_slam_amd import synth
import search_sim3_cases as cases_mod
import search_sim3_ref as ref_mod
import host_check_lib as hc
from host_check_lib import checksum, up

DIR = np.dtype([("off", "<i8", 5), ("i", "<i4", 8), ("c", "<f8", 36)])
KEY = np.dtype([("d", "u1", 32), ("u", "<f8"), ("v", "<f8"), ("oct", "u1"), ("pad", "u1", 15)])
QUERY = np.dtype([("d", "u1", 32), ("pos", "<f8", 3), ("dist", "<f8", 3), ("idx", "<i4"), ("pad", "<i4", 3)])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return hc.build(tmp_path_factory, "host_search_sim3_check", pthread=True)


def _write_kf(f, kf, o):
    f.write(np.array([o.get("n_keys", kf.n_keys), kf.n_keys, o.get("n_levels", kf.n_levels), kf.n_levels, o.get("grid_cols", kf.grid_cols),
                      o.get("grid_rows", kf.grid_rows), len(kf.cell_begin), len(kf.cell_feat)], dtype="<i4").tobytes())
    f.write(np.concatenate([kf.Rcw.ravel(), kf.tcw, kf.bounds, [kf.log_scale_factor, kf.grid_inv_w, kf.grid_inv_h]]).astype("<f8").tobytes())
    f.write(kf.desc.tobytes()); f.write(kf.uv.astype("<f8").tobytes()); f.write(kf.oct.tobytes()); f.write(kf.scale.astype("<f8").tobytes())
    f.write(kf.cell_begin.astype("<i4").tobytes()); f.write(kf.cell_feat.astype("<i4").tobytes())
    f.write(kf.has_pt.tobytes()); f.write(kf.matched.tobytes())
    for a in (kf.pos, kf.dist_min, kf.dist_max, kf.pred_max):
        f.write(a.astype("<f8").tobytes())
    f.write(kf.pt_desc.tobytes())


def _write(path, items, back=None):
    """items: (pair, dict of overrides: nulls, kf1 / kf2 -> dict of n_keys / n_levels / grid_cols / grid_rows); back: what came back
    for the call's queries (match, best_dist, level, state), the formula of synthetic_back by default"""
    if back is None:
        back = synthetic_back(sum(len(live(kf)) for p, _ in items for kf in (p.kf1, p.kf2)))
    with open(path, "wb") as f:
        f.write(np.array([len(items)], dtype="<i4").tobytes())
        for p, o in items:
            f.write(np.array([p.th_high, o.get("nulls", 0)], dtype="<i4").tobytes())
            f.write(np.concatenate([p.K, [p.s12], p.R12.ravel(), p.t12, [p.th]]).astype("<f8").tobytes())
            _write_kf(f, p.kf1, o.get("kf1", {}))
            _write_kf(f, p.kf2, o.get("kf2", {}))
        f.write(np.array([len(back[0])], dtype="<i4").tobytes())
        for a, dt in zip(back, ("<i4", "<u2", "i1", "u1")):
            f.write(np.asarray(a).astype(dt).tobytes())


def live(kf):
    """the keypoints that get a query record, in packed order"""
    return np.nonzero((kf.has_pt != 0) & (kf.matched == 0))[0]


def synthetic_back(n):
    """query m of the call came back with match = m mod 7 - 1, best_dist = m mod 257, level = m mod 200 - 128, state = m mod 6 + 3
    (0 where the match is not -1)"""
    m = np.arange(n)
    match = m % 7 - 1
    return match, m % 257, m % 200 - 128, np.where(match >= 0, 0, m % 6 + 3)


def keys(kf):
    k = np.zeros(kf.n_keys, dtype=KEY)
    k["d"], k["u"], k["v"], k["oct"] = kf.desc, kf.uv[:, 0], kf.uv[:, 1], kf.oct
    return k


def queries(kf):
    i = live(kf)
    q = np.zeros(len(i), dtype=QUERY)
    q["d"], q["pos"], q["idx"] = kf.pt_desc[i], kf.pos[i], i
    q["dist"] = np.stack([kf.dist_min[i], kf.dist_max[i], kf.pred_max[i]], axis=1).reshape(-1, 3)
    return q


def written_back(ps, back):
    """what unpack leaves in the callers' arrays, restated: per pair (match1, dist1, level1, state1, match12, match2, dist2, level2,
    state2, n_found)"""
    out, o = [], 0
    for p in ps:
        side = []
        for kf in (p.kf1, p.kf2):
            n, i = kf.n_keys, live(kf)
            match, dist, level = np.full(n, -1), np.full(n, 256), np.full(n, -128)
            state = np.where(kf.has_pt == 0, 1, 2)
            match[i], dist[i], level[i], state[i] = (np.asarray(a)[o:o + len(i)] for a in back)
            o += len(i)
            side.append((match, dist, level, state))
        m1, m2 = side[0][0], side[1][0]
        m12 = np.full(p.kf1.n_keys, -1)
        for i1 in range(p.kf1.n_keys):
            if 0 <= m1[i1] < p.kf2.n_keys and m2[m1[i1]] == i1:
                m12[i1] = m1[i1]
        out.append(side[0] + (m12,) + side[1] + (int((m12 >= 0).sum()),))
    return out


def weighted(ps, arrays, shift):
    """the harness's order-sensitive sum of one output over the pairs"""
    return sum((k + 1) * int(((np.arange(len(a)) + 1) * (np.asarray(a, dtype=np.int64) + shift)).sum()) for k, a in enumerate(arrays)) % 2 ** 64


def _batches():
    C = cases_mod.cases()
    many = [synth.sim3_search_scene(700 + k, n_keys1=(k * 5) % 23, n_keys2=(k * 7) % 19 * (k % 3 > 0), n_common=(k * 3) % 11, n_levels=(1 + k % 8, 1 + k % 5),
                                    grid=((1 + k % 5, 1 + k % 3), (1 + k % 4, 1 + k % 2)), extra_points=0.5) for k in range(300)]   # the threaded path
    return [[C["empty_kf1"]], [C["micro"]], [C["agree"]], [C["queries_257_3"], C["empty_kf2"], C["queries_513_0"], C["nothing_searchable"], C["queries_256_0"],
                                                           C["queries_3_257"], C["z_zero"]], list(C.values()), many]


def check_line(ps, line, back):
    f = hc.fields(line)
    n = len(ps)
    kfs = [kf for p in ps for kf in (p.kf1, p.kf2)]
    nq = [len(live(kf)) for kf in kfs]
    nk, ntq = sum(kf.n_keys for kf in kfs), sum(nq)
    nc, ft, lv = sum(len(kf.cell_begin) for kf in kfs), sum(len(kf.cell_feat) for kf in kfs), sum(kf.n_levels for kf in kfs)
    # a tile never spans two directions: every direction starts its own tiles, and one without queries gets none
    tiles = [(s // 2, s % 2, first, 0) for s in range(2 * n) for first in range(0, nq[s], 256)]
    assert (f["keys"], f["queries"], f["cells"], f["feat_tot"], f["lev_tot"], f["tiles"], f["n_tiles"]) == (nk, ntq, nc, ft, lv, len(tiles), len(tiles))
    # the arena, restated from the sizes: seven upload regions, four back regions, nothing device-only
    assert DIR.itemsize == 360 and KEY.itemsize == 64 and QUERY.itemsize == 96
    o, offs = 0, []
    for b in (360 * 2 * n, 16 * (len(tiles) + 1), 64 * (nk + 1), 96 * (ntq + 1), 4 * (nc + 1), 4 * (ft + 1), 8 * (lv + 1),
              4 * (ntq + 1), 2 * (ntq + 1), ntq + 1, ntq + 1):
        offs.append(o)
        o += up(b)
    names = ("dir", "tile", "key", "query", "cell", "feat", "lev", "match", "best_dist", "level", "state")
    assert [f[k] for k in names] == offs
    hc.assert_bound(f, [("cell_begin", "cell"), ("cell_feat", "feat")] + [(k, k) for k in names if k not in ("cell", "feat")])
    assert f["upload"] == offs[7] and f["back"] == o - offs[7] and f["total"] == o
    # the descriptors: direction d of a pair reads the queries of side d and every table of side 1 - d
    d = np.zeros(2 * n, dtype=DIR)
    off = np.zeros((2 * n, 5), dtype=np.int64)                  # per side: keys, queries, cells, feat, levels in front of it
    for s in range(1, 2 * n):
        kf = kfs[s - 1]
        off[s] = off[s - 1] + [kf.n_keys, nq[s - 1], len(kf.cell_begin), len(kf.cell_feat), kf.n_levels]
    for k, p in enumerate(ps):
        sR12, sR21, t21 = ref_mod.transforms(p, np.float64)
        for dr in range(2):
            src, tgt, s, t = kfs[2 * k + dr], kfs[2 * k + 1 - dr], 2 * k + dr, 2 * k + 1 - dr
            d[s]["off"] = [off[s][1], off[t][0], off[t][2], off[t][3], off[t][4]]
            d[s]["i"] = [nq[s], tgt.n_keys, tgt.n_levels, p.th_high, tgt.grid_cols, tgt.grid_rows, 0, 0]
            d[s]["c"] = np.concatenate([src.Rcw.ravel(), src.tcw, (sR12 if dr else sR21).ravel(), p.t12 if dr else t21, p.K, tgt.bounds,
                                        [tgt.grid_inv_w, tgt.grid_inv_h, tgt.log_scale_factor, p.th]])
    assert f["sum_dir"] == checksum(d)
    assert f["sum_tile"] == checksum(np.array(tiles, dtype="<i4").reshape(-1, 4))
    assert f["sum_key"] == checksum(*[keys(kf) for kf in kfs])
    # query compaction: only keypoints with has_pt && !matched get a record, in keypoint order, with their index
    assert f["sum_query"] == checksum(*[queries(kf) for kf in kfs])
    assert f["sum_cell"] == checksum(*[kf.cell_begin for kf in kfs])
    assert f["sum_feat"] == checksum(*[kf.cell_feat for kf in kfs])
    assert f["sum_lev"] == checksum(*[kf.scale for kf in kfs])
    # the write-back of what "came back"
    w = written_back(ps, back)
    assert f["got_status"] == 0 and f["got_found"] == sum((k + 1) * (r[9] + 1) for k, r in enumerate(w))
    for name, col, shift in (("match1", 0, 2), ("dist1", 1, 0), ("level1", 2, 129), ("state1", 3, 0), ("match12", 4, 2), ("match2", 5, 2), ("dist2", 6, 0),
                             ("level2", 7, 129), ("state2", 8, 0)):
        assert f["got_" + name] == weighted(ps, [r[col] for r in w], shift), name
    return f, w


def test_offsets_tiles_packing_and_write_back(checker, tmp_path):
    batches = _batches()
    files, backs = [], []
    for k, ps in enumerate(batches):
        files.append(str(tmp_path / ("b%d.ss" % k)))
        backs.append(synthetic_back(sum(len(live(kf)) for p in ps for kf in (p.kf1, p.kf2))))
        _write(files[-1], [(p, {}) for p in ps], backs[-1])
    for ps, line, back in zip(batches, hc.run(checker, files, len(files)), backs):
        f, w = check_line(ps, line, back)
    assert f["tiles"] > 100 and sum(r[9] for r in w) > 0          # the last batch: 300 pairs, packed on four threads


def test_agreement_in_the_write_back(checker, tmp_path):
    """the device result of the yardstick for the agreement cases, compacted as the kernel returns it: match12 and n_found literally"""
    p = cases_mod.cases()["agree"]
    r, e = cases_mod.ref("agree"), cases_mod.agree_expect()
    i1, i2 = live(p.kf1), live(p.kf2)
    back = [np.concatenate([r[k + "1"][i1], r[k + "2"][i2]]) for k in ("match", "best_dist", "level", "state")]
    path = str(tmp_path / "a.ss")
    ps = [cases_mod.cases()["micro"], p]
    n0 = len(live(ps[0].kf1)) + len(live(ps[0].kf2))
    assert n0 == 16                                                         # nine carriers a side, one of them already matched
    back = [np.concatenate([a, b]) for a, b in zip(synthetic_back(n0), back)]
    _write(path, [(q, {}) for q in ps], back)
    f, w = check_line(ps, hc.run(checker, [path], 1)[0], back)
    assert w[1][4].tolist() == e["match12"] == [0, -1, -1, -1, -1, -1, 4] and w[1][9] == e["n_found"] == 2
    assert w[1][0].tolist() == e["match1"] and w[1][5].tolist() == e["match2"] and w[1][3].tolist() == e["state1"] and w[1][8].tolist() == e["state2"]


def _with(kf, **kw):
    """a copy of the keyframe with single entries of its arrays replaced: name=(index, value)"""
    ch = {}
    for k, (i, v) in kw.items():
        a = getattr(kf, k).copy()
        a.reshape(-1)[i] = v
        ch[k] = a
    return kf.copy(**ch)


SIDE_REFUSALS = [
    (dict(over=dict(n_keys=-1)), "negative n_keys"),
    (dict(over=dict(n_levels=0)), "n_levels outside 1 .. 64"),
    (dict(over=dict(n_levels=65)), "n_levels outside 1 .. 64"),
    (dict(over=dict(grid_cols=0)), "grid size outside 1 .. 65536 cells"),
    (dict(over=dict(grid_rows=-3)), "grid size outside 1 .. 65536 cells"),
    (dict(over=dict(grid_cols=65536, grid_rows=2)), "grid size outside 1 .. 65536 cells"),
    (dict(over=dict(grid_cols=2147483647, grid_rows=2147483647)), "grid size outside 1 .. 65536 cells"),
    (dict(edit=dict(oct=(6, 8))), "keypoint 6: octave >= n_levels"),
    (dict(edit=dict(uv=(11, np.nan))), "keypoint 5: a pixel is not finite"),
    (dict(edit=dict(Rcw=(4, np.nan))), "the pose is not finite"),
    (dict(edit=dict(tcw=(1, np.inf))), "the pose is not finite"),
    (dict(edit=dict(bounds=(3, np.inf))), "a bound or cell size is not finite"),
    (dict(copy=dict(grid_inv_h=np.nan)), "a bound or cell size is not finite"),
    (dict(edit=dict(scale=(7, np.nan))), "a level table is not finite"),
    (dict(copy=dict(log_scale_factor=np.nan)), "a level table is not finite"),
    (dict(point=dict(pos=np.nan)), "keypoint P: the position is not finite"),
    (dict(point=dict(dist_min=np.nan)), "keypoint P: a distance is not finite"),
    (dict(point=dict(dist_max=np.inf)), "keypoint P: a distance is not finite"),
    (dict(point=dict(pred_max=np.nan)), "keypoint P: a distance is not finite"),
    (dict(edit=dict(cell_begin=(0, 1))), "cell_begin does not start at 0"),
    (dict(edit=dict(cell_begin=(5, -1))), "cell_begin decreases at cell 4"),
    (dict(edit=dict(cell_begin=(3072, 41))), "cell_begin ends above n_keys"),
    (dict(edit=dict(cell_feat=(4, 40))), "cell_feat entry 4: keypoint index out of range"),
    (dict(edit=dict(cell_feat=(0, -1))), "cell_feat entry 0: keypoint index out of range"),
    (dict(dup=1), "cell_feat entry 9: keypoint K listed twice"),
]
PAIR_REFUSALS = [
    (dict(nulls=4), "NULL problem or result"),
    (dict(nulls=16), "NULL problem or result"),
    (dict(nulls=1), "keyframe 1: NULL array with n_keys > 0"),
    (dict(nulls=2), "keyframe 1: NULL array with n_keys > 0"),
    (dict(nulls=512), "keyframe 1: NULL array with n_keys > 0"),
    (dict(nulls=2048), "keyframe 1: NULL array with n_keys > 0"),
    (dict(nulls=4096), "keyframe 1: NULL array with n_keys > 0"),
    (dict(nulls=16384), "keyframe 1: NULL array with n_keys > 0"),
    (dict(nulls=32), "keyframe 2: NULL array with n_keys > 0"),
    (dict(nulls=256), "keyframe 2: NULL array with n_keys > 0"),
    (dict(nulls=1024), "keyframe 2: NULL array with n_keys > 0"),
    (dict(nulls=8192), "keyframe 2: NULL array with n_keys > 0"),
    (dict(nulls=8), "keyframe 2: NULL level table"),
    (dict(nulls=64), "keyframe 1: NULL cell_begin"),
    (dict(nulls=128), "keyframe 2: NULL cell_feat"),
    (dict(copy=dict(s12=0.0)), "s12 is not finite or not positive"),
    (dict(copy=dict(s12=-1.5)), "s12 is not finite or not positive"),
    (dict(copy=dict(s12=np.nan)), "s12 is not finite or not positive"),
    (dict(copy=dict(s12=np.inf)), "s12 is not finite or not positive"),
    (dict(R12=np.nan), "the Sim3 is not finite"),
    (dict(t12=np.inf), "the Sim3 is not finite"),
    (dict(K=np.nan), "an intrinsic is not finite"),
    (dict(copy=dict(th=np.inf)), "a threshold is not finite"),
    (dict(copy=dict(th_high=257)), "th_high outside 0 .. 256"),
    (dict(copy=dict(th_high=-1)), "th_high outside 0 .. 256"),
]
REFUSALS = ([(side, ch, "keyframe %d: %s" % (side, m)) for side in (1, 2) for ch, m in SIDE_REFUSALS] + [(0, ch, m) for ch, m in PAIR_REFUSALS])


def _scene(seed):
    return synth.sim3_search_scene(seed, n_keys1=40, n_keys2=40, n_common=20)


@pytest.mark.parametrize("side,change,message", REFUSALS, ids=["%d_%s_%d" % (s, m.split(": ")[-1].replace(" ", "_").replace("/", ""), k)
                                                               for k, (s, _, m) in enumerate(REFUSALS)])
def test_refusals(checker, tmp_path, side, change, message):
    good, bad = _scene(40), _scene(41)
    o = {}
    if side:
        name = "kf%d" % side
        kf = getattr(bad, name)
        assert len(kf.cell_feat) > 10
        if "over" in change:
            o[name] = change["over"]
        if "edit" in change:
            kf = _with(kf, **change["edit"])
        if "copy" in change:
            kf = kf.copy(**change["copy"])
        if "point" in change:                                   # a keypoint with a usable point; one without may hold anything
            i, j = int(np.nonzero(kf.has_pt)[0][3]), int(np.nonzero(kf.has_pt == 0)[0][0])
            (k, v), = change["point"].items()
            kf = _with(_with(kf, **{k: (j * (3 if k == "pos" else 1), v)}), **{k: (i * (3 if k == "pos" else 1) + (k == "pos"), v)})
            assert j < i
            message = message.replace("P", str(i))
        if "dup" in change:
            a = kf.cell_feat.copy()
            a[9] = a[2]
            message = message.replace("K", str(a[2]))
            kf = kf.copy(cell_feat=a)
        bad = bad.copy(**{name: kf})
    else:
        o = {k: v for k, v in change.items() if k == "nulls"}
        if "copy" in change:
            bad = bad.copy(**change["copy"])
        for k in ("R12", "t12", "K"):
            if k in change:
                a = getattr(bad, k).copy()
                a.reshape(-1)[2] = change[k]
                bad = bad.copy(**{k: a})
    path = str(tmp_path / "r.ss")
    _write(path, [(good, {}), (bad, o)])
    assert hc.run(checker, [path], 1) == ["error pair 1: " + message]


def test_legal_edges(checker, tmp_path):
    """a keyframe without keypoints needs no keypoint or result arrays of its side and no cell_feat; 64 levels and octave 63 are legal;
    th_high 0 and 256 are legal; a 65536 x 1 grid is legal; a negative th is legal"""
    C = cases_mod.cases()
    e1 = C["empty_kf1"].copy(th_high=256, th=-1.0)
    e2 = C["empty_kf2"].copy(th_high=0)
    s = 1.01 ** np.arange(64)
    b = _scene(8)
    b = b.copy(kf2=_with(b.kf2.copy(scale=s), oct=(5, 63)))
    g = synth.sim3_search_scene(9, n_keys1=20, n_keys2=300, n_common=10, grid=((65536, 1), (64, 48)), extra_points=0.95)
    path = str(tmp_path / "e.ss")
    items = [(e1, dict(nulls=1 | 2 | 512 | 2048 | 4096 | 16384)), (e2, dict(nulls=32 | 128 | 256 | 1024 | 8192)), (b, {}), (g, {})]
    _write(path, items)
    back = synthetic_back(sum(len(live(kf)) for p, _ in items for kf in (p.kf1, p.kf2)))
    f, _ = check_line([p for p, _ in items], hc.run(checker, [path], 1)[0], back)
    assert f["lev_tot"] == 16 + 16 + 8 + 64 + 16 and f["cells"] == 2 * 3073 * 3 + 65537 + 3073 and f["tiles"] >= 5
