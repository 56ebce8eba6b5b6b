"""The host half of vba_search_by_projection (mc_slam_amd/csrc/vba_host_search_proj.h, vba_host_arena.h: refusals, arena offsets, the
keypoint and query records, the grid copy, and the write-back that replays the apply loop: overwrite, drop and counts) under
AddressSanitizer + UBSan (CPU only, a stand-alone program, nothing preloaded).  The harness (tests/host_search_proj_check.cpp) packs
into heap blocks of exactly the arena's sizes; every expected offset below is restated from the sizes alone, the packed regions are
compared with records built in NumPy through an order-sensitive checksum, and the replay of a synthetic device result is restated
here in Python."""
import numpy as np
import pytest

from mc_slam_amd import abi, synth
import search_proj_cases as cases_mod
import search_proj_ref as ref_mod
import host_check_lib as hc
from host_check_lib import checksum, up

DESC = np.dtype([("off", "<i8", 5), ("i", "<i4", 8), ("nn_ratio", "<f4"), ("pad1", "<i4"), ("c", "<f8", 28)])
KEY = np.dtype([("d", "u1", 32), ("u", "<f8"), ("v", "<f8"), ("oct", "u1"), ("pad", "u1", 15)])
QUERY = np.dtype([("d", "u1", 32), ("pos", "<f8", 3), ("normal", "<f8", 3), ("dist", "<f8", 3), ("skip", "u1"), ("blocks", "u1"), ("oct", "u1"), ("pad", "u1", 5)])
LAST, LOCAL = abi.SEARCH_PROJ_LAST_FRAME, abi.SEARCH_PROJ_LOCAL_MAP


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return hc.build(tmp_path_factory, "host_search_proj_check", pthread=True)


def consts(p, packed=False):
    """the 28 doubles of a descriptor (packed: what the mode does not read is zero) or, with nn_ratio behind them, of a file"""
    loc = p.local or not packed
    c = np.concatenate([p.Rcw.ravel(), p.tcw, p.Ow if loc else np.zeros(3), p.K, p.bounds,
                        [p.grid_inv_w, p.grid_inv_h, p.log_scale_factor if loc else 0.0, p.th, p.cos_view if loc else 0.0]])
    return c if packed else np.concatenate([c, [p.nn_ratio]])


def _or(a, n, dtype, cols=None):
    return np.zeros((n,) if cols is None else (n, cols), dtype=dtype) if a is None else a.astype(dtype)


def _write(path, items):
    """items: (problem, dict of n_keys / n_q / n_levels / grid_cols / grid_rows / nulls overrides)"""
    with open(path, "wb") as f:
        f.write(np.array([len(items)], dtype="<i4").tobytes())
        for p, o in items:
            nk, nq = p.n_keys, p.n_q
            f.write(np.array([o.get("mode", p.mode), int(p.check_orientation), o.get("n_keys", nk), nk, o.get("n_q", nq), nq, o.get("n_levels", p.n_levels),
                              p.n_levels, o.get("grid_cols", p.grid_cols), o.get("grid_rows", p.grid_rows), len(p.cell_begin), len(p.cell_feat), p.th_high,
                              o.get("nulls", 0)], dtype="<i4").tobytes())
            f.write(consts(p).astype("<f8").tobytes())
            f.write(p.desc.tobytes()); f.write(p.uv.astype("<f8").tobytes()); f.write(p.oct.tobytes())
            f.write(_or(p.angle, nk, "<f4").tobytes()); f.write(p.occupied.tobytes()); f.write(p.scale.astype("<f8").tobytes())
            f.write(p.cell_begin.astype("<i4").tobytes()); f.write(p.cell_feat.astype("<i4").tobytes())
            f.write(p.q_pos.astype("<f8").tobytes()); f.write(p.q_desc.tobytes()); f.write(p.q_skip.tobytes()); f.write(p.q_blocks.tobytes())
            f.write(_or(p.q_oct, nq, "u1").tobytes()); f.write(_or(p.q_angle, nq, "<f4").tobytes()); f.write(_or(p.q_normal, nq, "<f8", 3).tobytes())
            for a in (p.q_dist_min, p.q_dist_max, p.q_pred_max):
                f.write(_or(a, nq, "<f8").tobytes())


def keys(p):
    k = np.zeros(p.n_keys, dtype=KEY)
    k["d"], k["u"], k["v"], k["oct"] = p.desc, p.uv[:, 0], p.uv[:, 1], p.oct
    return k


def queries(p):
    q = np.zeros(p.n_q, dtype=QUERY)
    q["d"], q["pos"], q["skip"], q["blocks"] = p.q_desc, p.q_pos, p.q_skip != 0, p.q_blocks != 0
    if p.local:
        q["normal"] = p.q_normal
        q["dist"] = np.stack([p.q_dist_min, p.q_dist_max, p.q_pred_max], axis=1).reshape(-1, 3)
    else:
        q["oct"] = p.q_oct
    return q


def _batches():
    C = cases_mod.cases()
    many = [synth.search_proj_scene(700 + k, k % 2, n_keys=(k * 5) % 23, n_q=(k * 7) % 5 * (k % 3), n_levels=1 + k % 8, cols=1 + k % 5, rows=1 + k % 3,
                                    check_orientation=bool(k % 4 < 2)) for k in range(300)]   # the threaded path, a third without queries
    small = [n for n in C if n != "max_keys"]
    return [[C["empty_q_last"]], [C["micro_last"]], [C["micro_local"]],
            [C["queries_257"], C["empty_keys_local"], C["queries_513"], C["empty_q_local"], C["queries_256"], C["z_zero_last"], C["drop_clears_kept"]],
            [C[n] for n in small], many]


def replay(ps):
    """the write-back of the harness's synthetic device result, restated: the sums the harness prints"""
    s = dict.fromkeys(("match", "before", "rounds", "bi", "bd", "bd2", "lv", "st", "bin", "km", "hist", "ind", "uv", "vc"), 0)
    i0 = 0
    for k, p in enumerate(ps):
        nk, nq = p.n_keys, p.n_q
        i = np.arange(i0, i0 + nq)
        i0 += nq
        bi = (5 * i) % nk if nk else np.full(nq, -1)
        st = np.where((i % 3 == 0) & (nk > 0), 0, 1 + i % 9)
        ori = (not p.local) and p.check_orientation
        km = np.full(nk, -1)
        bins = np.full(nq, 255)
        hist = np.zeros(30, dtype=int)
        n = 0
        for q in range(nq):
            if st[q] == 0:
                km[bi[q]] = q
                n += 1
                if ori:
                    bins[q] = ref_mod.rot_bin(p.q_angle[q], p.angle[bi[q]])
                    hist[bins[q]] += 1
        before, ind = n, (-1, -1, -1)
        if ori:
            ind = ref_mod.three_maxima(hist)
            for q in range(nq):
                if bins[q] != 255 and bins[q] not in ind:
                    km[bi[q]], st[q] = -2, 6
                    n -= 1
        j = np.arange(nq)
        s["match"] += n * (k + 1); s["before"] += before * (k + 1); s["rounds"] += (k + 1) * (k + 1)
        s["hist"] += int((hist * (np.arange(30) + 1)).sum()) * (k + 1); s["ind"] += sum(v * (b + 1) for b, v in enumerate(ind)) * (k + 1)
        s["bi"] += int(bi.sum()); s["bd"] += int((i % 257).sum()); s["bd2"] += int(((3 * i) % 257).sum()); s["lv"] += int((i % 200 - 128).sum())
        s["st"] += int((st * (j % 5 + 1)).sum()); s["bin"] += int((bins * (j % 7 + 1)).sum()); s["km"] += int((km * (np.arange(nk) % 11 + 1)).sum())
        s["uv"] += -int(i.sum()); s["vc"] += int(i.sum())
    return s


def test_offsets_packing_and_write_back(checker, tmp_path):
    batches = _batches()
    files = []
    for k, ps in enumerate(batches):
        files.append(str(tmp_path / ("b%d.sp" % k)))
        _write(files[-1], [(p, {}) for p in ps])
    dropped = 0
    for ps, line in zip(batches, hc.run(checker, files, len(files))):
        f = hc.fields(line)
        n = len(ps)
        nk, nq = sum(p.n_keys for p in ps), sum(p.n_q for p in ps)
        nc, ft, lv = sum(len(p.cell_begin) for p in ps), sum(len(p.cell_feat) for p in ps), sum(p.n_levels for p in ps)
        mk = max(p.n_keys for p in ps)
        assert (f["keys"], f["qs"], f["cells"], f["feat_tot"], f["lev_tot"], f["max_keys"], f["lds"], f["grid"]) == (nk, nq, nc, ft, lv, mk, 4 * (mk + 1), n)
        # the arena, restated from the sizes: seven upload regions, eight back regions, two that stay on the device
        assert DESC.itemsize == 304 and KEY.itemsize == 64 and QUERY.itemsize == 112
        o, offs = 0, []
        for b in (304 * n, 64 * (nk + 1), nk + 1, 112 * (nq + 1), 4 * (nc + 1), 4 * (ft + 1), 8 * (lv + 1),
                  4 * (n + 1), 4 * (nq + 1), 2 * (nq + 1), 2 * (nq + 1), nq + 1, 8 * (nq + 1), 16 * (nq + 1), nq + 1, 8 * (nq + 1), 4 * (nq + 1)):
            offs.append(o)
            o += up(b)
        names = ("desc", "key", "occupied", "query", "cell", "feat", "lev", "rounds", "best_idx", "best_dist", "best_dist2", "level", "view_cos", "uv", "state",
                 "rad", "prev")
        assert [f[k] for k in names] == offs
        # SpBatch reads every region where it is: the pairs of equal element size are the ones a swap would not show on the CPU otherwise
        hc.assert_bound(f, [("cell_begin", "cell"), ("cell_feat", "feat")] + [(k, k) for k in names if k not in ("cell", "feat")])
        assert f["upload"] == offs[7] and f["back"] == offs[15] - offs[7] and f["total"] == o
        d = np.zeros(n, dtype=DESC)
        ok = oq = oc = of = ol = 0
        for k, p in enumerate(ps):
            d[k]["off"] = [ok, oq, oc, of, ol]
            d[k]["i"] = [p.n_keys, p.n_q, p.n_levels, p.th_high, p.grid_cols, p.grid_rows, int(p.local), 0]
            d[k]["nn_ratio"] = p.nn_ratio if p.local else 0.0
            d[k]["c"] = consts(p, packed=True)
            ok += p.n_keys; oq += p.n_q; oc += len(p.cell_begin); of += len(p.cell_feat); ol += p.n_levels
        assert f["sum_desc"] == checksum(d)
        assert f["sum_key"] == checksum(*[keys(p) for p in ps])
        assert f["sum_occ"] == checksum(*[(p.occupied != 0).astype("u1") for p in ps])
        assert f["sum_query"] == checksum(*[queries(p) for p in ps])
        assert f["sum_cell"] == checksum(*[p.cell_begin for p in ps])
        assert f["sum_feat"] == checksum(*[p.cell_feat for p in ps])
        assert f["sum_lev"] == checksum(*[p.scale for p in ps])
        # the write-back: the apply loop replayed on the synthetic result of the harness
        s = replay(ps)
        assert (f["got_match"], f["got_before"], f["got_status"], f["got_rounds"]) == (s["match"], s["before"], 0, s["rounds"])
        assert (f["got_bi"], f["got_bd"], f["got_bd2"], f["got_lv"], f["got_uv8"], f["got_vc16"]) == (s["bi"], s["bd"], s["bd2"], s["lv"], s["uv"], s["vc"])
        assert (f["got_st"], f["got_bin"], f["got_km"], f["got_hist"], f["got_ind"]) == (s["st"], s["bin"], s["km"], s["hist"], s["ind"])
        dropped += s["before"] - s["match"]
    assert dropped > 50            # the drop of the orientation filter ran


def test_write_back_overwrite_and_drop_by_hand(checker, tmp_path):
    """5 queries over 3 keypoints in last-frame mode: the synthetic result matches the queries 0 and 3, both on keypoint 0 (5 i mod 3), so
    query 3 overwrites query 0.  Their angles put them into the bins 3 and 0; with two bins filled both are kept and the counts are 2
    and 2"""
    p = synth.search_proj_scene(5, LAST, n_keys=3, n_q=5)
    p = p.copy(angle=np.array([10, 10, 10], dtype=np.float32), q_angle=np.array([100, 0, 0, 10, 0], dtype=np.float32))
    path = str(tmp_path / "h.sp")
    _write(path, [(p, {})])
    f = hc.fields(hc.run(checker, [path], 1)[0])
    # key_match = [3, -1, -1]: weights 1, 2, 3; hist: bin 3 (query 0) and bin 0 (query 3), both kept
    assert (f["got_match"], f["got_before"], f["got_km"], f["got_hist"], f["got_ind"]) == (2, 2, 3 - 2 - 3, 4 + 1, 0 * 1 + 3 * 2 - 1 * 3)


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
    (LAST, dict(n_keys=-1), "negative n_keys"),
    (LAST, dict(n_q=-2), "negative n_q"),
    (LAST, dict(mode=2), "unknown mode"),
    (LOCAL, dict(mode=-1), "unknown mode"),
    (LAST, dict(nulls=4), "NULL problem or result"),
    (LOCAL, dict(nulls=16), "NULL problem or result"),
    (LAST, dict(nulls=1), "NULL array with n_keys > 0"),
    (LOCAL, dict(nulls=1024), "NULL array with n_keys > 0"),
    (LOCAL, dict(nulls=2048), "NULL array with n_keys > 0"),
    (LAST, dict(nulls=8192), "NULL array with n_keys > 0"),
    (LAST, dict(nulls=256), "NULL array with n_q > 0"),
    (LOCAL, dict(nulls=512), "NULL array with n_q > 0"),
    (LAST, dict(nulls=2), "NULL array with n_q > 0"),
    (LOCAL, dict(nulls=32), "NULL array with n_q > 0"),
    (LAST, dict(nulls=32768), "NULL array with n_q > 0"),
    (LAST, dict(nulls=4096), "NULL last-frame array with n_q > 0"),
    (LAST, dict(nulls=16384), "NULL last-frame array with n_q > 0"),
    (LOCAL, dict(nulls=4096), "NULL local-map array with n_q > 0"),
    (LAST, dict(nulls=8), "NULL level table"),
    (LOCAL, dict(nulls=64), "NULL cell_begin"),
    (LAST, dict(nulls=128), "NULL cell_feat"),
    (LAST, dict(n_levels=0), "n_levels outside 1 .. 64"),
    (LOCAL, dict(n_levels=65), "n_levels outside 1 .. 64"),
    (LAST, dict(copy=dict(th_high=257)), "th_high outside 0 .. 256"),
    (LOCAL, dict(copy=dict(th_high=-1)), "th_high outside 0 .. 256"),
    (LAST, dict(grid_cols=0), "grid size outside 1 .. 65536 cells"),
    (LOCAL, dict(grid_cols=65536, grid_rows=2), "grid size outside 1 .. 65536 cells"),
    (LAST, dict(grid_cols=2147483647, grid_rows=2147483647), "grid size outside 1 .. 65536 cells"),
    (LAST, dict(edit=dict(oct=(6, 8))), "keypoint 6: octave >= n_levels"),
    (LOCAL, dict(edit=dict(uv=(11, np.nan))), "keypoint 5: a pixel is not finite"),
    (LAST, dict(edit=dict(angle=(3, 360.0))), "keypoint 3: angle outside [0, 360)"),
    (LAST, dict(edit=dict(angle=(2, np.nan))), "keypoint 2: angle outside [0, 360)"),
    (LAST, dict(edit=dict(q_angle=(4, -1.0))), "query 4: angle outside [0, 360)"),
    (LAST, dict(edit=dict(q_oct=(9, 8))), "query 9: octave >= n_levels"),
    (LAST, dict(edit=dict(Rcw=(4, np.nan))), "the pose is not finite"),
    (LOCAL, dict(edit=dict(tcw=(1, np.inf))), "the pose is not finite"),
    (LOCAL, dict(edit=dict(Ow=(2, -np.inf))), "the pose is not finite"),
    (LAST, dict(edit=dict(K=(0, np.nan))), "an intrinsic is not finite"),
    (LOCAL, dict(edit=dict(bounds=(3, np.inf))), "a bound or cell size is not finite"),
    (LAST, dict(copy=dict(grid_inv_h=np.nan)), "a bound or cell size is not finite"),
    (LAST, dict(copy=dict(th=np.inf)), "a threshold is not finite"),
    (LOCAL, dict(copy=dict(cos_view=np.nan)), "a threshold is not finite"),
    (LOCAL, dict(copy=dict(nn_ratio=np.nan)), "a threshold is not finite"),
    (LAST, dict(edit=dict(scale=(7, np.nan))), "a level table is not finite"),
    (LOCAL, dict(copy=dict(log_scale_factor=np.nan)), "a level table is not finite"),
    (LAST, dict(edit=dict(q_pos=(10, np.nan))), "query 3: the position is not finite"),
    (LOCAL, dict(edit=dict(q_normal=(2, np.inf))), "query 0: the normal is not finite"),
    (LOCAL, dict(edit=dict(q_dist_min=(4, np.nan))), "query 4: a distance is not finite"),
    (LOCAL, dict(edit=dict(q_dist_max=(5, np.inf))), "query 5: a distance is not finite"),
    (LOCAL, dict(edit=dict(q_pred_max=(6, np.nan))), "query 6: a distance is not finite"),
    (LAST, dict(edit=dict(cell_begin=(0, 1))), "cell_begin does not start at 0"),
    (LOCAL, dict(edit=dict(cell_begin=(5, -1))), "cell_begin decreases at cell 4"),
    (LAST, dict(edit=dict(cell_begin=(3072, 41))), "cell_begin ends above n_keys"),
    (LOCAL, dict(edit=dict(cell_feat=(4, 40))), "cell_feat entry 4: keypoint index out of range"),
    (LAST, dict(edit=dict(cell_feat=(0, -1))), "cell_feat entry 0: keypoint index out of range"),
    (LOCAL, dict(dup=1), "cell_feat entry 9: keypoint K listed twice"),
    (LOCAL, dict(big=1), "n_keys above 16384: the claim table of a frame lives in LDS"),
]


@pytest.mark.parametrize("mode,change,message", REFUSALS, ids=[m.replace(" ", "_").replace("/", "").replace(":", "") + str(k) for k, (_, _, m) in enumerate(REFUSALS)])
def test_refusals(checker, tmp_path, mode, change, message):
    good, bad = synth.search_proj_scene(40, mode, n_keys=40, n_q=20), synth.search_proj_scene(41, mode, n_keys=40, n_q=20)
    assert len(bad.cell_feat) > 10
    o = {k: v for k, v in change.items() if k in ("mode", "n_keys", "n_q", "n_levels", "grid_cols", "grid_rows", "nulls")}
    if "edit" in change:
        bad = _with(bad, **change["edit"])
    if "copy" in change:
        bad = bad.copy(**change["copy"])
    if "dup" in change:
        a = bad.cell_feat.copy()
        a[9] = a[2]
        message = message.replace("K", str(a[2]))
        bad = bad.copy(cell_feat=a)
    if "big" in change:
        bad = synth.search_proj_scene(42, mode, n_keys=abi.SEARCH_PROJ_MAX_KEYS + 1, n_q=3, twins=0.0)
    path = str(tmp_path / "r.sp")
    _write(path, [(good, {}), (bad, o)])
    assert hc.run(checker, [path], 1) == ["error problem 1: " + message]


def test_legal_edges(checker, tmp_path):
    """a problem without queries needs no query or per-query result arrays, one without keypoints no keypoint arrays, no key_match and
    no cell_feat; the arrays of the other mode are NULL throughout (the harness passes them so); without check_orientation no angles
    are needed and none is checked; 64 levels and octave 63 are legal; th_high 0 and 256 are legal; a 65536 x 1 grid is legal; a
    negative th is legal; a frame of exactly 16384 keypoints is legal"""
    C = cases_mod.cases()
    e = C["empty_q_last"]
    k = C["empty_keys_local"].copy(th_high=256, th=-1.0)
    s = 1.01 ** np.arange(64)
    b = synth.search_proj_scene(8, LAST, n_keys=30, n_q=10, check_orientation=False).copy(scale=s, th_high=0)
    b = _with(b, oct=(5, 63), q_oct=(2, 63), angle=(1, 400.0))
    g = synth.search_proj_scene(9, LOCAL, n_keys=20, n_q=300, cols=65536, rows=1)
    m = C["max_keys"]
    path = str(tmp_path / "e.sp")
    _write(path, [(e, dict(nulls=2 | 32 | 256 | 512 | 4096 | 16384 | 32768)), (k, dict(nulls=1 | 128 | 1024 | 2048)), (b, dict(nulls=8192 | 16384)), (g, {}), (m, {})])
    f = hc.fields(hc.run(checker, [path], 1)[0])
    assert (f["keys"], f["qs"], f["lev_tot"], f["grid"], f["max_keys"], f["lds"]) == (e.n_keys + 30 + 20 + 16384, k.n_q + 10 + 300 + m.n_q, 8 + 8 + 64 + 8 + 8, 5, 16384, 65540)
    assert f["cells"] == 2 * 3073 + 3073 + 65537 + 128 * 96 + 1
