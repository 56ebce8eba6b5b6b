"""The host half of vba_search_by_projection_kf (mc_slam_amd/csrc/vba_host_search_proj_kf.h, vba_host_arena.h: refusals, arena offsets,
the keypoint and query records, the grid copy, and the write-back that replays the apply loop: key_match, histogram, maxima, drop
and counts) under AddressSanitizer + UBSan (CPU only, a stand-alone program, nothing preloaded).  The harness
(tests/host_search_proj_kf_check.cpp) packs into heap blocks of exactly the arena's sizes; every expected offset below is restated
from the sizes alone, the packed regions are compared with records built in NumPy through an order-sensitive checksum, and the replay
of a synthetic device result is restated here in Python."""
import numpy as np
import pytest

from mc_slam_amd import abi, synth
import search_proj_kf_cases as cases_mod
import search_proj_kf_ref as ref_mod
import host_check_lib as hc
from host_check_lib import checksum, up

DESC = np.dtype([("off", "<i8", 5), ("i", "<i4", 8), ("nn_ratio", "<f4"), ("pad1", "<i4"), ("c", "<f8", 28)])
KEY = np.dtype([("d", "u1", 32), ("u", "<f8"), ("v", "<f8"), ("oct", "u1"), ("pad", "u1", 15)])
QUERY = np.dtype([("d", "u1", 32), ("pos", "<f8", 3), ("normal", "<f8", 3), ("dist", "<f8", 3), ("skip", "u1"), ("blocks", "u1"), ("oct", "u1"), ("pad", "u1", 5)])
LOOP, RELOC = abi.SEARCH_PROJ_KF_LOOP, abi.SEARCH_PROJ_KF_RELOC


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return hc.build(tmp_path_factory, "host_search_proj_kf_check", pthread=True)


def consts(p, packed=False):
    """the 28 doubles of a file or of a descriptor (packed: cos_view is zero in reloc mode)"""
    return np.concatenate([p.Rcw.ravel(), p.tcw, p.Ow, p.K, p.bounds,
                           [p.grid_inv_w, p.grid_inv_h, p.log_scale_factor, p.th, 0.0 if (packed and p.reloc) else p.cos_view]])


def _or(a, n, dtype, cols=None):
    return np.zeros((n,) if cols is None else (n, cols), dtype=dtype) if a is None else a.astype(dtype)


def _write(path, items):
    """items: (problem, dict of mode / n_keys / n_q / n_levels / grid_cols / grid_rows / nulls overrides)"""
    with open(path, "wb") as f:
        f.write(np.array([len(items)], dtype="<i4").tobytes())
        for p, o in items:
            nk, nq = p.n_keys, p.n_q
            f.write(np.array([o.get("mode", p.mode), int(p.check_orientation), o.get("n_keys", nk), nk, o.get("n_q", nq), nq, o.get("n_levels", p.n_levels),
                              p.n_levels, o.get("grid_cols", p.grid_cols), o.get("grid_rows", p.grid_rows), len(p.cell_begin), len(p.cell_feat), p.th_dist,
                              o.get("nulls", 0)], dtype="<i4").tobytes())
            f.write(consts(p).astype("<f8").tobytes())
            f.write(p.desc.tobytes()); f.write(p.uv.astype("<f8").tobytes()); f.write(p.oct.tobytes())
            f.write(_or(p.angle, nk, "<f4").tobytes()); f.write(p.occupied.tobytes()); f.write(p.scale.astype("<f8").tobytes())
            f.write(p.cell_begin.astype("<i4").tobytes()); f.write(p.cell_feat.astype("<i4").tobytes())
            f.write(p.q_pos.astype("<f8").tobytes()); f.write(p.q_desc.tobytes()); f.write(p.q_skip.tobytes())
            f.write(_or(p.q_angle, nq, "<f4").tobytes()); f.write(_or(p.q_normal, nq, "<f8", 3).tobytes())
            for a in (p.q_dist_min, p.q_dist_max, p.q_pred_max):
                f.write(a.astype("<f8").tobytes())


def keys(p):
    k = np.zeros(p.n_keys, dtype=KEY)
    k["d"], k["u"], k["v"], k["oct"] = p.desc, p.uv[:, 0], p.uv[:, 1], p.oct
    return k


def queries(p):
    q = np.zeros(p.n_q, dtype=QUERY)
    q["d"], q["pos"], q["skip"], q["blocks"] = p.q_desc, p.q_pos, p.q_skip != 0, 1
    if not p.reloc:
        q["normal"] = p.q_normal
    q["dist"] = np.stack([p.q_dist_min, p.q_dist_max, p.q_pred_max], axis=1).reshape(-1, 3)
    return q


def _batches():
    C = cases_mod.cases()
    many = [synth.search_proj_kf_scene(700 + k, k % 2, n_keys=(k * 5) % 23, n_q=(k * 7) % 5 * (k % 3), n_levels=1 + k % 8, cols=1 + k % 5, rows=1 + k % 3,
                                       check_orientation=bool(k % 4 < 2)) for k in range(300)]   # the threaded path, a third without queries
    small = [n for n in C if n != "max_keys"]
    return [[C["empty_q_loop"]], [C["micro_loop"]], [C["micro_reloc"]],
            [C["queries_257"], C["empty_keys_reloc"], C["queries_513"], C["empty_q_reloc"], C["queries_256"], C["z_zero_loop"], C["synth_mid_reloc"]],
            [C[n] for n in small], many]


def replay(ps):
    """the write-back of the harness's synthetic device result, restated: the sums the harness prints"""
    s = dict.fromkeys(("match", "before", "rounds", "bi", "bd", "lv", "st", "bin", "km", "hist", "ind", "uv"), 0)
    i0 = 0
    for k, p in enumerate(ps):
        nk, nq = p.n_keys, p.n_q
        i = np.arange(i0, i0 + nq)
        i0 += nq
        bi = (5 * i) % nk if nk else np.full(nq, -1)
        st = np.where((i % 3 == 0) & (nk > 0), 0, 1 + i % 8)
        ori = p.reloc and p.check_orientation
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
                    km[bi[q]], st[q] = -2, 7
                    n -= 1
        j = np.arange(nq)
        s["match"] += n * (k + 1); s["before"] += before * (k + 1); s["rounds"] += (k + 1) * (k + 1)
        s["hist"] += int((hist * (np.arange(30) + 1)).sum()) * (k + 1); s["ind"] += sum(v * (b + 1) for b, v in enumerate(ind)) * (k + 1)
        s["bi"] += int(bi.sum()); s["bd"] += int((i % 257).sum()); s["lv"] += int((i % 200 - 128).sum())
        s["st"] += int((st * (j % 5 + 1)).sum()); s["bin"] += int((bins * (j % 7 + 1)).sum()); s["km"] += int((km * (np.arange(nk) % 11 + 1)).sum())
        s["uv"] += -int(i.sum())
    return s


def test_offsets_packing_and_write_back(checker, tmp_path):
    batches = _batches()
    files = []
    for k, ps in enumerate(batches):
        files.append(str(tmp_path / ("b%d.sk" % k)))
        _write(files[-1], [(p, {}) for p in ps])
    dropped = 0
    for ps, line in zip(batches, hc.run(checker, files, len(files))):
        f = hc.fields(line)
        n = len(ps)
        nk, nq = sum(p.n_keys for p in ps), sum(p.n_q for p in ps)
        nc, ft, lv = sum(len(p.cell_begin) for p in ps), sum(len(p.cell_feat) for p in ps), sum(p.n_levels for p in ps)
        mk = max(p.n_keys for p in ps)
        assert (f["keys"], f["qs"], f["cells"], f["feat_tot"], f["lev_tot"], f["max_keys"], f["lds"], f["grid"]) == (nk, nq, nc, ft, lv, mk, 4 * (mk + 1), n)
        # the arena, restated from the sizes: seven upload regions, six back regions, two that stay on the device
        assert DESC.itemsize == 304 and KEY.itemsize == 64 and QUERY.itemsize == 112
        o, offs = 0, []
        for b in (304 * n, 64 * (nk + 1), nk + 1, 112 * (nq + 1), 4 * (nc + 1), 4 * (ft + 1), 8 * (lv + 1),
                  4 * (n + 1), 4 * (nq + 1), 2 * (nq + 1), nq + 1, 16 * (nq + 1), nq + 1, 8 * (nq + 1), 4 * (nq + 1)):
            offs.append(o)
            o += up(b)
        names = ("desc", "key", "occupied", "query", "cell", "feat", "lev", "rounds", "best_idx", "best_dist", "level", "uv", "state", "rad", "prev")
        assert [f[k] for k in names] == offs
        # SkBatch reads every region where it is: the pairs of equal element size are the ones a swap would not show on the CPU otherwise
        hc.assert_bound(f, [("cell_begin", "cell"), ("cell_feat", "feat")] + [(k, k) for k in names if k not in ("cell", "feat")])
        assert f["upload"] == offs[7] and f["back"] == offs[13] - offs[7] and f["total"] == o
        d = np.zeros(n, dtype=DESC)
        ok = oq = oc = of = ol = 0
        for k, p in enumerate(ps):
            d[k]["off"] = [ok, oq, oc, of, ol]
            d[k]["i"] = [p.n_keys, p.n_q, p.n_levels, p.th_dist, p.grid_cols, p.grid_rows, int(p.reloc), 0]
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
        assert (f["got_bi"], f["got_bd"], f["got_lv"], f["got_uv8"]) == (s["bi"], s["bd"], s["lv"], s["uv"])
        assert (f["got_st"], f["got_bin"], f["got_km"], f["got_hist"], f["got_ind"]) == (s["st"], s["bin"], s["km"], s["hist"], s["ind"])
        dropped += s["before"] - s["match"]
    assert dropped > 50            # the drop of the orientation filter ran


def test_write_back_two_matches_in_a_dropped_bin_by_hand(checker, tmp_path):
    """22 queries over 128 keypoints in reloc mode: the synthetic result matches the queries 0, 3, .. 21 on the keypoints 0, 15, .. 105
    (5 i mod 128).  Their angles put them pairwise into the bins 0, 1, 2 and 3; ComputeThreeMaxima keeps 0, 1 and 2 (a later bin
    needs MORE entries to displace one), so bin 3 is dropped with its two matches: the queries 18 and 21 leave with state 7, the
    keypoints 90 and 105 are cleared, the counts are 8 and 6.  In loop mode the same result keeps all 8 and fills no bin"""
    p = synth.search_proj_kf_scene(5, RELOC, n_keys=128, n_q=22)
    q_angle = np.zeros(22, dtype=np.float32)
    q_angle[::3] = 10.0 + 30.0 * (np.arange(8) // 2)
    p = p.copy(angle=np.full(128, 10.0, dtype=np.float32), q_angle=q_angle)
    path = str(tmp_path / "h.sk")
    _write(path, [(p, {})])
    f = hc.fields(hc.run(checker, [path], 1)[0])
    km = np.full(128, -1)
    km[[0, 15, 30, 45, 60, 75]] = [0, 3, 6, 9, 12, 15]
    km[[90, 105]] = -2
    st = np.where(np.arange(22) % 3 == 0, 0, 1 + np.arange(22) % 8)
    st[[18, 21]] = 7
    bins = np.full(22, 255)
    bins[::3] = np.arange(8) // 2
    assert (f["got_match"], f["got_before"], f["got_hist"], f["got_ind"]) == (6, 8, 2 * (1 + 2 + 3 + 4), 0 * 1 + 1 * 2 + 2 * 3)
    assert f["got_km"] == int((km * (np.arange(128) % 11 + 1)).sum()) and f["got_st"] == int((st * (np.arange(22) % 5 + 1)).sum())
    assert f["got_bin"] == int((bins * (np.arange(22) % 7 + 1)).sum())
    lp = synth.search_proj_kf_scene(5, LOOP, n_keys=128, n_q=22)
    _write(path, [(lp, {})])
    f = hc.fields(hc.run(checker, [path], 1)[0])
    km[[90, 105]] = [18, 21]
    assert (f["got_match"], f["got_before"], f["got_hist"], f["got_ind"]) == (8, 8, 0, -6)
    assert f["got_km"] == int((km * (np.arange(128) % 11 + 1)).sum()) and f["got_bin"] == 255 * int((np.arange(22) % 7 + 1).sum())


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
    (LOOP, dict(n_keys=-1), "negative n_keys"),
    (RELOC, dict(n_q=-2), "negative n_q"),
    (LOOP, dict(mode=2), "unknown mode"),
    (RELOC, dict(mode=-1), "unknown mode"),
    (LOOP, dict(nulls=4), "NULL problem or result"),
    (RELOC, dict(nulls=16), "NULL problem or result"),
    (LOOP, dict(nulls=1), "NULL array with n_keys > 0"),
    (RELOC, dict(nulls=1024), "NULL array with n_keys > 0"),
    (LOOP, dict(nulls=2048), "NULL array with n_keys > 0"),
    (RELOC, dict(nulls=8192), "NULL array with n_keys > 0"),
    (LOOP, dict(nulls=256), "NULL array with n_q > 0"),
    (RELOC, dict(nulls=512), "NULL array with n_q > 0"),
    (LOOP, dict(nulls=2), "NULL array with n_q > 0"),
    (RELOC, dict(nulls=32), "NULL array with n_q > 0"),
    (RELOC, dict(nulls=32768), "NULL array with n_q > 0"),
    (LOOP, dict(nulls=4096), "NULL loop array with n_q > 0"),
    (RELOC, dict(nulls=16384), "NULL reloc array with n_q > 0"),
    (LOOP, dict(nulls=8), "NULL level table"),
    (RELOC, dict(nulls=64), "NULL cell_begin"),
    (LOOP, dict(nulls=128), "NULL cell_feat"),
    (LOOP, dict(n_levels=0), "n_levels outside 1 .. 64"),
    (RELOC, dict(n_levels=65), "n_levels outside 1 .. 64"),
    (LOOP, dict(copy=dict(th_dist=257)), "th_dist outside 0 .. 256"),
    (RELOC, dict(copy=dict(th_dist=-1)), "th_dist outside 0 .. 256"),
    (LOOP, dict(grid_cols=0), "grid size outside 1 .. 65536 cells"),
    (RELOC, dict(grid_cols=65536, grid_rows=2), "grid size outside 1 .. 65536 cells"),
    (LOOP, dict(grid_cols=2147483647, grid_rows=2147483647), "grid size outside 1 .. 65536 cells"),
    (LOOP, dict(edit=dict(oct=(6, 8))), "keypoint 6: octave >= n_levels"),
    (RELOC, dict(edit=dict(uv=(11, np.nan))), "keypoint 5: a pixel is not finite"),
    (RELOC, dict(edit=dict(angle=(3, 360.0))), "keypoint 3: angle outside [0, 360)"),
    (RELOC, dict(edit=dict(angle=(2, np.nan))), "keypoint 2: angle outside [0, 360)"),
    (RELOC, dict(edit=dict(q_angle=(4, -1.0))), "query 4: angle outside [0, 360)"),
    (LOOP, dict(edit=dict(Rcw=(4, np.nan))), "the pose is not finite"),
    (RELOC, dict(edit=dict(tcw=(1, np.inf))), "the pose is not finite"),
    (RELOC, dict(edit=dict(Ow=(2, -np.inf))), "the pose is not finite"),
    (LOOP, dict(edit=dict(K=(0, np.nan))), "an intrinsic is not finite"),
    (RELOC, dict(edit=dict(bounds=(3, np.inf))), "a bound or cell size is not finite"),
    (LOOP, dict(copy=dict(grid_inv_h=np.nan)), "a bound or cell size is not finite"),
    (RELOC, dict(copy=dict(th=np.inf)), "a threshold is not finite"),
    (LOOP, dict(copy=dict(cos_view=np.nan)), "a threshold is not finite"),
    (LOOP, dict(edit=dict(scale=(7, np.nan))), "a level table is not finite"),
    (RELOC, dict(copy=dict(log_scale_factor=np.nan)), "a level table is not finite"),
    (RELOC, dict(edit=dict(q_pos=(10, np.nan))), "query 3: the position is not finite"),
    (LOOP, dict(edit=dict(q_normal=(2, np.inf))), "query 0: the normal is not finite"),
    (RELOC, dict(edit=dict(q_dist_min=(4, np.nan))), "query 4: a distance is not finite"),
    (LOOP, dict(edit=dict(q_dist_max=(5, np.inf))), "query 5: a distance is not finite"),
    (RELOC, dict(edit=dict(q_pred_max=(6, np.nan))), "query 6: a distance is not finite"),
    (LOOP, dict(edit=dict(cell_begin=(0, 1))), "cell_begin does not start at 0"),
    (RELOC, dict(edit=dict(cell_begin=(5, -1))), "cell_begin decreases at cell 4"),
    (LOOP, dict(edit=dict(cell_begin=(3072, 41))), "cell_begin ends above n_keys"),
    (RELOC, dict(edit=dict(cell_feat=(4, 40))), "cell_feat entry 4: keypoint index out of range"),
    (LOOP, dict(edit=dict(cell_feat=(0, -1))), "cell_feat entry 0: keypoint index out of range"),
    (RELOC, dict(dup=1), "cell_feat entry 9: keypoint K listed twice"),
    (LOOP, dict(big=1), "n_keys above 16384: the claim table of a target lives in LDS"),
]


@pytest.mark.parametrize("mode,change,message", REFUSALS, ids=[m.replace(" ", "_").replace("/", "").replace(":", "") + str(k) for k, (_, _, m) in enumerate(REFUSALS)])
def test_refusals(checker, tmp_path, mode, change, message):
    good, bad = synth.search_proj_kf_scene(40, mode, n_keys=40, n_q=20), synth.search_proj_kf_scene(41, mode, n_keys=40, n_q=20)
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
        bad = synth.search_proj_kf_scene(42, mode, n_keys=abi.SEARCH_PROJ_KF_MAX_KEYS + 1, n_q=3, twins=0.0)
    path = str(tmp_path / "r.sk")
    _write(path, [(good, {}), (bad, o)])
    assert hc.run(checker, [path], 1) == ["error problem 1: " + message]


def test_legal_edges(checker, tmp_path):
    """a problem without queries needs no query or per-query result arrays, one without keypoints no keypoint arrays, no key_match and
    no cell_feat; the arrays of the other mode are NULL throughout (the harness passes them so); without check_orientation no angles
    are needed and none is checked; 64 levels and octave 63 are legal; th_dist 0 and 256 are legal; a 65536 x 1 grid is legal; a
    negative th is legal; a target of exactly 16384 keypoints is legal"""
    C = cases_mod.cases()
    e = C["empty_q_reloc"]
    k = C["empty_keys_loop"].copy(th_dist=256, th=-1.0)
    s = 1.01 ** np.arange(64)
    b = synth.search_proj_kf_scene(8, RELOC, n_keys=30, n_q=10, check_orientation=False).copy(scale=s, th_dist=0)
    b = _with(b, oct=(5, 63), angle=(1, 400.0), q_angle=(2, -5.0))
    g = synth.search_proj_kf_scene(9, LOOP, n_keys=20, n_q=300, cols=65536, rows=1)
    m = C["max_keys"]
    path = str(tmp_path / "e.sk")
    _write(path, [(e, dict(nulls=2 | 32 | 256 | 512 | 16384 | 32768)), (k, dict(nulls=1 | 128 | 1024 | 2048)), (b, dict(nulls=8192 | 16384)), (g, {}), (m, {})])
    f = hc.fields(hc.run(checker, [path], 1)[0])
    assert (f["keys"], f["qs"], f["lev_tot"], f["grid"], f["max_keys"], f["lds"]) == (e.n_keys + 30 + 20 + 16384, k.n_q + 10 + 300 + m.n_q, 8 + 8 + 64 + 8 + 8, 5, 16384, 65540)
    assert f["cells"] == 2 * 3073 + 3073 + 65537 + 128 * 96 + 1
