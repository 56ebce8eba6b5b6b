"""The host half of vba_fuse (mc_slam_amd/csrc/vba_host_fuse.h, vba_host_arena.h: refusals, arena offsets, the tile table, the keypoint
and point records, the grid copy, write-back with n_found) under AddressSanitizer + UBSan (CPU only).  The harness
(tests/host_fuse_check.cpp) packs into heap blocks of exactly the arena's sizes; every expected offset below is restated from the
sizes alone and the packed regions are compared with records built in NumPy through an order-sensitive checksum."""
import numpy as np
import pytest

from mc_slam_amd import synth
import fuse_cases as cases_mod
import host_check_lib as hc
from host_check_lib import checksum, up

DESC = np.dtype([("off", "<i8", 5), ("i", "<i4", 8), ("c", "<f8", 29)])
KEY = np.dtype([("d", "u1", 32), ("u", "<f8"), ("v", "<f8"), ("oct", "u1"), ("pad", "u1", 15)])
PT = np.dtype([("d", "u1", 32), ("pos", "<f8", 3), ("normal", "<f8", 3), ("dist", "<f8", 3), ("skip", "<i4"), ("pad", "<i4", 5)])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return hc.build(tmp_path_factory, "host_fuse_check", pthread=True)


def consts(p):
    return np.concatenate([p.Rcw.ravel(), p.tcw, p.Ow, p.K, p.bounds, [p.grid_inv_w, p.grid_inv_h, p.log_scale_factor, p.th, p.cos_view, p.chi2_reproj]])


def _write(path, items):
    """items: (problem, dict of n_keys / n_pt / n_levels / grid_cols / grid_rows / nulls overrides)"""
    with open(path, "wb") as f:
        f.write(np.array([len(items)], dtype="<i4").tobytes())
        for p, o in items:
            f.write(np.array([o.get("n_keys", p.n_keys), p.n_keys, o.get("n_pt", p.n_pt), p.n_pt, o.get("n_levels", p.n_levels), p.n_levels,
                              o.get("grid_cols", p.grid_cols), o.get("grid_rows", p.grid_rows), len(p.cell_begin), len(p.cell_feat), p.th_low,
                              int(p.check_reproj), o.get("nulls", 0)], dtype="<i4").tobytes())
            f.write(consts(p).astype("<f8").tobytes())
            f.write(p.desc.tobytes()); f.write(p.uv.astype("<f8").tobytes()); f.write(p.oct.tobytes())
            f.write(p.scale.astype("<f8").tobytes()); f.write(p.inv_level_sigma2.astype("<f8").tobytes())
            f.write(p.cell_begin.astype("<i4").tobytes()); f.write(p.cell_feat.astype("<i4").tobytes())
            for a in (p.pos, p.normal, p.dist_min, p.dist_max, p.pred_max):
                f.write(a.astype("<f8").tobytes())
            f.write(p.pt_desc.tobytes()); f.write(p.skip.tobytes())


def keys(p):
    k = np.zeros(p.n_keys, dtype=KEY)
    k["d"], k["u"], k["v"], k["oct"] = p.desc, p.uv[:, 0], p.uv[:, 1], p.oct
    return k


def points(p):
    q = np.zeros(p.n_pt, dtype=PT)
    q["d"], q["pos"], q["normal"], q["skip"] = p.pt_desc, p.pos, p.normal, p.skip != 0
    q["dist"] = np.stack([p.dist_min, p.dist_max, p.pred_max], axis=1).reshape(-1, 3)
    return q


def _batches():
    C = cases_mod.cases()
    many = [synth.fuse_scene(700 + k, n_keys=(k * 5) % 23, n_pt=(k * 7) % 5 * (k % 3), n_levels=1 + k % 8, cols=1 + k % 5, rows=1 + k % 3,
                             check_reproj=bool(k % 2)) for k in range(300)]   # the threaded path, a third without points
    return [[C["empty_pt"]], [C["micro"]], [C["tiles_257"], C["empty_keys"], C["tiles_513"], C["empty_pt"], C["tiles_256"], C["z_zero"]], list(C.values()), many]


def test_offsets_tiles_packing_and_write_back(checker, tmp_path):
    batches = _batches()
    files = []
    for k, ps in enumerate(batches):
        files.append(str(tmp_path / ("b%d.fu" % k)))
        _write(files[-1], [(p, {}) for p in ps])
    for ps, line in zip(batches, hc.run(checker, files, len(files))):
        f = hc.fields(line)
        n = len(ps)
        nk, npt = sum(p.n_keys for p in ps), sum(p.n_pt for p in ps)
        nc, ft, lv = sum(len(p.cell_begin) for p in ps), sum(len(p.cell_feat) for p in ps), sum(2 * p.n_levels for p in ps)
        tiles = [(k, first) for k, p in enumerate(ps) for first in range(0, p.n_pt, 256)]
        assert (f["keys"], f["pts"], f["cells"], f["feat_tot"], f["lev_tot"], f["tiles"], f["n_tiles"]) == (nk, npt, nc, ft, lv, len(tiles), len(tiles))
        # the arena, restated from the sizes: seven upload regions, five back regions, nothing device-only
        assert DESC.itemsize == 304 and KEY.itemsize == 64 and PT.itemsize == 128
        o, offs = 0, []
        for b in (304 * n, 8 * (len(tiles) + 1), 64 * (nk + 1), 128 * (npt + 1), 4 * (nc + 1), 4 * (ft + 1), 8 * (lv + 1),
                  4 * (npt + 1), 2 * (npt + 1), npt + 1, 16 * (npt + 1), npt + 1):
            offs.append(o)
            o += up(b)
        assert [f[k] for k in ("desc", "tile", "key", "pt", "cell", "feat", "lev", "best_idx", "best_dist", "level", "uv", "state")] == offs
        # FuBatch reads every region where it is: the two grid copies are the pair that a swap would not show on the CPU otherwise
        hc.assert_bound(f, [("cell_begin", "cell"), ("cell_feat", "feat")] +
                        [(k, k) for k in ("desc", "tile", "key", "pt", "lev", "best_idx", "best_dist", "level", "uv", "state")])
        assert f["upload"] == offs[7] and f["back"] == o - offs[7] and f["total"] == o
        d = np.zeros(n, dtype=DESC)
        ok = op = oc = of = ol = 0
        for k, p in enumerate(ps):
            d[k]["off"] = [ok, op, oc, of, ol]
            d[k]["i"] = [p.n_keys, p.n_pt, p.n_levels, p.th_low, p.grid_cols, p.grid_rows, int(p.check_reproj), 0]
            d[k]["c"] = consts(p)
            ok += p.n_keys; op += p.n_pt; oc += len(p.cell_begin); of += len(p.cell_feat); ol += 2 * p.n_levels
        assert f["sum_desc"] == checksum(d)
        assert f["sum_tile"] == checksum(np.array(tiles, dtype="<i4").reshape(-1, 2))
        assert f["sum_key"] == checksum(*[keys(p) for p in ps])
        assert f["sum_pt"] == checksum(*[points(p) for p in ps])
        assert f["sum_cell"] == checksum(*[p.cell_begin for p in ps])
        assert f["sum_feat"] == checksum(*[p.cell_feat for p in ps])
        assert f["sum_lev"] == checksum(*[np.concatenate([p.scale, p.inv_level_sigma2]) for p in ps])
        # the write-back of the synthetic result (see the harness)
        i = np.arange(npt)
        found, o1 = 0, 0
        for k, p in enumerate(ps):
            found += int((i[o1:o1 + p.n_pt] % 9 == 0).sum()) * (k + 1)
            o1 += p.n_pt
        assert (f["got_found"], f["got_status"]) == (found, 0)
        assert (f["got_bi"], f["got_bd"], f["got_lv"], f["got_st"], f["got_uv8"]) == (int((i % 7 - 1).sum()), int((i % 257).sum()), int((i % 200 - 128).sum()),
                                                                                        int((i % 9).sum()), -int(i.sum()))


def _with(p, **kw):
    """a copy of p with single entries of its arrays replaced: name=(index, value)"""
    ch = {}
    for k, (i, v) in kw.items():
        a = getattr(p, k).copy()
        a.reshape(-1)[i] = v
        ch[k] = a
    return p.copy(**ch)


REFUSALS = [
    (dict(n_keys=-1), "problem 1: negative n_keys"),
    (dict(n_pt=-2), "problem 1: negative n_pt"),
    (dict(nulls=4), "problem 1: NULL problem or result"),
    (dict(nulls=16), "problem 1: NULL problem or result"),
    (dict(nulls=1), "problem 1: NULL array with n_keys > 0"),
    (dict(nulls=1024), "problem 1: NULL array with n_keys > 0"),
    (dict(nulls=256), "problem 1: NULL array with n_pt > 0"),
    (dict(nulls=512), "problem 1: NULL array with n_pt > 0"),
    (dict(nulls=2), "problem 1: NULL array with n_pt > 0"),
    (dict(nulls=32), "problem 1: NULL array with n_pt > 0"),
    (dict(nulls=2048), "problem 1: NULL array with n_pt > 0"),
    (dict(nulls=8), "problem 1: NULL level table"),
    (dict(nulls=64), "problem 1: NULL cell_begin"),
    (dict(nulls=128), "problem 1: NULL cell_feat"),
    (dict(n_levels=0), "problem 1: n_levels outside 1 .. 64"),
    (dict(n_levels=65), "problem 1: n_levels outside 1 .. 64"),
    (dict(copy=dict(th_low=257)), "problem 1: th_low outside 0 .. 256"),
    (dict(copy=dict(th_low=-1)), "problem 1: th_low outside 0 .. 256"),
    (dict(grid_cols=0), "problem 1: grid size outside 1 .. 65536 cells"),
    (dict(grid_rows=-3), "problem 1: grid size outside 1 .. 65536 cells"),
    (dict(grid_cols=65536, grid_rows=2), "problem 1: grid size outside 1 .. 65536 cells"),
    (dict(grid_cols=2147483647, grid_rows=2147483647), "problem 1: grid size outside 1 .. 65536 cells"),
    (dict(edit=dict(oct=(6, 8))), "problem 1: keypoint 6: octave >= n_levels"),
    (dict(edit=dict(uv=(11, np.nan))), "problem 1: keypoint 5: a pixel is not finite"),
    (dict(edit=dict(Rcw=(4, np.nan))), "problem 1: the pose is not finite"),
    (dict(edit=dict(tcw=(1, np.inf))), "problem 1: the pose is not finite"),
    (dict(edit=dict(Ow=(2, -np.inf))), "problem 1: the pose is not finite"),
    (dict(edit=dict(K=(0, np.nan))), "problem 1: an intrinsic is not finite"),
    (dict(edit=dict(bounds=(3, np.inf))), "problem 1: a bound or cell size is not finite"),
    (dict(copy=dict(grid_inv_h=np.nan)), "problem 1: a bound or cell size is not finite"),
    (dict(copy=dict(th=np.inf)), "problem 1: a threshold is not finite"),
    (dict(copy=dict(cos_view=np.nan)), "problem 1: a threshold is not finite"),
    (dict(copy=dict(chi2_reproj=np.nan)), "problem 1: a threshold is not finite"),
    (dict(edit=dict(scale=(7, np.nan))), "problem 1: a level table is not finite"),
    (dict(edit=dict(inv_level_sigma2=(0, np.inf))), "problem 1: a level table is not finite"),
    (dict(copy=dict(log_scale_factor=np.nan)), "problem 1: a level table is not finite"),
    (dict(edit=dict(pos=(10, np.nan))), "problem 1: point 3: the position is not finite"),
    (dict(edit=dict(normal=(2, np.inf))), "problem 1: point 0: the normal is not finite"),
    (dict(edit=dict(dist_min=(4, np.nan))), "problem 1: point 4: a distance is not finite"),
    (dict(edit=dict(dist_max=(5, np.inf))), "problem 1: point 5: a distance is not finite"),
    (dict(edit=dict(pred_max=(6, np.nan))), "problem 1: point 6: a distance is not finite"),
    (dict(edit=dict(cell_begin=(0, 1))), "problem 1: cell_begin does not start at 0"),
    (dict(edit=dict(cell_begin=(5, -1))), "problem 1: cell_begin decreases at cell 4"),
    (dict(edit=dict(cell_begin=(3072, 41))), "problem 1: cell_begin ends above n_keys"),
    (dict(edit=dict(cell_feat=(4, 40))), "problem 1: cell_feat entry 4: keypoint index out of range"),
    (dict(edit=dict(cell_feat=(0, -1))), "problem 1: cell_feat entry 0: keypoint index out of range"),
    (dict(dup=1), "problem 1: cell_feat entry 9: keypoint K listed twice"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m.split(": ", 1)[1].replace(" ", "_").replace("/", "") + str(k) for k, (_, m) in enumerate(REFUSALS)])
def test_refusals(checker, tmp_path, change, message):
    good, bad = synth.fuse_scene(40, n_keys=40, n_pt=20), synth.fuse_scene(41, n_keys=40, n_pt=20)
    assert len(bad.cell_feat) > 10
    o = {k: v for k, v in change.items() if k in ("n_keys", "n_pt", "n_levels", "grid_cols", "grid_rows", "nulls")}
    if "edit" in change:
        bad = _with(bad, **change["edit"])
    if "copy" in change:
        bad = bad.copy(**change["copy"])
    if "dup" in change:
        a = bad.cell_feat.copy()
        a[9] = a[2]
        message = message.replace("K", str(a[2]))
        bad = bad.copy(cell_feat=a)
    path = str(tmp_path / "r.fu")
    _write(path, [(good, {}), (bad, o)])
    assert hc.run(checker, [path], 1) == ["error " + message]


def test_legal_edges(checker, tmp_path):
    """a problem without points needs no point or result arrays, one without keypoints no keypoint arrays and no cell_feat; 64 levels
    and octave 63 are legal; th_low 0 and 256 are legal; a 65536 x 1 grid is legal; a negative th is legal"""
    e = cases_mod.cases()["empty_pt"]
    k = cases_mod.cases()["empty_keys"].copy(th_low=256, th=-1.0)
    s = 1.01 ** np.arange(64)
    b = synth.fuse_scene(8, n_keys=30, n_pt=10).copy(scale=s, inv_level_sigma2=1 / (s * s), th_low=0)
    b = _with(b, oct=(5, 63))
    g = synth.fuse_scene(9, n_keys=20, n_pt=300, cols=65536, rows=1)
    path = str(tmp_path / "e.fu")
    _write(path, [(e, dict(nulls=2 | 32 | 256 | 512 | 2048)), (k, dict(nulls=1 | 128 | 1024)), (b, {}), (g, {})])
    f = hc.fields(hc.run(checker, [path], 1)[0])
    assert (f["keys"], f["pts"], f["lev_tot"], f["tiles"], f["cells"]) == (e.n_keys + 30 + 20, k.n_pt + 10 + 300, 16 + 16 + 128 + 16, 1 + 1 + 2, 2 * 3073 + 3073 + 65537)
