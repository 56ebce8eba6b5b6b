"""The host half of vba_posegraph_optimize (validation, free-vertex numbering, block envelope, owner lists) under
AddressSanitizer + UBSan (CPU only): every graph of the GPU tests, every bad input of the entry point, and a 5 000-vertex graph
with a 40-keyframe band.  The harness (tests/host_posegraph_check.cpp) checks the envelope invariants itself."""
import subprocess

import numpy as np
import pytest

import posegraph_cases as pc
from mc_slam_amd import abi
import host_check_lib as hc

MUTATE = dict(n_vertices_neg=1, n_edges_neg=2, n_pt_neg=3, S_null=4, edge_S_null=5, pt_null=6, fixed_null=7)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return hc.build(tmp_path_factory, "host_posegraph_check", pthread=True)


def _write(path, p, mutate=0, env_before=0):
    with open(path, "wb") as f:
        f.write(np.array([p.n_vertices, p.n_edges, p.fix_scale, p.its, p.n_pt, mutate], dtype="<i4").tobytes())
        f.write(np.array([p.lambda_init, env_before], dtype="<f8").tobytes())
        for a in (p.S, p.fixed, p.edge_i, p.edge_j, p.edge_S, p.pt, p.pt_ref):
            f.write(np.ascontiguousarray(a).tobytes())


def _run(checker, tmp_path, items):
    files = []
    for i, it in enumerate(items):
        p, mutate, env_before = it if isinstance(it, tuple) else (it, 0, 0)
        f = str(tmp_path / ("g%d.pg" % i))
        _write(f, p, mutate, env_before)
        files.append(f)
    return hc.run(checker, files, len(items))


def _big(n=5000, band=40, n_loop=8):
    """5 000 vertices, every one tied to its 40 predecessors, a loop of 8 edges over the whole length; identity poses (the host
    side reads the values only to validate them)"""
    i = np.repeat(np.arange(n), band)
    j = i - np.tile(np.arange(1, band + 1), n)
    keep = j >= 0
    ei = np.concatenate([i[keep], n - 1 - np.arange(n_loop)])
    ej = np.concatenate([j[keep], 1 + np.arange(n_loop)])
    unit = np.array([0, 0, 0, 0, 0, 0, 1.0, 1.0])
    fixed = np.zeros(n, dtype=np.uint8)
    fixed[0] = 1
    return abi.PoseGraphProblem(S=np.tile(unit, (n, 1)), fixed=fixed, edge_i=ei, edge_j=ej, edge_S=np.tile(unit, (len(ei), 1)))


def test_every_gpu_graph_has_a_consistent_envelope(checker, tmp_path):
    names = pc.CASES + ["REJECT"]
    ps = [pc.case(n) for n in names]
    got = dict(zip(names, map(hc.fields, _run(checker, tmp_path, ps))))
    for n, p in zip(names, ps):
        f = got[n]
        assert f["n_free"] == int((p.fixed == 0).sum())
        assert f["inc"] == int((p.fixed[p.edge_i] == 0).sum() + (p.fixed[p.edge_j] == 0).sum())
        assert f["pair_edges"] == int(((p.fixed[p.edge_i] == 0) & (p.fixed[p.edge_j] == 0)).sum())
    assert got["TWO_I"]["env"] == got["TWO_J"]["env"] == 1 and got["TWO_I"]["pairs"] == 0
    assert got["ARROW"]["widest"] == 11 and got["ARROW"]["env"] == 1 + 2 * 9 + 11      # vertex 0 fixed: rows of 1, 2 ... 2, then (1, 11)
    assert got["MID"]["widest"] == 10 and got["MID"]["n_free"] == 11                   # free numbering skips vertex 5
    assert got["BAND"]["pair_edges"] == got["BAND"]["pairs"] + 1                       # the duplicated edge shares its pair
    assert got["BAND"]["n_free"] == 70 and got["BAND"]["widest"] == 68              # rows of 66..69 reach back to vertex 2
    assert got["NEST"]["widest"] == 129 and got["NEST"]["env"] == 1 + 2 + 3 * 127 + 126 + 48    # the loop (90, 40) inside the loop (129, 1)


def test_five_thousand_vertices_fit_the_bound_eight_times(checker, tmp_path):
    p = _big()
    f = hc.fields(_run(checker, tmp_path, [p])[0])
    assert f["n_free"] == 4999 and f["widest"] == 4999
    assert f["env"] * 8 <= 2 ** 21
    line = _run(checker, tmp_path, [(p, 0, 2 ** 21 - f["env"] + 1)])[0]                 # the bound holds for the whole call
    assert line.startswith("error ") and "exceeds the bound of 2097152 blocks" in line
    assert _run(checker, tmp_path, [(p, 0, 2 ** 21 - f["env"])])[0].startswith("ok ")


def test_bad_graphs_are_refused_with_a_message(checker, tmp_path):
    from test_gpu_posegraph import _bad_graphs
    bad = _bad_graphs()
    for (q, msg), line in zip(bad, _run(checker, tmp_path, [b[0] for b in bad])):
        assert line.startswith("error ") and msg in line, (msg, line)
    p = pc.case("BIG")
    muts = [("n_vertices_neg", "negative count"), ("n_edges_neg", "negative count"), ("n_pt_neg", "negative count"),
            ("S_null", "NULL array"), ("edge_S_null", "NULL array"), ("pt_null", "NULL array"), ("fixed_null", "NULL array")]
    for (m, msg), line in zip(muts, _run(checker, tmp_path, [(p, MUTATE[m], 0) for m, _ in muts])):
        assert line.startswith("error ") and msg in line, (m, line)
    # a truncated file is refused by the harness' reader, not read out of bounds
    f = str(tmp_path / "t.pg")
    _write(f, p)
    raw = open(f, "rb").read()
    open(f, "wb").write(raw[:len(raw) // 2])
    r = subprocess.run([checker, f], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("error load") and "ERROR" not in r.stderr


def _layout_sizes(p):
    """free count, envelope rows and list totals of one graph, from its edges alone"""
    free_of = np.cumsum(p.fixed == 0) - 1
    free_of[p.fixed != 0] = -1
    nf = int((p.fixed == 0).sum())
    a, b = free_of[p.edge_i], free_of[p.edge_j]
    both = (a >= 0) & (b >= 0)
    first = np.arange(nf)
    np.minimum.at(first, np.maximum(a, b)[both], np.minimum(a, b)[both])
    pairs = {(max(x, y), min(x, y)) for x, y in zip(a[both], b[both])}
    return dict(nv=p.n_vertices, ne=p.n_edges, nf=nf, nenv=int((np.arange(nf) - first + 1).sum()), ninc=int((a >= 0).sum() + (b >= 0).sum()),
                npair=len(pairs), npe=int(both.sum()), npt=p.n_pt), first


def test_arena_of_a_two_graph_call(checker, tmp_path):
    """every region of the arena [upload | back | work] sits where the entry point has always put it: in this order, each
    (bytes + 8) rounded up to 256, nothing overlapping; packing runs into a block of exactly the upload section"""
    ps = [pc.case("ARROW"), pc.case("BIG")]                     # the graph with map points second: its references move by the first one's vertices
    files = []
    for i, p in enumerate(ps):
        files.append(str(tmp_path / ("c%d.pg" % i)))
        _write(files[-1], p)
    t = hc.run(checker, ["--call"] + files, 1)[0].split()
    assert t[0] == "call" and t[23] == "offsets"
    got = {k: int(v) for k, v in zip(t[1:23:2], t[2:23:2])}
    offs = [int(v) for v in t[24:55]]
    s = {k: sum(_layout_sizes(p)[0][k] for p in ps) for k in ("nv", "ne", "nf", "nenv", "ninc", "npair", "npe", "npt")}
    assert {k: got[k] for k in s} == s and s["npt"] > 0
    G, nv, ne, nf, nenv, npt = 2, s["nv"], s["ne"], s["nf"], s["nenv"], s["npt"]
    upload = [120 * G, 64 * nv, 64 * ne, 4 * ne, 4 * ne, 4 * nv, 4 * nf, 4 * nf, 4 * nf, 4 * (nf + G), 4 * (nf + G), 4 * s["ninc"], 4 * s["npair"],
              4 * s["npair"], 4 * (s["npair"] + G), 4 * s["npe"], 24 * npt, 4 * npt]
    back = [40 * G, 64 * nv, 24 * npt]
    work = [64 * nv, 56 * ne, 784 * ne, 392 * nenv, 392 * nenv, 392 * nf, 56 * nf, 56 * nf, 56 * nf, 56 * nf]
    sizes = upload + back + work
    assert len(offs) == len(sizes) == 31
    assert all(o % 256 == 0 for o in offs) and offs[0] == 0                                       # aligned
    assert all(offs[k] + sizes[k] + 8 <= offs[k + 1] for k in range(30))                          # in today's order, disjoint (slack of 8 included)
    assert offs[30] + sizes[30] + 8 <= got["total"]
    want = np.concatenate([[0], np.cumsum([(b + 8 + 255) // 256 * 256 for b in sizes])])
    assert offs == want[:31].tolist()                                                              # and exactly where they were
    assert (got["upload"], got["back"], got["total"]) == (want[18], want[21] - want[18], want[31])
    assert t[55] == "last_ref" and int(t[56]) == ps[0].n_vertices + int(ps[1].pt_ref[-1])
    # PgBatch reads every region where it is, and knows the call's points
    assert t[57] == "bind" and [int(v) for v in t[58:89]] == offs and t[89:91] == ["n_pt_total", str(npt)]
    # the write-back of a synthetic result (see the harness): graph g says g, the estimates come back as 0, 1, 2, ..., the points as -0, -1, ...
    assert t[91:] == ["got_its", "1", "got_S", str(8 * nv * (8 * nv - 1) // 2), "got_pt", str(-(3 * npt * (3 * npt - 1) // 2))]


def test_dense_expansion_of_a_three_vertex_envelope(checker, tmp_path):
    """vertex 0 fixed, a chain 1 - 2 - 3: the envelope holds (0,0), (1,0), (1,1), (2,1), (2,2) and no block (2,0)"""
    from mc_slam_amd import synth
    p = synth.make_posegraph(3, 4, span=1, fixed_at=0)
    sizes, first = _layout_sizes(p)
    assert sizes["nf"] == 3 and first.tolist() == [0, 0, 1]
    f = str(tmp_path / "e.pg")
    _write(f, p)
    t = hc.run(checker, ["--expand", f], 1)[0].split()
    assert t[:3] == ["expand", "n_free", "3"] and [int(v) for v in t[4:7]] == first.tolist() and t[7] == "H"
    H = np.array(t[8:], dtype=float).reshape(21, 21)
    assert np.array_equal(H, H.T)
    q = 0
    for row in range(3):
        for col in range(3):
            blk = H[7 * row:7 * row + 7, 7 * col:7 * col + 7]
            if first[row] <= col <= row:                 # block q of the envelope, row by row: 100 q + 7 a + k + 1 at (a, k)
                want = 100 * q + np.arange(1, 50).reshape(7, 7)
                assert np.array_equal(blk, want if col < row else np.triu(want) + np.triu(want, 1).T), (row, col)
                q += 1
            elif col <= row:
                assert not blk.any(), (row, col)
    assert q == sizes["nenv"] == 5
