"""CPU-side checks of the vba_search_triangulation boundary: the ctypes structs against what gcc makes of include/vislam_ba.h, the
symbol in both library flavours, and no answer without a handle (the library has no CPU path)."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from mc_slam_amd import abi, backend, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_FIELDS = ["n_keys1", "n_keys2", "desc1", "desc2", "has_mp1", "has_mp2", "n_nodes1", "n_nodes2", "node_id1", "node_id2", "node_begin1", "node_begin2",
            "node_feat1", "node_feat2", "uv1", "uv2", "angle1", "angle2", "oct2", "n_levels2", "level_sigma2_2", "scale_2", "F12", "epipole", "th_low",
            "check_orientation", "chi2_epi", "epipole_r2"]
R_FIELDS = ["status", "n_matches", "n_before_filter", "hist", "ind", "match12", "best_dist", "state", "pairs"]


def test_struct_layout_matches_header(tmp_path):
    pr = ", ".join(["sizeof(vba_search_tri_problem)"] + ["offsetof(vba_search_tri_problem, %s)" % f for f in P_FIELDS] +
                   ["sizeof(vba_search_tri_result)"] + ["offsetof(vba_search_tri_result, %s)" % f for f in R_FIELDS])
    n = 2 + len(P_FIELDS) + len(R_FIELDS)
    src = textwrap.dedent('''
        #include <stdio.h>
        #include <stddef.h>
        #include "vislam_ba.h"
        int main(){printf("%s\\n", %s);return 0;}''') % (" ".join(["%zu"] * n), pr)
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    got = list(map(int, subprocess.check_output([exe]).split()))
    want = ([C.sizeof(abi.vba_search_tri_problem)] + [getattr(abi.vba_search_tri_problem, f).offset for f in P_FIELDS] +
            [C.sizeof(abi.vba_search_tri_result)] + [getattr(abi.vba_search_tri_result, f).offset for f in R_FIELDS])
    assert got == want
    assert [f for f, _ in abi.vba_search_tri_problem._fields_] == P_FIELDS and [f for f, _ in abi.vba_search_tri_result._fields_] == R_FIELDS


def test_symbol_in_both_flavours():
    assert "vba_search_triangulation" in backend.EXPORTS
    for hooks in (False, True):
        lib = backend.load_library(hooks)
        assert lib.vba_search_triangulation.argtypes[2] == C.POINTER(C.POINTER(abi.vba_search_tri_problem))


def test_no_answer_without_a_handle():
    """a NULL handle is refused with -1 and nothing is written; where no device exists no handle can be made at all"""
    lib = backend.load_library()
    p = synth.synth_match_pair(1)
    s, buf = p.as_struct(), abi.SearchTriResultBuf(p)
    buf.s.n_matches = 12345
    pp = (C.POINTER(abi.vba_search_tri_problem) * 1)(C.pointer(s))
    rr = (C.POINTER(abi.vba_search_tri_result) * 1)(C.pointer(buf.s))
    assert lib.vba_search_triangulation(None, 1, pp, rr) == -1
    assert buf.s.n_matches == 12345 and (buf.st == 255).all() and (buf.m12 == -7).all()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            backend.LocalBA(0).search_triangulation([p])


def test_python_views():
    p = synth.synth_match_pair(3, n_true=30, n_distract1=5, n_distract2=9)
    assert (p.n_keys1, p.n_keys2, p.n_levels2) == (35, 39, 8) and p.desc1.shape == (35, 32) and p.angle2.dtype == np.float32
    for a in (p.uv1, p.uv2, p.F12, p.epipole, p.scale_2, p.level_sigma2_2):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))          # everything went through float32
    assert (p.th_low, p.chi2_epi, p.epipole_r2, p.check_orientation) == (50, 3.84, 100.0, True)
    assert (p.angle1 >= 0).all() and (p.angle1 < 360).all() and (p.angle2 >= 0).all() and (p.angle2 < 360).all()
    for ids, begin, feat, n in ((p.node_id1, p.node_begin1, p.node_feat1, 35), (p.node_id2, p.node_begin2, p.node_feat2, 39)):
        assert (np.diff(ids.astype(np.int64)) > 0).all() and begin[0] == 0 and begin[-1] == len(feat) == n and sorted(feat) == list(range(n))
    t = p.truth["pair"]
    d = np.unpackbits(p.desc1[t[:, 0]] ^ p.desc2[t[:, 1]], axis=1).sum(axis=1)
    assert d.max() <= 24 and d.min() >= 0                                           # two copies with 12 flipped bits each
    x1 = np.hstack([p.uv1[t[:, 0]], np.ones((30, 1))]); x2 = np.hstack([p.uv2[t[:, 1]], np.ones((30, 1))])
    l = x1 @ p.F12
    assert (np.abs((l * x2).sum(axis=1)) / np.hypot(l[:, 0], l[:, 1])).max() < 4.0  # true pairs lie on each other's epipolar lines (pixels)
    s = p.as_struct()
    assert (s.n_keys1, s.n_nodes1, s.th_low, s.check_orientation) == (35, len(p.node_id1), 50, 1) and s.F12[5] == p.F12[1, 2]
    assert abi.feat_vec_csr({7: [3, 1], 2: [0]})[0].tolist() == [2, 7] and abi.feat_vec_csr({7: [3, 1], 2: [0]})[2].tolist() == [0, 3, 1]
