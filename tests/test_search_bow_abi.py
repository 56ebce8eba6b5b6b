"""CPU-side checks of the vba_search_by_bow boundary: the ctypes structs against what gcc makes of include/vislam_ba.h, the symbol in
both library flavours, and no answer without a handle (the library has no CPU path)."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from mc_slam_amd import abi, backend, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_FIELDS = ["mode", "check_orientation", "th_low", "nn_ratio", "n_keys1", "n_keys2", "desc1", "desc2", "good_mp1", "good_mp2", "angle1", "angle2",
            "n_nodes1", "n_nodes2", "node_id1", "node_id2", "node_begin1", "node_begin2", "node_feat1", "node_feat2"]
R_FIELDS = ["status", "n_matches", "n_before_filter", "hist", "ind", "rounds", "match12", "best_idx", "best_dist", "best_dist2", "bin", "state", "match21"]


def test_struct_layout_matches_header(tmp_path):
    pr = ", ".join(["sizeof(vba_search_bow_problem)"] + ["offsetof(vba_search_bow_problem, %s)" % f for f in P_FIELDS] +
                   ["sizeof(vba_search_bow_result)"] + ["offsetof(vba_search_bow_result, %s)" % f for f in R_FIELDS] +
                   ["(size_t)VBA_SEARCH_BOW_KF_FRAME", "(size_t)VBA_SEARCH_BOW_KF_KF", "(size_t)VBA_SEARCH_BOW_MAX_KEYS"])
    n = 5 + len(P_FIELDS) + len(R_FIELDS)
    src = textwrap.dedent('''
        #include <stdio.h>
        #include <stddef.h>
        #include "vislam_ba.h"
        int main(){printf("%s\\n", %s);return 0;}''') % (" ".join(["%zu"] * n), pr)
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    got = list(map(int, subprocess.check_output([exe]).split()))
    want = ([C.sizeof(abi.vba_search_bow_problem)] + [getattr(abi.vba_search_bow_problem, f).offset for f in P_FIELDS] +
            [C.sizeof(abi.vba_search_bow_result)] + [getattr(abi.vba_search_bow_result, f).offset for f in R_FIELDS] +
            [abi.SEARCH_BOW_KF_FRAME, abi.SEARCH_BOW_KF_KF, abi.SEARCH_BOW_MAX_KEYS])
    assert got == want
    assert [f for f, _ in abi.vba_search_bow_problem._fields_] == P_FIELDS and [f for f, _ in abi.vba_search_bow_result._fields_] == R_FIELDS


def test_symbol_in_both_flavours():
    assert "vba_search_by_bow" in backend.EXPORTS
    for hooks in (False, True):
        lib = backend.load_library(hooks)
        assert lib.vba_search_by_bow.argtypes[2] == C.POINTER(C.POINTER(abi.vba_search_bow_problem))


@pytest.mark.parametrize("mode", [abi.SEARCH_BOW_KF_FRAME, abi.SEARCH_BOW_KF_KF])
def test_no_answer_without_a_handle(mode):
    """a NULL handle is refused with -1 and nothing is written; where no device exists no handle can be made at all"""
    lib = backend.load_library()
    p = synth.search_bow_scene(1, mode, n_keys1=40, n_keys2=30, n_nodes=4)
    s, buf = p.as_struct(), abi.SearchBowResultBuf(p)
    pp = (C.POINTER(abi.vba_search_bow_problem) * 1)(C.pointer(s))
    rr = (C.POINTER(abi.vba_search_bow_result) * 1)(C.pointer(buf.s))
    assert lib.vba_search_by_bow(None, 1, pp, rr) == -1
    assert buf.untouched()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            backend.LocalBA(0).search_by_bow([p])


def test_python_views():
    p = synth.search_bow_scene(3, abi.SEARCH_BOW_KF_FRAME, n_keys1=90, n_keys2=50, n_nodes=7)
    assert (p.n_keys1, p.n_keys2) == (90, 50) and p.desc1.shape == (90, 32) and p.desc2.shape == (50, 32) and p.node_begin1.shape == (p.n_nodes1 + 1,)
    assert (p.th_low, p.nn_ratio, p.check_orientation, p.kf_kf) == (50, 0.75, True, False) and p.angle1.dtype == np.float32 and p.good_mp2 is None
    assert p.node_id1.dtype == np.uint32 and (np.diff(p.node_id1.astype(np.int64)) > 0).all() and sorted(p.node_feat2.tolist()) == list(range(50))
    s = p.as_struct()
    assert (s.mode, s.n_keys1, s.n_keys2, s.n_nodes1, s.n_nodes2, s.th_low, s.check_orientation) == (0, 90, 50, p.n_nodes1, p.n_nodes2, 50, 1)
    assert s.desc1[33] == p.desc1[1, 1] and s.angle2[7] == p.angle2[7] and s.node_id2[1] == p.node_id2[1] and s.node_feat1[5] == p.node_feat1[5] and not s.good_mp2
    m = synth.search_bow_scene(3, abi.SEARCH_BOW_KF_KF, n_keys1=90, n_keys2=50, n_nodes=7, nn_ratio=0.7, check_orientation=False)
    assert m.kf_kf and m.nn_ratio == float(np.float32(0.7)) and m.angle1 is None and m.good_mp2.shape == (50,)
    t = m.as_struct()
    assert t.mode == 1 and t.nn_ratio == np.float32(0.7) and t.good_mp2[4] == m.good_mp2[4] and not t.angle1 and not t.angle2
    q = m.copy(th_low=30, good_mp1=np.ones(90))
    assert q.th_low == 30 and q.good_mp1.dtype == np.uint8 and m.th_low == 50 and not m.good_mp1.all()
    b = abi.SearchBowResultBuf(m)
    assert b.untouched() and b.get().match21.shape == (50,) and b.get().state.shape == (90,)
    # the twins of the scene share a node on both sides unless they were moved
    pair = p.truth["pair"]
    assert len(pair) == int(50 * 0.6)
