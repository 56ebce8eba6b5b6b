"""CPU-side checks of the vba_search_for_initialization boundary: the ctypes structs against what gcc makes of include/vislam_ba.h, the
symbol in both library flavours, and no answer without a handle (the library has no CPU path)."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from mc_slam_amd import abi, backend, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_FIELDS = ["check_orientation", "th_low", "nn_ratio", "window_size", "n_keys1", "desc1", "oct1", "angle1", "prev_matched", "n_keys2", "desc2", "uv2",
            "oct2", "angle2", "bounds", "grid_cols", "grid_rows", "grid_inv_w", "grid_inv_h", "cell_begin", "cell_feat"]
R_FIELDS = ["status", "n_matches", "n_before_filter", "n_stolen", "hist", "ind", "rounds", "match12", "best_idx", "best_dist", "best_dist2", "bin", "state",
            "prev_matched", "match21", "matched_dist"]


def test_struct_layout_matches_header(tmp_path):
    pr = ", ".join(["sizeof(vba_search_init_problem)"] + ["offsetof(vba_search_init_problem, %s)" % f for f in P_FIELDS] +
                   ["sizeof(vba_search_init_result)"] + ["offsetof(vba_search_init_result, %s)" % f for f in R_FIELDS] +
                   ["(size_t)VBA_SEARCH_INIT_MAX_KEYS"])
    n = 3 + len(P_FIELDS) + len(R_FIELDS)
    src = textwrap.dedent('''
        #include <stdio.h>
        #include <stddef.h>
        #include "vislam_ba.h"
        int main(){printf("%s\\n", %s);return 0;}''') % (" ".join(["%zu"] * n), pr)
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    got = list(map(int, subprocess.check_output([exe]).split()))
    want = ([C.sizeof(abi.vba_search_init_problem)] + [getattr(abi.vba_search_init_problem, f).offset for f in P_FIELDS] +
            [C.sizeof(abi.vba_search_init_result)] + [getattr(abi.vba_search_init_result, f).offset for f in R_FIELDS] + [abi.SEARCH_INIT_MAX_KEYS])
    assert got == want
    assert [f for f, _ in abi.vba_search_init_problem._fields_] == P_FIELDS and [f for f, _ in abi.vba_search_init_result._fields_] == R_FIELDS


def test_symbol_in_both_flavours():
    assert "vba_search_for_initialization" in backend.EXPORTS
    for hooks in (False, True):
        lib = backend.load_library(hooks)
        assert lib.vba_search_for_initialization.argtypes[2] == C.POINTER(C.POINTER(abi.vba_search_init_problem))
        out = subprocess.check_output(["nm", "-D", "--defined-only", backend.HOOKS_LIB_PATH if hooks else backend.LIB_PATH], text=True)
        assert any(l.split()[-1] == "vba_search_for_initialization" for l in out.splitlines() if l.split())


def test_no_answer_without_a_handle():
    """a NULL handle is refused with -1 and nothing is written; where no device exists no handle can be made at all"""
    lib = backend.load_library()
    p = synth.search_init_scene(1, n_keys1=40, n_keys2=30)
    s, buf = p.as_struct(), abi.SearchInitResultBuf(p)
    pp = (C.POINTER(abi.vba_search_init_problem) * 1)(C.pointer(s))
    rr = (C.POINTER(abi.vba_search_init_result) * 1)(C.pointer(buf.s))
    assert lib.vba_search_for_initialization(None, 1, pp, rr) == -1
    assert buf.untouched()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            backend.LocalBA(0).search_for_initialization([p])


def test_python_views():
    p = synth.search_init_scene(3, n_keys1=90, n_keys2=70)
    assert (p.n_keys1, p.n_keys2) == (90, 70) and p.desc1.shape == (90, 32) and p.desc2.shape == (70, 32) and p.cell_begin.shape == (64 * 48 + 1,)
    assert (p.window_size, p.th_low, p.check_orientation) == (100.0, 50, True) and p.nn_ratio == float(np.float32(0.9))
    assert p.prev_matched.dtype == np.float32 and p.prev_matched.shape == (90, 2) and p.uv2.dtype == np.float64 and p.n_q == int((p.oct1 == 0).sum())
    # off the integer lattice: eighths in frame 2, quarters in vbPrevMatched
    assert (np.mod(p.uv2 * 8, 2) == 1).all() and (np.mod(p.prev_matched.astype(np.float64) * 4, 2) == 1).all()
    s = p.as_struct()
    assert (s.n_keys1, s.n_keys2, s.grid_cols, s.grid_rows, s.th_low, s.check_orientation) == (90, 70, 64, 48, 50, 1)
    assert s.prev_matched[5] == p.prev_matched[2, 1] and s.uv2[7] == p.uv2[3, 1] and s.angle1[4] == p.angle1[4] and s.bounds[1] == 640.0
    q = p.copy(window_size=10.0, check_orientation=False, angle1=None, angle2=None, oct1=np.ones(90))
    assert (q.window_size, q.n_q) == (10.0, 0) and q.oct1.dtype == np.uint8 and p.window_size == 100.0 and not q.as_struct().angle1
    b = abi.SearchInitResultBuf(p)
    assert b.untouched() and b.get().match12.shape == (90,) and b.get().match21.shape == (70,) and b.get().prev_matched.shape == (90, 2)
