"""CPU-side checks of the vba_search_by_sim3 boundary: the ctypes structs against what gcc makes of include/vislam_ba.h, the symbol in
both library flavours, and no answer without a handle (the library has no CPU path)."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from mc_slam_amd import abi, backend, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KF_FIELDS = ["Rcw", "tcw", "bounds", "n_keys", "n_levels", "desc", "uv", "oct", "scale", "log_scale_factor", "grid_cols", "grid_rows", "grid_inv_w",
             "grid_inv_h", "cell_begin", "cell_feat", "has_pt", "matched", "pos", "dist_min", "dist_max", "pred_max", "pt_desc"]
P_FIELDS = ["kf1", "kf2", "K", "s12", "R12", "t12", "th", "th_high"]
R_FIELDS = ["status", "n_found", "match1", "match2", "best_dist1", "best_dist2", "level1", "level2", "state1", "state2", "match12"]
STRUCTS = (("vba_search_sim3_kf", KF_FIELDS), ("vba_search_sim3_problem", P_FIELDS), ("vba_search_sim3_result", R_FIELDS))


def test_struct_layout_matches_header(tmp_path):
    pr = ", ".join(x for name, fields in STRUCTS for x in ["sizeof(%s)" % name] + ["offsetof(%s, %s)" % (name, f) for f in fields])
    n = sum(1 + len(fields) for _, fields in STRUCTS)
    src = textwrap.dedent('''
        #include <stdio.h>
        #include <stddef.h>
        #include "vislam_ba.h"
        int main(){printf("%s\\n", %s);return 0;}''') % (" ".join(["%zu"] * n), pr)
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    got = list(map(int, subprocess.check_output([exe]).split()))
    want = [x for name, fields in STRUCTS for x in [C.sizeof(getattr(abi, name))] + [getattr(getattr(abi, name), f).offset for f in fields]]
    assert got == want
    for name, fields in STRUCTS:
        assert [f for f, _ in getattr(abi, name)._fields_] == fields


def test_symbol_in_both_flavours():
    assert "vba_search_by_sim3" in backend.EXPORTS
    for hooks in (False, True):
        lib = backend.load_library(hooks)
        assert lib.vba_search_by_sim3.argtypes == [C.c_void_p, C.c_int32, C.POINTER(C.POINTER(abi.vba_search_sim3_problem)),
                                                   C.POINTER(C.POINTER(abi.vba_search_sim3_result))]
        assert lib.vba_search_by_sim3.restype == C.c_int


def test_no_answer_without_a_handle():
    """a NULL handle is refused with -1 and nothing is written; where no device exists no handle can be made at all"""
    lib = backend.load_library()
    p = synth.sim3_search_scene(1, n_keys1=40, n_keys2=30, n_common=20)
    s, buf = p.as_struct(), abi.SearchSim3ResultBuf(p)
    pp = (C.POINTER(abi.vba_search_sim3_problem) * 1)(C.pointer(s))
    rr = (C.POINTER(abi.vba_search_sim3_result) * 1)(C.pointer(buf.s))
    assert lib.vba_search_by_sim3(None, 1, pp, rr) == -1
    assert buf.untouched()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            backend.LocalBA(0).search_by_sim3([p])


def test_python_views():
    p = synth.sim3_search_scene(3, n_keys1=90, n_keys2=70, n_common=50, n_levels=(8, 6), grid=((64, 48), (32, 24)))
    a, b = p.kf1, p.kf2
    assert (a.n_keys, b.n_keys, a.n_levels, b.n_levels) == (90, 70, 8, 6) and a.pt_desc.shape == (90, 32) and b.cell_begin.shape == (32 * 24 + 1,)
    assert (p.th, p.th_high) == (7.5, 100) and p.s12 == float(np.float32(1.1))
    s = p.as_struct()
    assert (s.kf1.n_keys, s.kf2.n_keys, s.kf2.n_levels, s.kf2.grid_cols, s.kf2.grid_rows, s.th_high) == (90, 70, 6, 32, 24, 100)
    assert s.kf2.Rcw[5] == b.Rcw[1, 2] and s.K[3] == p.K[3] and s.kf1.bounds[1] == 640.0 and s.kf2.pos[4] == b.pos[1, 1] and s.R12[7] == p.R12[2, 1]
    assert s.kf1.cell_begin[64 * 48] == len(a.cell_feat) and s.kf2.has_pt[3] == b.has_pt[3] and s.kf1.matched[5] == a.matched[5]
    q = p.copy(th=5.0, kf2=dict(matched=np.ones(70)))
    assert q.th == 5.0 and q.kf2.matched.dtype == np.uint8 and q.kf2.matched.all() and p.th == 7.5 and not p.kf2.matched.all() and q.kf1 is p.kf1
    assert set(p.truth) == {"kind", "key1", "key2"} and len(p.truth["key1"]) == 50
