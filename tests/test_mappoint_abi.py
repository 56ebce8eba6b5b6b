"""CPU-side checks of the vba_mappoint_update boundary: the ctypes structs against what gcc makes of include/vislam_ba.h, the symbol in
both library flavours, and no answer without a handle (the library has no CPU path)."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

import mappoint_cases as cases
from mc_slam_amd import abi, backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_FIELDS = ["n_kf", "kf_center", "kf_bad", "n_pt", "what", "pos", "ref_kf", "ref_scale", "ref_top_scale", "obs_begin", "obs_kf", "obs_desc"]
R_FIELDS = ["status", "n_desc_done", "n_normal_done", "best_obs", "best_median", "n_desc", "desc", "normal", "dist_max", "dist_min", "desc_state",
            "normal_state"]


def test_struct_layout_matches_header(tmp_path):
    pr = ", ".join(["sizeof(vba_mappoint_problem)"] + ["offsetof(vba_mappoint_problem, %s)" % f for f in P_FIELDS] +
                   ["sizeof(vba_mappoint_result)"] + ["offsetof(vba_mappoint_result, %s)" % f for f in R_FIELDS] +
                   ["(size_t)VBA_MAPPOINT_MAX_OBS", "(size_t)VBA_MAPPOINT_DESC", "(size_t)VBA_MAPPOINT_NORMAL"])
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
    want = ([C.sizeof(abi.vba_mappoint_problem)] + [getattr(abi.vba_mappoint_problem, f).offset for f in P_FIELDS] +
            [C.sizeof(abi.vba_mappoint_result)] + [getattr(abi.vba_mappoint_result, f).offset for f in R_FIELDS] +
            [abi.MAPPOINT_MAX_OBS, abi.MAPPOINT_DESC, abi.MAPPOINT_NORMAL])
    assert got == want
    assert [f for f, _ in abi.vba_mappoint_problem._fields_] == P_FIELDS and [f for f, _ in abi.vba_mappoint_result._fields_] == R_FIELDS


def test_symbol_in_both_flavours():
    assert "vba_mappoint_update" in backend.EXPORTS
    for hooks in (False, True):
        lib = backend.load_library(hooks)
        assert lib.vba_mappoint_update.argtypes[2] == C.POINTER(C.POINTER(abi.vba_mappoint_problem))
        out = subprocess.check_output(["nm", "-D", "--defined-only", backend.HOOKS_LIB_PATH if hooks else backend.LIB_PATH], text=True)
        assert any(l.split()[-1] == "vba_mappoint_update" for l in out.splitlines() if l.split())


def test_no_answer_without_a_handle():
    """a NULL handle is refused with -1 and nothing is written; where no device exists no handle can be made at all"""
    lib = backend.load_library()
    p = cases.cases()["bad_kf"]
    s, buf = p.as_struct(), abi.MapPointResultBuf(p)
    pp = (C.POINTER(abi.vba_mappoint_problem) * 1)(C.pointer(s))
    rr = (C.POINTER(abi.vba_mappoint_result) * 1)(C.pointer(buf.s))
    assert lib.vba_mappoint_update(None, 1, pp, rr) == -1
    assert buf.untouched()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            backend.LocalBA(0).mappoint_update([p])


def test_python_views():
    p = cases.cases()["bad_kf"]
    assert (p.n_kf, p.n_pt, p.n_obs) == (10, 5, 25) and p.obs_desc.shape == (25, 32) and p.kf_center.shape == (10, 3) and p.what.dtype == np.uint8
    assert p.obs_begin.dtype == np.int32 and p.obs_kf.dtype == np.int32 and p.pos.dtype == np.float64 and p.kf_bad.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0]
    s = p.as_struct()
    assert (s.n_kf, s.n_pt) == (10, 5) and s.obs_begin[5] == 25 and s.obs_kf[9] == 1 and s.pos[4] == p.pos[1, 1] and s.kf_center[29] == p.kf_center[9, 2]
    assert s.ref_scale[2] == p.ref_scale[2] and s.obs_desc[33] == p.obs_desc[1, 1] and s.what[0] == 3
    q = p.copy(what=[1, 1, 1, 1, 1], pos=None, ref_kf=None, ref_scale=None, ref_top_scale=None)
    t = q.as_struct()
    assert q.what.dtype == np.uint8 and p.what[0] == 3 and not t.pos and not t.ref_kf and not t.ref_scale and not t.ref_top_scale and bool(t.obs_desc)
    assert not p.copy(obs_desc=None).as_struct().obs_desc
    b = abi.MapPointResultBuf(p)
    g = b.get()
    assert b.untouched() and g.best_obs.shape == (5,) and g.desc.shape == (5, 32) and g.normal.shape == (5, 3) and g.desc_state.tolist() == [255] * 5
    assert (g.status, g.best_median[0], g.normal[0, 0]) == (-7, -7, -7.0)
    assert abi.MapPointResultBuf(cases.cases()["n_pt_0"]).get().best_obs.shape == (0,)
