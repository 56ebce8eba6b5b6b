"""CPU-side checks of the vba_search_by_projection_kf boundary: the ctypes structs against what gcc makes of include/vislam_ba.h, the
symbol in both library flavours, and no answer without a handle (the library has no CPU path)."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from mc_slam_amd import abi, backend, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_FIELDS = ["mode", "check_orientation", "Rcw", "tcw", "Ow", "K", "bounds", "n_keys", "n_levels", "desc", "uv", "oct", "angle", "scale",
            "log_scale_factor", "grid_cols", "grid_rows", "grid_inv_w", "grid_inv_h", "cell_begin", "cell_feat", "occupied", "n_q", "th_dist", "th",
            "cos_view", "q_pos", "q_desc", "q_skip", "q_normal", "q_dist_min", "q_dist_max", "q_pred_max", "q_angle"]
R_FIELDS = ["status", "n_matches", "n_before_filter", "hist", "ind", "rounds", "best_idx", "best_dist", "level", "uv", "bin", "state", "key_match"]


def test_struct_layout_matches_header(tmp_path):
    pr = ", ".join(["sizeof(vba_search_proj_kf_problem)"] + ["offsetof(vba_search_proj_kf_problem, %s)" % f for f in P_FIELDS] +
                   ["sizeof(vba_search_proj_kf_result)"] + ["offsetof(vba_search_proj_kf_result, %s)" % f for f in R_FIELDS] +
                   ["(size_t)VBA_SEARCH_PROJ_KF_LOOP", "(size_t)VBA_SEARCH_PROJ_KF_RELOC", "(size_t)VBA_SEARCH_PROJ_KF_MAX_KEYS"])
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
    want = ([C.sizeof(abi.vba_search_proj_kf_problem)] + [getattr(abi.vba_search_proj_kf_problem, f).offset for f in P_FIELDS] +
            [C.sizeof(abi.vba_search_proj_kf_result)] + [getattr(abi.vba_search_proj_kf_result, f).offset for f in R_FIELDS] +
            [abi.SEARCH_PROJ_KF_LOOP, abi.SEARCH_PROJ_KF_RELOC, abi.SEARCH_PROJ_KF_MAX_KEYS])
    assert got == want
    assert [f for f, _ in abi.vba_search_proj_kf_problem._fields_] == P_FIELDS and [f for f, _ in abi.vba_search_proj_kf_result._fields_] == R_FIELDS


def test_symbol_in_both_flavours():
    assert "vba_search_by_projection_kf" in backend.EXPORTS
    for hooks in (False, True):
        lib = backend.load_library(hooks)
        assert lib.vba_search_by_projection_kf.argtypes[2] == C.POINTER(C.POINTER(abi.vba_search_proj_kf_problem))
        out = subprocess.check_output(["nm", "-D", "--defined-only", backend.HOOKS_LIB_PATH if hooks else backend.LIB_PATH], text=True)
        assert any(l.split()[-1] == "vba_search_by_projection_kf" for l in out.splitlines() if l.split())


@pytest.mark.parametrize("mode", [abi.SEARCH_PROJ_KF_LOOP, abi.SEARCH_PROJ_KF_RELOC])
def test_no_answer_without_a_handle(mode):
    """a NULL handle is refused with -1 and nothing is written; where no device exists no handle can be made at all"""
    lib = backend.load_library()
    p = synth.search_proj_kf_scene(1, mode, n_keys=40, n_q=20)
    s, buf = p.as_struct(), abi.SearchProjKfResultBuf(p)
    pp = (C.POINTER(abi.vba_search_proj_kf_problem) * 1)(C.pointer(s))
    rr = (C.POINTER(abi.vba_search_proj_kf_result) * 1)(C.pointer(buf.s))
    assert lib.vba_search_by_projection_kf(None, 1, pp, rr) == -1
    assert buf.untouched()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            backend.LocalBA(0).search_by_projection_kf([p])


def test_python_views():
    p = synth.search_proj_kf_scene(3, abi.SEARCH_PROJ_KF_LOOP, n_keys=90, n_q=50)
    assert (p.n_keys, p.n_q, p.n_levels) == (90, 50, 8) and p.desc.shape == (90, 32) and p.q_desc.shape == (50, 32) and p.cell_begin.shape == (64 * 48 + 1,)
    assert (p.th, p.th_dist, p.cos_view, p.reloc) == (10.0, 50, 0.5, False) and p.angle is None and p.q_angle is None
    s = p.as_struct()
    assert (s.mode, s.n_keys, s.n_q, s.n_levels, s.grid_cols, s.grid_rows, s.th_dist) == (0, 90, 50, 8, 64, 48, 50)
    assert s.Rcw[5] == p.Rcw[1, 2] and s.K[3] == p.K[3] and s.q_pos[4] == p.q_pos[1, 1] and s.q_normal[5] == p.q_normal[1, 2] and not s.q_angle and not s.angle
    m = synth.search_proj_kf_scene(3, abi.SEARCH_PROJ_KF_RELOC, n_keys=90, n_q=50)
    assert (m.th, m.th_dist, m.reloc, m.check_orientation) == (10.0, 100, True, True) and m.q_normal is None and m.angle.dtype == np.float32
    t = m.as_struct()
    assert t.mode == 1 and t.check_orientation == 1 and not t.q_normal and t.q_angle[7] == m.q_angle[7] and t.angle[3] == m.angle[3] and t.Ow[2] == m.Ow[2]
    q = m.copy(th=3.0, th_dist=64, q_skip=np.ones(50))
    assert (q.th, q.th_dist) == (3.0, 64) and q.q_skip.dtype == np.uint8 and m.th == 10.0 and not m.q_skip.all()
    b = abi.SearchProjKfResultBuf(m)
    assert b.untouched() and b.get().key_match.shape == (90,) and b.get().state.shape == (50,)
