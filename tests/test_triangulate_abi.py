"""CPU-side checks of the vba_triangulate boundary: the ctypes structs against what gcc makes of include/vislam_ba.h, the symbol in
both library flavours, and no answer without a handle (the library has no CPU path)."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from mc_slam_amd import abi, backend, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_FIELDS = ["Rcw1", "tcw1", "Ow1", "K1", "Rcw2", "tcw2", "Ow2", "K2", "n_levels1", "n_levels2", "level_sigma2_1", "scale_1", "level_sigma2_2",
            "scale_2", "ratio_factor", "cos_max", "chi2_th", "n_matches", "uv1", "uv2", "oct1", "oct2"]
R_FIELDS = ["status", "n_accepted", "x3d", "reason"]


def test_struct_layout_matches_header(tmp_path):
    pr = ", ".join(["sizeof(vba_triangulate_problem)"] + ["offsetof(vba_triangulate_problem, %s)" % f for f in P_FIELDS] +
                   ["sizeof(vba_triangulate_result)"] + ["offsetof(vba_triangulate_result, %s)" % f for f in R_FIELDS])
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
    want = ([C.sizeof(abi.vba_triangulate_problem)] + [getattr(abi.vba_triangulate_problem, f).offset for f in P_FIELDS] +
            [C.sizeof(abi.vba_triangulate_result)] + [getattr(abi.vba_triangulate_result, f).offset for f in R_FIELDS])
    assert got == want
    assert [f for f, _ in abi.vba_triangulate_problem._fields_] == P_FIELDS and [f for f, _ in abi.vba_triangulate_result._fields_] == R_FIELDS


def test_symbol_in_both_flavours():
    assert "vba_triangulate" in backend.EXPORTS
    for hooks in (False, True):
        lib = backend.load_library(hooks)
        assert lib.vba_triangulate.argtypes[2] == C.POINTER(C.POINTER(abi.vba_triangulate_problem))


def test_no_answer_without_a_handle():
    """a NULL handle is refused with -1 and nothing is written; where no device exists no handle can be made at all"""
    lib = backend.load_library()
    p = synth.make_triangulate(1, 25)
    s, buf = p.as_struct(), abi.TriangulateResultBuf(p)
    buf.s.n_accepted = 12345
    pp = (C.POINTER(abi.vba_triangulate_problem) * 1)(C.pointer(s))
    rr = (C.POINTER(abi.vba_triangulate_result) * 1)(C.pointer(buf.s))
    assert lib.vba_triangulate(None, 1, pp, rr) == -1
    assert buf.s.n_accepted == 12345 and (buf.r == 255).all() and not buf.x.any()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            backend.LocalBA(0).triangulate([p])


def test_python_views():
    p = synth.make_triangulate(3, 40, "forward")
    assert p.n_matches == 40 and p.n_levels1 == p.n_levels2 == 8 and p.oct1.dtype == np.uint8
    for a in (p.Rcw1, p.tcw1, p.Ow1, p.K1, p.Rcw2, p.tcw2, p.Ow2, p.uv1, p.uv2, p.scale_1, p.level_sigma2_1):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))          # everything went through float32
    assert np.array_equal(p.level_sigma2_1, (p.scale_1.astype(np.float32) ** 2).astype(np.float64))
    assert p.ratio_factor == float(np.float32(1.5) * np.float32(1.2)) and (p.cos_max, p.chi2_th) == (0.9998, 5.991)
    b = np.linalg.norm(p.Ow2 - p.Ow1)
    assert 0.1 <= b <= 0.5 + 1e-6
    assert abs(np.linalg.norm(synth.make_triangulate(3, 4, "far").Ow1) - 50.0) < 1e-3
    s = p.as_struct()
    assert (s.n_matches, s.n_levels1, s.n_levels2) == (40, 8, 8) and s.Rcw2[5] == p.Rcw2[1, 2] and s.K1[0] == p.K1[0]
    q = p.copy(uv1=p.uv1[:7], uv2=p.uv2[:7], oct1=p.oct1[:7], oct2=p.oct2[:7])
    assert q.n_matches == 7 and p.n_matches == 40
    assert set(np.unique(p.truth["kind"])) <= set(range(len(synth.TRI_KINDS)))
