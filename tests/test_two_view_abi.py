"""CPU-side checks of the vba_two_view_init boundary: the ctypes structs against what gcc makes of include/vislam_ba.h, the symbol
in both library flavours, and no answer without a handle (the library has no CPU path)."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from mc_slam_amd import abi, backend, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_FIELDS = ["n_keys1", "n_keys2", "uv1", "uv2", "n_matches", "n_hyp", "match", "sets", "K", "sigma", "min_parallax", "min_triangulated", "pad"]
R_FIELDS = ["status", "ok", "model", "reason", "best_hyp_h", "best_hyp_f", "n_inliers_h", "n_inliers_f", "n_rt", "best_rt", "rt_good", "score_h",
            "score_f", "rh", "H21", "F21", "rt_parallax", "R21", "t21", "inlier_h", "inlier_f", "x3d", "triangulated", "hyp_score_h", "hyp_score_f"]


def test_struct_layout_matches_header(tmp_path):
    pr = ", ".join(["sizeof(vba_two_view_problem)"] + ["offsetof(vba_two_view_problem, %s)" % f for f in P_FIELDS] +
                   ["sizeof(vba_two_view_result)"] + ["offsetof(vba_two_view_result, %s)" % f for f in R_FIELDS])
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
    want = ([C.sizeof(abi.vba_two_view_problem)] + [getattr(abi.vba_two_view_problem, f).offset for f in P_FIELDS] +
            [C.sizeof(abi.vba_two_view_result)] + [getattr(abi.vba_two_view_result, f).offset for f in R_FIELDS])
    assert got == want
    assert [f for f, _ in abi.vba_two_view_problem._fields_] == P_FIELDS and [f for f, _ in abi.vba_two_view_result._fields_] == R_FIELDS


def test_symbol_in_both_flavours():
    assert "vba_two_view_init" in backend.EXPORTS
    for hooks in (False, True):
        lib = backend.load_library(hooks)
        assert lib.vba_two_view_init.argtypes[2] == C.POINTER(C.POINTER(abi.vba_two_view_problem))


def test_no_answer_without_a_handle():
    """a NULL handle is refused with -1 and nothing is written; where no device exists no handle can be made at all"""
    lib = backend.load_library()
    p = synth.make_two_view(1, 25, 4)
    s, buf = p.as_struct(), abi.TwoViewResultBuf(p, fill=9)
    buf.s.ok = 12345
    pp = (C.POINTER(abi.vba_two_view_problem) * 1)(C.pointer(s))
    rr = (C.POINTER(abi.vba_two_view_result) * 1)(C.pointer(buf.s))
    assert lib.vba_two_view_init(None, 1, pp, rr) == -1
    assert buf.s.ok == 12345 and (buf.ih == 9).all() and (buf.tr == 9).all() and (buf.x == 9.0).all() and (buf.sh == 9.0).all()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            backend.LocalBA(0).two_view_init([p])


def test_python_views():
    p = synth.make_two_view(3, 40, 6, "plane")
    assert (p.n_matches, p.n_hyp, p.n_keys1, p.n_keys2) == (40, 6, 77, 93) and p.match.dtype == np.int32 and p.sets.dtype == np.int32
    for a in (p.uv1, p.uv2, p.K):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))          # everything went through float32
    assert len(set(p.match[:, 0])) == 40 and (np.diff(p.match[:, 0]) > 0).all()    # mvMatches12 ascends in the first index
    assert all(len(set(s)) == 8 for s in p.sets.tolist()) and p.sets.min() >= 0 and p.sets.max() < 40
    assert (p.sigma, p.min_parallax, p.min_triangulated) == (1.0, 1.0, 50)
    s = p.as_struct()
    assert (s.n_keys1, s.n_keys2, s.n_matches, s.n_hyp, s.min_triangulated) == (77, 93, 40, 6, 50) and s.K[1] == p.K[1] and s.match[3] == p.match[1, 1]
    q = p.copy(match=p.match[:9])
    assert q.n_matches == 9 and p.n_matches == 40
    b = abi.TwoViewResultBuf(p, want_scores=False)
    assert not b.s.hyp_score_h and b.get().hyp_score_f is None and b.get().x3d.shape == (77, 3)
