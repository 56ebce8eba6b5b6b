"""CPU-side checks of the vba_sim3_ransac boundary: the ctypes structs against what gcc makes of include/vislam_ba.h, the symbol in
both library flavours, and no answer without a handle (the library has no CPU path)."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from mc_slam_amd import abi, backend, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_FIELDS = ["n_pairs", "fix_scale", "p1c", "p2c", "max_err1", "max_err2", "K1", "K2", "min_inliers", "n_hyp", "sample", "best_inliers", "best_S12"]
R_FIELDS = ["status", "hit", "its_done", "best_hyp", "n_inliers", "S12", "inlier", "hyp_inliers"]


def test_struct_layout_matches_header(tmp_path):
    pr = ", ".join(["sizeof(vba_sim3_ransac_problem)"] + ["offsetof(vba_sim3_ransac_problem, %s)" % f for f in P_FIELDS] +
                   ["sizeof(vba_sim3_ransac_result)"] + ["offsetof(vba_sim3_ransac_result, %s)" % f for f in R_FIELDS])
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
    want = ([C.sizeof(abi.vba_sim3_ransac_problem)] + [getattr(abi.vba_sim3_ransac_problem, f).offset for f in P_FIELDS] +
            [C.sizeof(abi.vba_sim3_ransac_result)] + [getattr(abi.vba_sim3_ransac_result, f).offset for f in R_FIELDS])
    assert got == want


def test_symbol_in_both_flavours():
    assert "vba_sim3_ransac" in backend.EXPORTS
    for hooks in (False, True):
        lib = backend.load_library(hooks)
        assert lib.vba_sim3_ransac.argtypes[2] == C.POINTER(C.POINTER(abi.vba_sim3_ransac_problem))


def test_no_answer_without_a_handle():
    """a NULL handle is refused with -1 and nothing is written; where no device exists no handle can be made at all"""
    lib = backend.load_library()
    p = synth.make_sim3_ransac(1, 25, 0, 0.1)
    p = p.copy(sample=synth.draw_triples(2, 25, 5))
    s, buf = p.as_struct(), abi.Sim3RansacResultBuf(p)
    buf.s.hit = 12345
    pp = (C.POINTER(abi.vba_sim3_ransac_problem) * 1)(C.pointer(s))
    rr = (C.POINTER(abi.vba_sim3_ransac_result) * 1)(C.pointer(buf.s))
    assert lib.vba_sim3_ransac(None, 1, pp, rr) == -1
    assert buf.s.hit == 12345 and (buf.c == -1).all() and s.best_inliers == 0
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            backend.LocalBA(0).sim3_ransac([p])


def test_python_views():
    p = synth.make_sim3_ransac(3, 40, 1, 0.25, same_K=True)
    assert p.n_pairs == 40 and p.n_hyp == 0 and p.fix_scale == 1 and np.array_equal(p.K1, p.K2)
    assert set(np.round(p.max_err1 / 9.210, 6)) <= {1.0, 1.44, 2.0736, 2.985984}
    t = synth.draw_triples(5, 40, 100)
    assert t.shape == (100, 3) and t.dtype == np.int32 and t.min() >= 0 and t.max() < 40
    assert all(len(set(r)) == 3 for r in t.tolist())
    assert np.array_equal(t, synth.draw_triples(5, 40, 100))
    q = p.copy(sample=t, min_inliers=9)
    s = q.as_struct()
    assert (s.n_pairs, s.n_hyp, s.min_inliers, s.best_inliers) == (40, 100, 9, 0) and p.n_hyp == 0
    # the noise is on the 3D points: no pair maps exactly, the clean ones map to about a percent of the depth
    S = p.truth["S12"]
    from mc_slam_amd.synth import quat_to_rot
    y = S[7] * p.p2c @ quat_to_rot(S[3:7]).T + S[:3]
    e = np.linalg.norm(y - p.p1c, axis=1)
    clean = ~p.truth["is_outlier"]
    assert (e[clean] > 0).all() and np.median(e[clean] / p.p1c[clean, 2]) < 0.03 and np.median(e[~clean]) > 0.5
