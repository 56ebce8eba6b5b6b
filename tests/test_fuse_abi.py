"""CPU-side checks of the vba_fuse boundary: the ctypes structs against what gcc makes of include/vislam_ba.h, the symbol in both
library flavours, and no answer without a handle (the library has no CPU path)."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

from mc_slam_amd import abi, backend, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_FIELDS = ["Rcw", "tcw", "Ow", "K", "bounds", "n_keys", "n_levels", "desc", "uv", "oct", "scale", "inv_level_sigma2", "log_scale_factor", "grid_cols",
            "grid_rows", "grid_inv_w", "grid_inv_h", "cell_begin", "cell_feat", "n_pt", "th_low", "pos", "normal", "dist_min", "dist_max", "pred_max",
            "pt_desc", "skip", "th", "cos_view", "check_reproj", "chi2_reproj"]
R_FIELDS = ["status", "n_found", "best_idx", "best_dist", "level", "uv", "state"]


def test_struct_layout_matches_header(tmp_path):
    pr = ", ".join(["sizeof(vba_fuse_problem)"] + ["offsetof(vba_fuse_problem, %s)" % f for f in P_FIELDS] +
                   ["sizeof(vba_fuse_result)"] + ["offsetof(vba_fuse_result, %s)" % f for f in R_FIELDS])
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
    want = ([C.sizeof(abi.vba_fuse_problem)] + [getattr(abi.vba_fuse_problem, f).offset for f in P_FIELDS] +
            [C.sizeof(abi.vba_fuse_result)] + [getattr(abi.vba_fuse_result, f).offset for f in R_FIELDS])
    assert got == want
    assert [f for f, _ in abi.vba_fuse_problem._fields_] == P_FIELDS and [f for f, _ in abi.vba_fuse_result._fields_] == R_FIELDS


def test_symbol_in_both_flavours():
    assert "vba_fuse" in backend.EXPORTS
    for hooks in (False, True):
        lib = backend.load_library(hooks)
        assert lib.vba_fuse.argtypes[2] == C.POINTER(C.POINTER(abi.vba_fuse_problem))


def test_no_answer_without_a_handle():
    """a NULL handle is refused with -1 and nothing is written; where no device exists no handle can be made at all"""
    lib = backend.load_library()
    p = synth.fuse_scene(1, n_keys=40, n_pt=20)
    s, buf = p.as_struct(), abi.FuseResultBuf(p)
    pp = (C.POINTER(abi.vba_fuse_problem) * 1)(C.pointer(s))
    rr = (C.POINTER(abi.vba_fuse_result) * 1)(C.pointer(buf.s))
    assert lib.vba_fuse(None, 1, pp, rr) == -1
    assert buf.s.n_found == -7 and (buf.st == 255).all() and (buf.bi == -7).all() and (buf.uv == -7.0).all()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            backend.LocalBA(0).fuse([p])


def test_python_views():
    p = synth.fuse_scene(3, n_keys=90, n_pt=50)
    assert (p.n_keys, p.n_pt, p.n_levels) == (90, 50, 8) and p.desc.shape == (90, 32) and p.pt_desc.shape == (50, 32) and p.cell_begin.shape == (64 * 48 + 1,)
    assert (p.th, p.th_low, p.cos_view, p.chi2_reproj, p.check_reproj) == (3.0, 50, 0.5, 5.99, True)
    s = p.as_struct()
    assert (s.n_keys, s.n_pt, s.n_levels, s.grid_cols, s.grid_rows, s.th_low, s.check_reproj) == (90, 50, 8, 64, 48, 50, 1)
    assert s.Rcw[5] == p.Rcw[1, 2] and s.K[3] == p.K[3] and s.bounds[1] == 640.0 and s.pos[4] == p.pos[1, 1] and s.cell_begin[64 * 48] == len(p.cell_feat)
    q = p.copy(th=5.0, skip=np.ones(50))
    assert q.th == 5.0 and q.skip.dtype == np.uint8 and p.th == 3.0 and not p.skip.all()
    # the grid: Frame::AssignFeaturesToGrid puts keypoint i into cell round(x / 10), round(y / 10) unless that is outside the grid
    b, f = abi.grid_csr([[4.9, 5.1], [75.1, 3.0], [14.0, 26.0], [5.0, 14.9], [3.0, 55.0]], (0, 80, 0, 60), 8, 6, 0.1, 0.1)
    assert f.tolist() == [0, 3, 2] and np.nonzero(np.diff(b))[0].tolist() == [1, 6 + 1, 6 + 3] and b[-1] == 3    # cells (0, 1) (1, 1) (1, 3); 1 and 4 round out of the grid
