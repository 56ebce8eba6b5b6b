"""CPU-side checks of the pose-graph entry point: the header declares it, both library flavours export it (the hook only in the
hooks flavour), the ctypes mirrors have the C compiler's struct layout, and without a device the call path fails loudly."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import textwrap

import pytest

from mc_slam_amd import abi, backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return set(l.split()[-1] for l in out.splitlines() if l.split())


def test_header_declares_vba_posegraph_optimize_and_exports_lists_it():
    txt = open(os.path.join(ROOT, "include", "vislam_ba.h")).read()
    assert re.search(r"^\s*int\s+vba_posegraph_optimize\s*\(", txt, flags=re.M)
    assert "typedef struct vba_posegraph_problem" in txt and "typedef struct vba_posegraph_result" in txt
    assert "vba_posegraph_optimize" in backend.EXPORTS
    assert "src/Optimizer.cpp:4243-4552" in txt


def test_both_library_flavours_export_it():
    plain, hooks = _exported(backend.LIB_PATH), _exported(backend.HOOKS_LIB_PATH)
    assert "vba_posegraph_optimize" in plain and "vba_posegraph_optimize" in hooks
    assert "vba_debug_posegraph_system" in hooks and "vba_debug_posegraph_system" not in plain
    assert "posegraph_run" not in plain and "posegraph_run" not in hooks          # the worker behind both stays internal
    assert backend.load_library().vba_posegraph_optimize is not None


def test_struct_layout_matches_the_c_compiler():
    names_p = ["n_vertices", "n_edges", "fix_scale", "its", "lambda_init", "S", "fixed", "edge_i", "edge_j", "edge_S", "n_pt", "pt", "pt_ref"]
    names_r = ["status", "its_done", "lm_trials", "stop", "chi2_initial", "chi2_final", "lambda_final"]
    body = "".join('printf("%%zu ", offsetof(vba_posegraph_problem, %s));' % n for n in names_p)
    body += "".join('printf("%%zu ", offsetof(vba_posegraph_result, %s));' % n for n in names_r)
    src = textwrap.dedent('''
        #include <stdio.h>
        #include <stddef.h>
        #include "vislam_ba.h"
        int main(){printf("%%zu %%zu ", sizeof(vba_posegraph_problem), sizeof(vba_posegraph_result));%s printf("\\n");return 0;}''') % body
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c"); exe = os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = tuple(map(int, subprocess.check_output([exe]).split()))
    want = (C.sizeof(abi.vba_posegraph_problem), C.sizeof(abi.vba_posegraph_result))
    want += tuple(getattr(abi.vba_posegraph_problem, n).offset for n in names_p)
    want += tuple(getattr(abi.vba_posegraph_result, n).offset for n in names_r)
    assert got == want


def test_no_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    assert hasattr(backend.LocalBA, "posegraph_optimize")
    with pytest.raises(RuntimeError, match="no usable HIP device"):
        backend.LocalBA(0).posegraph_optimize([])
