"""CPU-side checks of the Sim3 entry point: the header declares it, both library flavours export it, the ctypes mirrors have the
C compiler's struct sizes, and without a device the call path fails loudly instead of falling back."""
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
    return set(l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("vba_"))


def test_header_declares_vba_sim3_optimize_and_exports_lists_it():
    txt = open(os.path.join(ROOT, "include", "vislam_ba.h")).read()
    assert re.search(r"^\s*int\s+vba_sim3_optimize\s*\(", txt, flags=re.M)
    assert "typedef struct vba_sim3_problem" in txt and "typedef struct vba_sim3_result" in txt
    assert "vba_sim3_optimize" in backend.EXPORTS


def test_both_library_flavours_export_it():
    assert "vba_sim3_optimize" in _exported(backend.LIB_PATH)
    assert "vba_sim3_optimize" in _exported(backend.HOOKS_LIB_PATH)
    assert backend.load_library().vba_sim3_optimize is not None


def test_struct_sizes_match_the_c_compiler():
    src = textwrap.dedent('''
        #include <stdio.h>
        #include <stddef.h>
        #include "vislam_ba.h"
        int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(vba_sim3_problem), sizeof(vba_sim3_result), offsetof(vba_sim3_problem, S12),
                          offsetof(vba_sim3_problem, min_inliers), offsetof(vba_sim3_result, outlier));return 0;}''')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c"); exe = os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = tuple(map(int, subprocess.check_output([exe]).split()))
    assert got == (C.sizeof(abi.vba_sim3_problem), C.sizeof(abi.vba_sim3_result), abi.vba_sim3_problem.S12.offset,
                   abi.vba_sim3_problem.min_inliers.offset, abi.vba_sim3_result.outlier.offset)


def test_no_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    assert hasattr(backend.LocalBA, "sim3_optimize")
    with pytest.raises(RuntimeError, match="no usable HIP device"):
        backend.LocalBA(0).sim3_optimize([])
