"""CPU-side checks of the asynchronous batch interface (vba_batch_submit / poll / wait): the header declares it, the Python
binding lists it, the shipped library exports it, and its test hook exists only in the hooks flavour."""
import os
import re
import subprocess

from mc_slam_amd import backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASYNC = ["vba_batch_set_depth", "vba_batch_submit", "vba_batch_submit_b", "vba_batch_poll", "vba_batch_wait"]


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return set(l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("vba_"))


def test_header_declares_the_async_entries_and_exports_lists_them():
    txt = open(os.path.join(ROOT, "include", "vislam_ba.h")).read()
    for n in ASYNC:
        assert re.search(r"^\s*int\s+%s\s*\(" % n, txt, flags=re.M), n
        assert n in backend.EXPORTS, n


def test_shipped_library_exports_the_async_entries():
    got = _exported(backend.LIB_PATH)
    assert set(ASYNC) <= got, sorted(set(ASYNC) - got)
    lib = backend.load_library()
    for n in ASYNC:
        assert getattr(lib, n) is not None


def test_async_hold_hook_only_in_the_hooks_flavour():
    assert "vba_debug_async_hold" not in _exported(backend.LIB_PATH)
    assert "vba_debug_async_hold" in _exported(backend.HOOKS_LIB_PATH)
