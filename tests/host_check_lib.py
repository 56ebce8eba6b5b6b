"""What the tests of the host halves (tests/test_host_*.py) share: building a sanitizer harness tests/host_*_check.cpp (stand-alone,
g++ -fsanitize=address,undefined, CPU only), running it, reading its "ok key value ..." lines, and restating arena offsets and
checksums from the sizes alone."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path_factory, name, pthread=False):
    """tests/<name>.cpp under ASan + UBSan: the path of the program"""
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + (["-pthread"] if pthread else []) +
                          ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe])
    return exe


def run(checker, args, n_lines=None, env=None, timeout=300):
    """the harness on args with leak detection on: its output lines, after asserting that no sanitizer spoke (n_lines: and that
    it printed that many)"""
    r = subprocess.run([checker] + list(args), capture_output=True, text=True, env=dict(os.environ if env is None else env, ASAN_OPTIONS="detect_leaks=1"),
                       timeout=timeout)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert n_lines is None or len(lines) == n_lines, lines
    return lines


def fields(line, floats=()):
    """the "ok key value ..." line of a harness as a dict of ints (floats: the keys that are not)"""
    assert line.startswith("ok "), line
    t = line.split()
    return {k: (float(v) if k in floats else int(v)) for k, v in zip(t[1::2], t[2::2])}


def up(b):
    """bytes of an arena region of b bytes: the next region starts at the next multiple of 256"""
    return (b + 255) // 256 * 256


def checksum(*arrays):
    """sum of (2 i + 1) * word i over the 64-bit words of the arrays' bytes (padded with zeros to whole words), mod 2^64"""
    b = b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)
    w = np.frombuffer(b + b"\0" * (-len(b) % 8), dtype="<u8")
    with np.errstate(over="ignore"):
        return int((w * (2 * np.arange(len(w), dtype=np.uint64) + 1)).sum(dtype=np.uint64))


def assert_bound(f, pairs):
    """every pointer of the kernel's argument sits at the offset of the arena region it is meant to read: pairs of (Batch field,
    region) names of a harness line f"""
    for field, region in pairs:
        assert f["bind_" + field] == f[region], (field, region)
