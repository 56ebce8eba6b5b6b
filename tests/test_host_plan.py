"""The policy of a batch (mc_slam_amd/csrc/vba_host_plan.h: knobs, overrides, plan_upload / plan_run, group_bounds, chunk_bounds)
under AddressSanitizer + UBSan (CPU only).  The harness (tests/host_plan_check.cpp) runs one command per line of a file against a
fake environment; every expected value below is restated from the documented thresholds, none is printed by the code under test."""
import os
import re
import subprocess

import pytest

import plan_cases as pc
import host_check_lib as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mc_slam_amd", "csrc")
SIZES = [1, 3, 4, 7, 8, 9, 15, 16, 63, 64, 65, 255, 256, 300]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return hc.build(tmp_path_factory, "host_plan_check")


def _run(checker, tmp_path, lines):
    path = str(tmp_path / "cases.txt")
    open(path, "w").write("".join(l + "\n" for l in lines))
    env = {k: v for k, v in os.environ.items() if not k.startswith("VBA_")}      # (the harness reads its fake environment only)
    r = subprocess.run([checker, path], capture_output=True, text=True, env=dict(env, ASAN_OPTIONS="detect_leaks=1"), timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines), out
    return out


def _plans(checker, tmp_path, lines):
    return [dict(zip(pc.FIELDS, map(int, l.split()))) for l in _run(checker, tmp_path, ["plan " + l for l in lines])]


# ------------------------------------------------------------------------------------------------------------ plan table
def test_plan_table_under_an_empty_environment(checker, tmp_path):
    cases = [(n, v, a, s) for n in SIZES for v in (pc.PRV_IDP, pc.PRV_XYZ, pc.SE3_XYZ) for a in (pc.GN, pc.LM) for s in (0, 1)]
    got = _run(checker, tmp_path, ["plan n=%d variant=%d algo=%d pcg=%d" % c for c in cases])
    for c, line in zip(cases, got):
        assert list(map(int, line.split())) == pc.expected(*c), (c, dict(zip(pc.FIELDS, line.split())))
    # the examples of the thresholds, spelled out
    p = {n: dict(zip(pc.FIELDS, pc.expected(n))) for n in SIZES}
    assert (p[7]["schur"], p[7]["pace_depth"], p[7]["poll"]) == (pc.SCHUR_ALL_W, 1, 0)
    assert (p[8]["schur"], p[8]["pace_depth"]) == (pc.SCHUR_ALL, 2)
    assert (p[64]["poll"], p[64]["dev_stop"], p[64]["imu_lin"], p[64]["ngroups"]) == (1, 1, pc.IMU_RES_HESS, 4)
    assert (p[256]["left_looking"], p[256]["trsv"], p[256]["factor"], p[256]["chain_on"]) == (1, pc.TRSV, pc.FACTOR_LL, 1)
    assert p[65]["chain_on"] == p[255]["chain_on"] == 0 and p[64]["chain_on"] == 1
    assert (p[3]["results_block"], p[4]["results_block"], p[8]["arena_on"], p[9]["arena_on"], p[9]["inc_copy"]) == (1, 0, 1, 0, 1)
    assert (p[1]["factor"], p[1]["word_report"], p[3]["factor"], p[15]["ngroups"], p[16]["ngroups"], p[63]["ngroups"]) == (pc.FACTOR_STEP4_ONE, 1, pc.FACTOR_STEP4, 1, 2, 2)


# ------------------------------------------------------------------------------------------------------------ precedence
PRECEDENCE = [
    # hook > environment > default: ll_min
    ("n=300", dict(left_looking=1)), ("n=300 VBA_LL_MIN=512", dict(left_looking=0, trsv=pc.TRSV_P)), ("n=512 VBA_LL_MIN=512", dict(left_looking=1)),
    ("n=8 VBA_LL_MIN=512 ov.ll_min=8", dict(left_looking=1, factor=pc.FACTOR_LL, trsv=pc.TRSV, zero_s=1, chain_on=1)),
    ("n=7 VBA_LL_MIN=4 ov.ll_min=8", dict(left_looking=0)),
    # VBA_RIGHT_LOOKING beats the hook
    ("n=300 VBA_RIGHT_LOOKING=1 ov.ll_min=8", dict(left_looking=0, factor=pc.FACTOR_STEP4, trsv=pc.TRSV_P, chain_on=0)),
    ("n=300 VBA_RIGHT_LOOKING=", dict(left_looking=0)),
    # chol_step
    ("n=8", dict(step_form=4, factor=pc.FACTOR_STEP4)), ("n=8 VBA_CHOL_STEP=1", dict(step_form=1, factor=pc.FACTOR_STEP1)),
    ("n=8 VBA_CHOL_STEP=1 ov.chol_step=4", dict(step_form=4, factor=pc.FACTOR_STEP4)), ("n=1 ov.chol_step=1", dict(step_form=1, factor=pc.FACTOR_STEP1)),
    ("n=300 ov.chol_step=1", dict(factor=pc.FACTOR_LL)), ("n=8 pcg=1 ov.chol_step=1", dict(factor=pc.FACTOR_PCG, trsv=-1)),
    # the A/B paths: trsv_old is irrelevant when left-looking; schur_split; pcg_jacobi
    ("n=8 VBA_TRSV_OLD=1", dict(trsv=pc.TRSV)), ("n=8 VBA_TRSV_OLD=1 ov.trsv_old=0", dict(trsv=pc.TRSV_P)), ("n=8 ov.trsv_old=1", dict(trsv=pc.TRSV)),
    ("n=300 ov.trsv_old=0", dict(trsv=pc.TRSV)), ("n=300 VBA_TRSV_OLD=1", dict(trsv=pc.TRSV)),
    ("n=7 VBA_SCHUR_SPLIT=1", dict(schur=pc.SCHUR_SPLIT_W)), ("n=8 ov.schur_split=1", dict(schur=pc.SCHUR_SPLIT)),
    ("n=8 VBA_SCHUR_SPLIT=1 ov.schur_split=0", dict(schur=pc.SCHUR_ALL)), ("n=8 variant=1 VBA_SCHUR_SPLIT=1", dict(schur=pc.SCHUR3)),
    ("n=8 pcg=1 VBA_PCG_JACOBI=1", dict(pcg_tri=0)), ("n=8 pcg=1 VBA_PCG_JACOBI=1 ov.pcg_jacobi=0", dict(pcg_tri=1)), ("n=8 pcg=1 ov.pcg_jacobi=1", dict(pcg_tri=0)),
    # VBA_LIN_IMU_SPLIT acts only on the inverse-depth variant, and only below 64 windows
    ("n=8 VBA_LIN_IMU_SPLIT=1", dict(imu_lin=pc.IMU_PAIR)), ("n=8 variant=1 VBA_LIN_IMU_SPLIT=1", dict(imu_lin=pc.IMU_PAIR)), ("n=8 variant=1", dict(imu_lin=pc.IMU_PAIR)),
    ("n=64 VBA_LIN_IMU_SPLIT=1", dict(imu_lin=pc.IMU_RES_HESS)),
    # chain
    ("n=8 VBA_NO_CHAIN=1", dict(chain_on=0)), ("n=300 ov.no_chain=1", dict(chain_on=0)), ("n=100 VBA_CHAIN_RL_MAX=128", dict(chain_on=1)),
    ("n=8 VBA_ONE_CHAIN=1", dict(two_sided=0)), ("n=8 VBA_ST_ROW_LDS=1", dict(row_lds=1)),
    ("n=9 VBA_ARENA_MAX=16", dict(arena_on=1, inc_copy=0)), ("n=9 VBA_UPLOAD_NO_OVERLAP=1", dict(arena_on=0, inc_copy=0)),
    ("n=8 VBA_PACE_DEPTH=3", dict(pace_depth=3)), ("n=8 VBA_PACE_DEPTH=0", dict(pace_depth=2)), ("n=8 ov.stop_after=5", dict(dbg_stop_after=5)),
    # streams: hook > VBA_STREAMS > (a lane: VBA_LANE_STREAMS) > the policy by batch size
    ("n=64", dict(ngroups=4)), ("n=64 VBA_STREAMS=2", dict(ngroups=2)), ("n=64 VBA_STREAMS=2 ov.streams=3", dict(ngroups=3)), ("n=64 ov.streams=1", dict(ngroups=1)),
    ("n=64 lane=1", dict(ngroups=2)), ("n=64 lane=1 VBA_LANE_STREAMS=3", dict(ngroups=3)), ("n=64 lane=1 VBA_LANE_STREAMS=3 VBA_STREAMS=4", dict(ngroups=4)),
    ("n=64 lane=1 VBA_LANE_STREAMS=3 ov.streams=1", dict(ngroups=1)), ("n=64 lane=1 VBA_LANE_STREAMS=0", dict(ngroups=4)), ("n=64 VBA_LANE_STREAMS=3", dict(ngroups=4)),
    # a profiling run gets one group; ngroups <= n / 8, <= the streams the handle can have, <= 14
    ("n=64 profile=1", dict(ngroups=1)), ("n=1 profile=1", dict(word_report=0)), ("n=20 VBA_STREAMS=14", dict(ngroups=2)), ("n=7 ov.streams=4", dict(ngroups=1)),
    ("n=15 ov.streams=4", dict(ngroups=1)), ("n=1000 ov.streams=20", dict(ngroups=14)), ("n=1000 ov.streams=20 avail=3", dict(ngroups=3)),
    ("n=64 lane=1 VBA_LANE_STREAMS=3 avail=2", dict(ngroups=2)), ("n=100 ov.streams=14", dict(ngroups=12)),
]


def test_precedence_of_hook_environment_and_default(checker, tmp_path):
    got = _plans(checker, tmp_path, [c for c, _ in PRECEDENCE])
    for (case, want), g in zip(PRECEDENCE, got):
        assert {k: g[k] for k in want} == want, (case, g)


# ---------------------------------------------------------------------------------------------------------------- groups
def test_group_bounds_cover_the_batch_in_order(checker, tmp_path):
    cases = [(n, g) for n in (8, 9, 37, 64, 100, 4096) for g in (1, 2, 3, 4, 14)]
    for (n, g), line in zip(cases, _run(checker, tmp_path, ["groups n=%d g=%d" % c for c in cases])):
        b = list(map(int, line.split()))
        assert len(b) == g + 1 and b[0] == 0 and b[-1] == n and all(x <= y for x, y in zip(b, b[1:])), (n, g, b)
        sizes = [y - x for x, y in zip(b, b[1:])]
        assert max(sizes) - min(sizes) <= 1                                      # an even split
    # the default policy: no group below the 8 windows of the XCD-aware mapping (xcd_windows, schur_map)
    ns = list(range(1, 140)) + [255, 256, 1000, 4096]
    plans = _plans(checker, tmp_path, ["n=%d" % n for n in ns] + ["n=%d ov.streams=14" % n for n in ns])
    lines = _run(checker, tmp_path, ["groups n=%d g=%d" % (p["n_win"], p["ngroups"]) for p in plans])
    for p, line in zip(plans, lines):
        b = list(map(int, line.split()))
        assert p["ngroups"] == 1 or min(y - x for x, y in zip(b, b[1:])) >= 8, (p, b)
        assert p["ngroups"] <= max(1, p["n_win"] // 8)


# ---------------------------------------------------------------------------------------------------------------- chunks
def _chunks(line):
    t = line.split()
    assert t[-2] == "lanes"
    return list(map(int, t[:-2])), int(t[-1])


CHUNKS = [
    # defaults: VBA_CHUNK = 1536, c = 384, ramp 384, 768, 1248, 1728 -- a step is taken while at least 256 windows stay behind it
    ("n=4096", [384, 768, 1248, 1696], 2),      # the fourth step, 1728 + 256 > 1696, is not taken
    ("n=1535", [384, 768, 383], 2), ("n=1536", [384, 768, 384], 2), ("n=1537", [384, 768, 385], 2),
    ("n=3000", [384, 768, 1248, 600], 2),
    ("n=300", [300], 1),                        # 300 < 384 + 256: one chunk, hence one lane
    ("n=4096 VBA_NO_RAMP=1", [1365, 1365, 1366], 2),         # ceil(4096 / 1536) = 3 equal chunks, bounds floor(4096 q / 3)
    ("n=29 ov.chunk=10", [9, 10, 10], 2),       # below 1024: no ramp; ceil(29 / 10) = 3 chunks, bounds floor(29 q / 3) = 9, 19, 29
    ("n=4096 VBA_CHUNKS=384,1024", [384, 1024, 2688], 2), ("n=300 VBA_CHUNKS=384,1024", [300], 1),
    # hook > environment > default: chunk (2048: c = 512, steps 512, 1024, 1664, 2304; 1024: c = 256, steps 256, 512, 832, 1152,
    # then ceil(1344 / 1152) = 2 equal chunks) and lanes (never more than there are chunks)
    ("n=4096 VBA_CHUNK=2048", [512, 1024, 1664, 896], 2),
    ("n=4096 VBA_CHUNK=2048 ov.chunk=1024", [256, 512, 832, 1152, 672, 672], 2),
    ("n=4096 VBA_LANES=3", [384, 768, 1248, 1696], 3), ("n=4096 VBA_LANES=3 ov.lanes=4", [384, 768, 1248, 1696], 4),
    ("n=4096 ov.lanes=9", [384, 768, 1248, 1696], 4), ("n=4096 VBA_LANES=0", [384, 768, 1248, 1696], 1),
]


def test_chunk_bounds(checker, tmp_path):
    for (case, sizes, lanes), line in zip(CHUNKS, _run(checker, tmp_path, ["chunks " + c for c, _, _ in CHUNKS])):
        assert _chunks(line) == (sizes, lanes), case
    # every result tiles [0, n) with positive sizes; from 256 windows on no chunk of a chunk_max >= 1024 falls below 256 windows
    cases = [(n, c, r) for n in list(range(1, 40)) + list(range(200, 6000, 37)) + [256, 511, 512, 1279, 1280, 100000]
             for c in (1, 10, 255, 1023, 1024, 1536, 2048, 5000) for r in ("", " VBA_NO_RAMP=1")]
    got = _run(checker, tmp_path, ["chunks n=%d ov.chunk=%d%s" % c for c in cases])
    for (n, c, r), line in zip(cases, got):
        sizes, _ = _chunks(line)
        assert sum(sizes) == n and min(sizes) > 0, (n, c, r, sizes)
        if n >= 256 and c >= 1024:
            assert min(sizes) >= 256, (n, c, r, sizes)
        if r or c < 1024:
            assert max(sizes) <= c and max(sizes) - min(sizes) <= 1, (n, c, r, sizes)


# ----------------------------------------------------------------------------------------------------------------- knobs
def _knobs(line):
    return dict(t.split("=", 1) for t in line.split())


def test_knob_parsing_and_read_time(checker, tmp_path):
    vals = [None, "", "0", "1", "abc", "12abc", "-3"]
    lines = ["knobs" + ("" if v is None else " VBA_NO_CHAIN=%s VBA_LL_MIN=%s VBA_CHUNKS=%s" % (v, v, v)) for v in vals]
    got = [_knobs(l) for l in _run(checker, tmp_path, lines)]
    assert [g["VBA_NO_CHAIN"] for g in got] == ["0", "1", "1", "1", "1", "1", "1"]              # a flag: set at all
    assert [g["VBA_LL_MIN"] for g in got] == ["256", "0", "0", "1", "0", "12", "-3"]           # an int: atoi, the default when unset
    assert [g["VBA_CHUNKS"] for g in got] == ["(null)", "", "0", "1", "abc", "12abc", "-3"]
    # the defaults of every knob
    d = got[0]
    assert {k: v for k, v in d.items() if v not in ("0", "(null)")} == {
        "VBA_LANE_STREAMS": "2", "VBA_LL_MIN": "256", "VBA_CHAIN_RL_MAX": "64", "VBA_CHAIN_MIN": "4", "VBA_ORDER": "-1", "VBA_ARENA_MAX": "8",
        "VBA_UPLOAD_THREADS": str(-2 ** 31), "LOCAL_WORLD_SIZE": "1", "VBA_CHUNK": "1536", "VBA_LANES": "2", "VBA_RUN_SLOTS": "1"}
    # the process snapshot and three uploads: the per-upload / per-call variables are read at each, the others once
    table, reads = _run(checker, tmp_path, ["table", "reads"])
    each = {"VBA_NO_CHAIN", "VBA_ONE_CHAIN", "VBA_ST_ROW_LDS", "VBA_CHUNKS"}
    entries = [t.split(":") for t in table.split()]
    assert {n for n, _, when in entries if when == "each"} == each
    assert _knobs(reads) == {n: ("3" if n in each else "1") for n, _, _ in entries}
    flags = {n for n, kind, _ in entries if kind == "flag"}
    assert {"VBA_RIGHT_LOOKING", "VBA_NO_CHAIN", "VBA_ONE_CHAIN", "VBA_TRSV_OLD", "VBA_SCHUR_SPLIT", "VBA_LIN_IMU_SPLIT", "VBA_PCG_JACOBI", "VBA_ST_ROW_LDS",
            "VBA_UPLOAD_NO_OVERLAP", "VBA_RANK_CPUS", "VBA_NO_RAMP", "VBA_TIMING"} == flags


# --------------------------------------------------------------------------------------------------------- single source
def test_the_environment_is_read_in_one_header_and_documented_row_by_row(checker, tmp_path):
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip")) and name != "vba_host_plan.h":
            assert "getenv(" not in open(os.path.join(CSRC, name)).read(), name
    names = [t.split(":")[0] for t in _run(checker, tmp_path, ["table"])[0].split()]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 8. Environment switches"):]
    tab = sec[:sec.index("Read outside the library")]
    rows = [m.group(1) for m in re.finditer(r"^\| `(\w+)` \|", tab, flags=re.M)]
    assert rows == names                                   # one row per entry, in the header's order (hence no variable twice)
    assert {n for n in names if n.startswith("VBA_")} == set(re.findall(r"VBA_\w+", "\n".join(l.split("|")[1] for l in tab.splitlines() if l.startswith("| `"))))
