"""Measures vba_mappoint_update on the device and writes profiles/mappoint_bench.json (fails without a device: there is no CPU path).

  keyframe       one keyframe's worth as ONE call: 1 000 points, observation counts long-tailed with a mean near 8, both parts
  single_points  the same 1 000 points as 1 000 single-point calls, same process, same handle: the per-point form of the reference
                 moved onto the device.  This feature's own baseline: the parent commit has nothing to compare with
  ba_write_back  5 000 points, the normal part only: the UpdateNormalAndDepth loop behind a local BA
  one_1024       one point of 1 024 observations: a workgroup item alone
  keyframes_64   a ragged batch of 64 keyframes' worth (64 problems of 1 000 points) in one call
  numpy          the NumPy yardstick (tests/mappoint_ref.py) on the one keyframe, one host core: NumPy, not a baseline
  bytes          what the keyframe call copies each way, from the record sizes

Host clock around LocalBA.mappoint_update_call, which returns after the library's stream synchronise and includes the host's checks,
the item table and the packing; building the ctypes views is outside the timed region.  Medians with p10-p90.  The GPU work runs in a
child process under a time limit; if it fails or runs out of time nothing more is started.  Two sanity conditions are asserted: a call
is one kernel launch, and the one call returns bit for bit what the single-point calls return.  There is no pass mark.

usage: python scripts/mappoint_bench.py [--out profiles/mappoint_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mappoint_cases as cases  # noqa: E402
import mappoint_ref as ref_mod  # noqa: E402
from mc_slam_amd import abi, backend  # noqa: E402

SIZEOF_ITEM = 80      # MpItem of mc_slam_amd/csrc/vba_layout.h
STEP_SECONDS = 420
ARRAYS = ("best_obs", "best_median", "n_desc", "desc", "normal", "dist_max", "dist_min", "desc_state", "normal_state")


def _up(b):
    return (b + 255) // 256 * 256


def arena_bytes(p):
    """bytes of the one H2D and the one D2H copy of a call of one problem in which every point has work (the arena layout of
    vba_mappoint_update), and its workgroups"""
    cnt = np.diff(p.obs_begin)
    ni, nb = p.n_pt, int((cnt > 256).sum())
    nd = int(sum((p.kf_bad[p.obs_kf[b:e]] == 0).sum() for b, e, w in zip(p.obs_begin[:-1], p.obs_begin[1:], p.what) if w & 1))
    no = int(cnt[(p.what & 2) != 0].sum())
    h2d = _up(SIZEOF_ITEM * (ni + 1)) + _up(24 * (p.n_kf + 1)) + _up(4 * (no + 1)) + _up(32 * (nd + 1))
    d2h = _up(4 * (ni + 1)) + _up(40 * (ni + 1)) + _up(ni + 1)
    return h2d, d2h, nb + (ni - nb + 3) // 4


def point_of(p, i):
    b, e = p.obs_begin[i], p.obs_begin[i + 1]
    return abi.MapPointProblem(kf_center=p.kf_center, kf_bad=p.kf_bad, what=p.what[i:i + 1], obs_begin=[0, e - b], obs_kf=p.obs_kf[b:e], obs_desc=p.obs_desc[b:e],
                               pos=p.pos[i:i + 1], ref_kf=p.ref_kf[i:i + 1], ref_scale=p.ref_scale[i:i + 1], ref_top_scale=p.ref_top_scale[i:i + 1])


def timed(fn, min_calls, min_seconds):
    ts = []
    while len(ts) < min_calls or sum(ts) < min_seconds:
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return np.array(ts)


def _stats(t, scale):
    return dict(calls=int(len(t)), median=float(np.median(t) * scale), p10=float(np.percentile(t, 10) * scale), p90=float(np.percentile(t, 90) * scale),
                min=float(t.min() * scale), max=float(t.max() * scale))


def step():
    ba = backend.LocalBA(0)
    both = np.full(1000, 3, dtype=np.uint8)
    kf = cases.ragged(7000, 1000, n_kf=1100, force=(300, 700), what=both)
    singles = [ba.mappoint_update_pack([point_of(kf, i)]) for i in range(kf.n_pt)]
    one = ba.mappoint_update_pack([kf])
    wb = ba.mappoint_update_pack([cases.ragged(7100, 5000, n_kf=1100, force=(300,), what=np.full(5000, 2, dtype=np.uint8))])
    big = ba.mappoint_update_pack([cases.single(7200, 1024).copy(what=[3, 0])])
    many_p = [cases.ragged(7300 + k, 1000, n_kf=1100, force=(300, 700)[:k % 3], what=both) for k in range(64)]
    many = ba.mappoint_update_pack(many_p)

    def each():
        for s in singles:
            ba.mappoint_update_call(s)
    for _ in range(3):
        each(); ba.mappoint_update_call(one); ba.mappoint_update_call(wb); ba.mappoint_update_call(big); ba.mappoint_update_call(many)
    ba.mappoint_update_call(one)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    t_each = timed(each, 10, 0.5)
    t_one = timed(lambda: ba.mappoint_update_call(one), 50, 0.5)
    t_wb = timed(lambda: ba.mappoint_update_call(wb), 50, 0.5)
    t_big = timed(lambda: ba.mappoint_update_call(big), 50, 0.5)
    t_many = timed(lambda: ba.mappoint_update_call(many), 10, 0.5)
    ba.close()
    y = one[2][0].get()
    for i, s in enumerate(singles):
        x = s[2][0].get()
        for k in ARRAYS:
            assert getattr(x, k)[0].tobytes() == getattr(y, k)[i].tobytes(), (i, k)
    t0 = time.perf_counter()
    ref_mod.mappoint_ref(kf)
    t_np = time.perf_counter() - t0
    h2d, d2h, grid = arena_bytes(kf)
    cnt = np.diff(kf.obs_begin)
    return dict(points=int(kf.n_pt), observations=int(kf.n_obs), mean_observations=float(cnt.mean()), max_observations=int(cnt.max()), workgroups=int(grid),
                kernel_launches=int(launches), h2d_bytes=int(h2d), d2h_bytes=int(d2h), desc_done=int(y.n_desc_done), normal_done=int(y.n_normal_done),
                keyframe_us=_stats(t_one, 1e6), single_points_us=_stats(t_each, 1e6), one_call_speedup_over_single_points=float(np.median(t_each) / np.median(t_one)),
                ba_write_back_points=5000, ba_write_back_us=_stats(t_wb, 1e6), one_1024_us=_stats(t_big, 1e6),
                keyframes_64_points=int(sum(p.n_pt for p in many_p)), keyframes_64_observations=int(sum(p.n_obs for p in many_p)), keyframes_64_us=_stats(t_many, 1e6),
                numpy_yardstick_keyframe_ms=float(t_np * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mappoint_bench.json"))
    ap.add_argument("--step", action="store_true", help="run the GPU work in this process and print its JSON (what the parent starts)")
    a = ap.parse_args()
    if a.step:
        print("STEP " + json.dumps(step()))
        return 0
    out = dict(what="vba_mappoint_update (k_mappoint_update): host clock around calls that end in the library's stream synchronise; one keyframe's map points")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step"], capture_output=True, text=True, timeout=STEP_SECONDS)
    except subprocess.TimeoutExpired:
        print("the GPU step ran out of its %d s" % STEP_SECONDS, file=sys.stderr)
        return 1
    lines = [l for l in r.stdout.splitlines() if l.startswith("STEP ")]
    if r.returncode != 0 or not lines:
        print("the GPU step failed (exit %d)\n%s" % (r.returncode, r.stderr[-2000:]), file=sys.stderr)
        return 1
    out.update(json.loads(lines[-1][5:]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
