"""Measures vba_triangulate on the device and writes profiles/triangulate_bench.json (fails without a device: there is no CPU path).

  latency      one keyframe pair of 150 matches per call: median and p10-p90 of >= 200 calls (and >= 0.5 s of timed work)
  keyframe     one keyframe's worth, 20 pairs of 150 matches: as 20 calls and as one call of 20 pairs
  batched      one call with 4 096 ragged pairs (20-400 matches)
  singles      the same 4 096 pairs as 4 096 calls, same process, same handle
  bytes        what a call copies each way, from the record sizes
  numpy        the NumPy yardstick (tests/triangulate_ref.py) on a few of the same pairs: a label, not a baseline

Host clock around LocalBA.triangulate_call, which returns after the library's stream synchronise; building the ctypes views is
outside the timed region.  Every step that uses the GPU runs in a child process of its own under a time limit; after a step that
fails or runs out of time nothing more is started.  One sanity condition is asserted: a call is one kernel launch.  No CPU
baseline of the reference's own per-match loop exists (it needs OpenCV), so no ratio against it is formed here.

usage: python scripts/triangulate_bench.py [--pairs 4096] [--out profiles/triangulate_bench.json]
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

from mc_slam_amd import backend, synth  # noqa: E402

SIZEOF_DESC, SIZEOF_BLOCK, NT = 360, 8, 256      # TriDesc / TriBlock / VBA_TRI_NT of mc_slam_amd/csrc/vba_layout.h
STEP_SECONDS = dict(latency=120, keyframe=120, batched=240, singles=240)
KINDS = ("std", "std", "forward", "far")


def _up(b):
    return (b + 255) // 256 * 256


def arena_bytes(probs):
    """bytes of the one H2D and the one D2H copy of a call (the arena layout of vba_triangulate)"""
    n, n_tot = len(probs), sum(p.n_matches for p in probs)
    l_tot = sum(2 * (p.n_levels1 + p.n_levels2) for p in probs)
    n_blocks = sum((p.n_matches + NT - 1) // NT for p in probs)
    h2d = _up(SIZEOF_DESC * n) + _up(SIZEOF_BLOCK * (n_blocks + 1)) + _up((l_tot + 1) * 8) + _up((4 * n_tot + 4) * 8) + _up(2 * n_tot + 2)
    d2h = _up((3 * n_tot + 3) * 8) + _up(n_tot + 1)
    return h2d, d2h


def pair(seed, n):
    return synth.make_triangulate(seed, n, KINDS[seed % 4])


def ragged(n_pairs):
    rng = np.random.default_rng(0)
    return [pair(1000 + k, int(rng.integers(20, 401))) for k in range(n_pairs)]


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


def step_latency(a):
    ba = backend.LocalBA(0)
    p = pair(12, 150)
    one = ba.triangulate_pack([p])
    for _ in range(20):
        ba.triangulate_call(one)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    lat = timed(lambda: ba.triangulate_call(one), 200, 0.5)
    ba.close()
    h2d, d2h = arena_bytes([p])
    return dict(latency_one_150_match_pair_us=dict(_stats(lat, 1e6), kernel_launches=int(launches), h2d_bytes=int(h2d), d2h_bytes=int(d2h),
                                                   accepted=int(one[2][0].get().n_accepted)))


def step_keyframe(a):
    ba = backend.LocalBA(0)
    probs = [pair(200 + k, 150) for k in range(20)]
    singles = [ba.triangulate_pack([p]) for p in probs]
    batch = ba.triangulate_pack(probs)

    def twenty():
        for s in singles:
            ba.triangulate_call(s)
    for _ in range(5):
        twenty(); ba.triangulate_call(batch)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    t20 = timed(twenty, 100, 0.5)
    t1 = timed(lambda: ba.triangulate_call(batch), 100, 0.5)
    ba.close()
    for s, b in zip(singles, batch[2]):
        assert s[2][0].get().x3d.tobytes() == b.get().x3d.tobytes()
    h2d, d2h = arena_bytes(probs)
    return dict(keyframe_20_pairs_of_150_matches_us=dict(as_20_calls=_stats(t20, 1e6), as_one_call=dict(_stats(t1, 1e6), h2d_bytes=int(h2d), d2h_bytes=int(d2h))))


def step_batched(a):
    import triangulate_ref as ref
    ba = backend.LocalBA(0)
    probs = ragged(a.pairs)
    n_tot = sum(p.n_matches for p in probs)
    batch = ba.triangulate_pack(probs)
    for _ in range(2):
        ba.triangulate_call(batch)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    tb = timed(lambda: ba.triangulate_call(batch), 5, 0.5)
    res = [b.get() for b in batch[2]]
    ba.close()
    k = min(16, len(probs))
    t0 = time.perf_counter()
    acc = [ref.triangulate(p)["n_accepted"] for p in probs[:k]]
    t_np = (time.perf_counter() - t0) / k
    assert acc == [r.n_accepted for r in res[:k]], (acc, [r.n_accepted for r in res[:k]])
    h2d, d2h = arena_bytes(probs)
    return dict(batched=dict(pairs=len(probs), matches=int(n_tot), calls=int(len(tb)), median_ms=float(np.median(tb) * 1e3), min_ms=float(tb.min() * 1e3),
                             max_ms=float(tb.max() * 1e3), pairs_per_s=float(len(probs) / np.median(tb)), matches_per_s=float(n_tot / np.median(tb)),
                             kernel_launches=int(launches), h2d_bytes=int(h2d), d2h_bytes=int(d2h),
                             accepted_share=float(sum(r.n_accepted for r in res) / n_tot)),
                numpy_yardstick=dict(what="tests/triangulate_ref.py in float64 on the host, per pair: NumPy, not a baseline", pairs=k,
                                     matches=int(sum(p.n_matches for p in probs[:k])), ms_per_pair=float(t_np * 1e3)))


def step_singles(a):
    ba = backend.LocalBA(0)
    probs = ragged(a.pairs)
    singles = [ba.triangulate_pack([p]) for p in probs]
    for s in singles[:20]:
        ba.triangulate_call(s)
    t0 = time.perf_counter()
    for s in singles:
        ba.triangulate_call(s)
    t_single = time.perf_counter() - t0
    ba.close()
    return dict(singles=dict(calls=len(probs), total_ms=float(t_single * 1e3), pairs_per_s=float(len(probs) / t_single)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate_bench.json"))
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), help="run one step in this process and print its JSON (what the parent starts)")
    a = ap.parse_args()
    steps = dict(latency=step_latency, keyframe=step_keyframe, batched=step_batched, singles=step_singles)
    if a.step:
        print("STEP " + json.dumps(steps[a.step](a)))
        return 0
    out = dict(what="vba_triangulate (k_triangulate): host clock around calls that end in the library's stream synchronise")
    for step in ("latency", "keyframe", "batched", "singles"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--pairs", str(a.pairs)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS[step])
        except subprocess.TimeoutExpired:
            print("step %s ran out of its %d s: nothing more is started" % (step, STEP_SECONDS[step]), file=sys.stderr)
            return 1
        lines = [l for l in r.stdout.splitlines() if l.startswith("STEP ")]
        if r.returncode != 0 or not lines:
            print("step %s failed (exit %d): nothing more is started\n%s" % (step, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        out.update(json.loads(lines[-1][5:]))
    out["batched_speedup_over_singles"] = out["singles"]["total_ms"] / out["batched"]["median_ms"]
    k = out["keyframe_20_pairs_of_150_matches_us"]
    out["keyframe_one_call_speedup_over_20_calls"] = k["as_20_calls"]["median"] / k["as_one_call"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
