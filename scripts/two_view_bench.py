"""Measures vba_two_view_init on the device and writes profiles/two_view_bench.json (fails without a device: there is no CPU path).

  latency      one frame pair of 300 matches x 200 hypotheses per call: median and p10-p90 of >= 100 calls (and >= 0.5 s of timed work)
  batched      one call with a ragged batch of pairs (100-500 matches, 200 hypotheses each)
  singles      the same pairs as single calls, same process, same handle
  bytes        what a call copies each way, from the record sizes
  numpy        the NumPy yardstick (tests/two_view_ref.py) on a few of the same pairs: a label, not a baseline

Host clock around LocalBA.two_view_call, which returns after the library's stream synchronise; building the ctypes views is outside
the timed region.  Every step that uses the GPU runs in a child process of its own under a time limit; after a step that fails or
runs out of time nothing more is started.  One sanity condition is asserted: a call is at most two kernel launches.  No CPU
baseline of the reference's own Initialize exists (it needs OpenCV), so no ratio against it is formed here.

usage: python scripts/two_view_bench.py [--pairs 256] [--out profiles/two_view_bench.json]
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

SIZEOF_DESC, SIZEOF_OUT = 104, 400      # TvDesc / TvOut of mc_slam_amd/csrc/vba_layout.h
STEP_SECONDS = dict(latency=120, batched=240, singles=240)
KINDS = ("general", "plane", "general", "rotation")


def _up(b):
    return (b + 255) // 256 * 256


def arena_bytes(probs):
    """bytes of the one H2D and the one D2H copy of a call without per-hypothesis scores (the arena layout of vba_two_view_init)"""
    n = len(probs)
    k1, k2, m, h = (sum(getattr(p, a) for p in probs) for a in ("n_keys1", "n_keys2", "n_matches", "n_hyp"))
    h2d = _up(SIZEOF_DESC * n) + _up((2 * k1 + 2) * 8) + _up((2 * k2 + 2) * 8) + _up((2 * m + 2) * 4) + _up((8 * h + 8) * 4)
    d2h = _up(SIZEOF_OUT * n) + 2 * _up(m + 1) + _up(k1 + 1) + _up((3 * k1 + 3) * 8)
    return h2d, d2h


def pair(seed, n, n_hyp=200):
    return synth.make_two_view(seed, n, n_hyp, KINDS[seed % 4], extra_keys=(n // 2, n // 2), outlier_frac=0.1)


def ragged(n_pairs):
    rng = np.random.default_rng(0)
    return [pair(1000 + k, int(rng.integers(100, 501))) for k in range(n_pairs)]


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
    p = pair(12, 300)
    one = ba.two_view_pack([p], want_scores=False)
    for _ in range(10):
        ba.two_view_call(one)
    launches = ba.get_profile()["kernel_launches"]
    assert 1 <= launches <= 2, launches
    lat = timed(lambda: ba.two_view_call(one), 100, 0.5)
    ba.close()
    h2d, d2h = arena_bytes([p])
    r = one[2][0].get()
    return dict(latency_one_pair_300_matches_200_hypotheses_us=dict(_stats(lat, 1e6), kernel_launches=int(launches), h2d_bytes=int(h2d), d2h_bytes=int(d2h),
                                                                    ok=int(r.ok), model=int(r.model)))


def step_batched(a):
    import two_view_ref as ref
    ba = backend.LocalBA(0)
    probs = ragged(a.pairs)
    batch = ba.two_view_pack(probs, want_scores=False)
    for _ in range(2):
        ba.two_view_call(batch)
    launches = ba.get_profile()["kernel_launches"]
    assert 1 <= launches <= 2, launches
    tb = timed(lambda: ba.two_view_call(batch), 5, 0.5)
    res = [b.get() for b in batch[2]]
    ba.close()
    k = min(4, len(probs))
    t0 = time.perf_counter()
    oks = [ref.two_view(p)["ok"] for p in probs[:k]]
    t_np = (time.perf_counter() - t0) / k
    h2d, d2h = arena_bytes(probs)
    return dict(batched=dict(pairs=len(probs), matches=int(sum(p.n_matches for p in probs)), hypotheses=int(sum(p.n_hyp for p in probs)), calls=int(len(tb)),
                             median_ms=float(np.median(tb) * 1e3), min_ms=float(tb.min() * 1e3), max_ms=float(tb.max() * 1e3),
                             pairs_per_s=float(len(probs) / np.median(tb)), kernel_launches=int(launches), h2d_bytes=int(h2d), d2h_bytes=int(d2h),
                             ok_share=float(np.mean([r.ok for r in res]))),
                numpy_yardstick=dict(what="tests/two_view_ref.py in float64 on the host, per pair: NumPy, not a baseline", pairs=k,
                                     ms_per_pair=float(t_np * 1e3), ok_equal=bool(oks == [r.ok for r in res[:k]])))


def step_singles(a):
    ba = backend.LocalBA(0)
    probs = ragged(a.pairs)
    singles = [ba.two_view_pack([p], want_scores=False) for p in probs]
    for s in singles[:5]:
        ba.two_view_call(s)
    t0 = time.perf_counter()
    for s in singles:
        ba.two_view_call(s)
    t_single = time.perf_counter() - t0
    ba.close()
    return dict(singles=dict(calls=len(probs), total_ms=float(t_single * 1e3), pairs_per_s=float(len(probs) / t_single)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_bench.json"))
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), help="run one step in this process and print its JSON (what the parent starts)")
    a = ap.parse_args()
    steps = dict(latency=step_latency, batched=step_batched, singles=step_singles)
    if a.step:
        print("STEP " + json.dumps(steps[a.step](a)))
        return 0
    out = dict(what="vba_two_view_init (k_two_view): host clock around calls that end in the library's stream synchronise")
    for step in ("latency", "batched", "singles"):
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
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
