"""Measures vba_sim3_ransac on the device and writes profiles/sim3_ransac_bench.json (fails without a device: there is no CPU path).

  latency      one 120-pair candidate x 300 hypotheses per call: median and p10-p90 of >= 200 calls (and >= 0.5 s of timed work)
  batched      one call with 4 096 ragged candidates (60-400 pairs) x 300 hypotheses each
  singles      the same 4 096 candidates as 4 096 calls, same process, same handle
  bytes        what one batched call copies each way, from the record sizes
  numpy        the NumPy yardstick (tests/sim3_ransac_ref.py) on a few of the same candidates: a label, not a baseline

Host clock around LocalBA.sim3_ransac_call, which returns after the library's stream synchronise; building the ctypes views and
putting the solvers' states back between calls are outside the timed region.  min_inliers is set beyond reach, so every call
consumes all of its hypotheses.  Every step that uses the GPU runs in a child process of its own under a time limit; after a step
that fails or runs out of time nothing more is started.  One sanity condition is asserted: a call is one kernel launch.  A
kernel-only time comes from one separate `rocprofv3 --kernel-trace --stats -- python scripts/sim3_ransac_bench.py --step batched`.

usage: python scripts/sim3_ransac_bench.py [--candidates 4096] [--hyp 300] [--out profiles/sim3_ransac_bench.json]
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

SIZEOF_DESC, SIZEOF_OUT = 104, 160      # RansacDesc / RansacOut of mc_slam_amd/csrc/vba_layout.h
STEP_SECONDS = dict(latency=120, batched=240, singles=240)
NO_HIT = 10 ** 6


def _up(b):
    return (b + 255) // 256 * 256


def arena_bytes(n_problems, n_pairs, n_hyp, want_counts):
    """bytes of the one H2D and the one D2H copy of a call (the arena layout of vba_sim3_ransac)"""
    h2d = _up(SIZEOF_DESC * n_problems) + _up((6 * n_pairs + 6) * 8) + _up((2 * n_pairs + 2) * 8) + _up((3 * n_hyp + 3) * 4)
    d2h = _up(SIZEOF_OUT * n_problems) + _up(n_pairs + 1) + (_up((n_hyp + 1) * 4) if want_counts else 0)
    return h2d, d2h


def triples(rng, n, n_hyp):
    """three distinct indices per hypothesis, all hypotheses at once"""
    a = rng.integers(0, n, n_hyp)
    b = rng.integers(0, n - 1, n_hyp)
    b = b + (b >= a)
    c = rng.integers(0, n - 2, n_hyp)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    c = c + (c >= lo)
    c = c + (c >= hi)
    return np.stack([a, b, c], axis=1).astype(np.int32)


def candidate(seed, n, n_hyp):
    rng = np.random.default_rng(seed)
    p = synth.make_sim3_ransac(seed, n, fix_scale=bool(seed % 4 == 3), outlier_frac=(0.2, 0.3, 0.5, 0.6)[seed % 4])
    return p.copy(sample=triples(rng, n, n_hyp), min_inliers=NO_HIT)


def ragged(n_candidates, n_hyp):
    rng = np.random.default_rng(0)
    return [candidate(1000 + k, int(rng.integers(60, 401)), n_hyp) for k in range(n_candidates)]


def timed(setup, fn, min_calls, min_seconds):
    ts = []
    while len(ts) < min_calls or sum(ts) < min_seconds:
        setup()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return np.array(ts)


def step_latency(a):
    ba = backend.LocalBA(0)
    one = ba.sim3_ransac_pack([candidate(12, 120, a.hyp)], want_counts=False)
    for _ in range(20):
        ba.sim3_ransac_reset(one); ba.sim3_ransac_call(one)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    lat = timed(lambda: ba.sim3_ransac_reset(one), lambda: ba.sim3_ransac_call(one), 200, 0.5)
    ba.close()
    return dict(latency_one_120_pair_candidate_us=dict(hypotheses=a.hyp, calls=int(len(lat)), median=float(np.median(lat) * 1e6),
                                                       p10=float(np.percentile(lat, 10) * 1e6), p90=float(np.percentile(lat, 90) * 1e6),
                                                       min=float(lat.min() * 1e6), max=float(lat.max() * 1e6), kernel_launches=int(launches)))


def step_batched(a):
    import sim3_ransac_ref as ref
    ba = backend.LocalBA(0)
    probs = ragged(a.candidates, a.hyp)
    n_pairs, n_hyp = sum(p.n_pairs for p in probs), sum(p.n_hyp for p in probs)
    batch = ba.sim3_ransac_pack(probs, want_counts=False)
    for _ in range(2):
        ba.sim3_ransac_reset(batch); ba.sim3_ransac_call(batch)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    tb = timed(lambda: ba.sim3_ransac_reset(batch), lambda: ba.sim3_ransac_call(batch), 3, 0.5)
    res = [b.get(s) for b, s in zip(batch[2], batch[1])]
    ba.close()
    k = min(8, len(probs))
    t0 = time.perf_counter()
    best = [ref.ransac(p)["best_inliers"] for p in probs[:k]]
    t_np = (time.perf_counter() - t0) / k
    assert best == [r.best_inliers for r in res[:k]], (best, [r.best_inliers for r in res[:k]])
    h2d, d2h = arena_bytes(len(probs), n_pairs, n_hyp, False)
    return dict(batched=dict(candidates=len(probs), pairs=int(n_pairs), hypotheses=int(n_hyp), calls=int(len(tb)), median_ms=float(np.median(tb) * 1e3),
                             min_ms=float(tb.min() * 1e3), max_ms=float(tb.max() * 1e3), candidates_per_s=float(len(probs) / np.median(tb)),
                             pair_tests_per_s=float(sum(p.n_pairs * p.n_hyp for p in probs) / np.median(tb)),
                             kernel_launches=int(launches), h2d_bytes=int(h2d), d2h_bytes=int(d2h),
                             best_inliers_mean=float(np.mean([r.best_inliers for r in res]))),
                numpy_yardstick=dict(what="tests/sim3_ransac_ref.py in float64 on the host, per candidate: NumPy, not a baseline", candidates=k,
                                     ms_per_candidate=float(t_np * 1e3)))


def step_singles(a):
    ba = backend.LocalBA(0)
    probs = ragged(a.candidates, a.hyp)
    singles = [ba.sim3_ransac_pack([p], want_counts=False) for p in probs]
    for s in singles[:20]:
        ba.sim3_ransac_call(s); ba.sim3_ransac_reset(s)
    t0 = time.perf_counter()
    for s in singles:
        ba.sim3_ransac_call(s)
    t_single = time.perf_counter() - t0
    ba.close()
    return dict(singles=dict(calls=len(probs), total_ms=float(t_single * 1e3), candidates_per_s=float(len(probs) / t_single)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=4096)
    ap.add_argument("--hyp", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_ransac_bench.json"))
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), help="run one step in this process and print its JSON (what the parent starts)")
    a = ap.parse_args()
    if a.step:
        print("STEP " + json.dumps(dict(latency=step_latency, batched=step_batched, singles=step_singles)[a.step](a)))
        return 0
    out = dict(what="vba_sim3_ransac (k_sim3_ransac): host clock around calls that end in the library's stream synchronise")
    for step in ("latency", "batched", "singles"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--candidates", str(a.candidates), "--hyp", str(a.hyp)]
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
