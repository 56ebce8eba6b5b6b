"""Measures vba_sim3_optimize on the device and writes profiles/sim3_bench.json (fails without a device: there is no CPU path).

  latency      one 120-pair candidate per call: median and spread of >= 200 calls (and >= 0.5 s of timed work)
  batched      one call with 4 096 ragged candidates (60-400 pairs, the generator's mix of free / fixed scale and outlier fractions)
  singles      the same 4 096 candidates as 4 096 calls, same process, same handle
  bytes        what one batched call copies each way

Host clock around LocalBA.sim3_call, which returns after the library's stream synchronise; building the ctypes views and putting
the initial estimates back between calls are outside the timed region.  Two sanity conditions are asserted: the batched call is one kernel launch, and it is faster than the single calls it
replaces.

usage: python scripts/sim3_bench.py [--candidates 4096] [--out profiles/sim3_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mc_slam_amd import backend, synth  # noqa: E402

SIZEOF_DESC, SIZEOF_OUT = 176, 112      # Sim3Desc / Sim3Out of mc_slam_amd/csrc/vba_layout.h


def _up(b):
    return (b + 255) // 256 * 256


def arena_bytes(n_problems, n_pairs, want_chi2):
    """bytes of the one H2D and the one D2H copy of a call (the arena layout of vba_sim3_optimize)"""
    h2d = _up(SIZEOF_DESC * n_problems) + _up((6 * n_pairs + 6) * 8) + _up((4 * n_pairs + 4) * 8) + _up((2 * n_pairs + 2) * 8)
    d2h = _up(SIZEOF_OUT * n_problems) + _up(n_pairs + 1) + (_up((2 * n_pairs + 2) * 8) if want_chi2 else 0)
    return h2d, d2h


def timed(setup, fn, min_calls, min_seconds):
    """durations of fn() alone; setup() (putting the initial estimates back) runs before every call, outside the clock"""
    ts = []
    while len(ts) < min_calls or sum(ts) < min_seconds:
        setup()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return np.array(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_bench.json"))
    a = ap.parse_args()
    ba = backend.LocalBA(0)
    rng = np.random.default_rng(0)

    one = ba.sim3_pack([synth.make_sim3_pair(12, 120)], want_chi2=False)
    for _ in range(20):
        ba.sim3_reset(one); ba.sim3_call(one)

    lat = timed(lambda: ba.sim3_reset(one), lambda: ba.sim3_call(one), 200, 0.5)

    probs = [synth.make_sim3_pair(1000 + k, int(rng.integers(60, 401)), fix_scale=bool(k % 4 == 3), outlier_frac=(0.0, 0.1, 0.2, 0.3)[k % 4])
             for k in range(a.candidates)]
    n_pairs = sum(p.n_pairs for p in probs)
    batch = ba.sim3_pack(probs, want_chi2=False)
    for _ in range(2):
        ba.sim3_reset(batch); ba.sim3_call(batch)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches

    tb = timed(lambda: ba.sim3_reset(batch), lambda: ba.sim3_call(batch), 3, 0.5)
    res = [b.get(s) for b, s in zip(batch[2], batch[1])]

    singles = [ba.sim3_pack([p], want_chi2=False) for p in probs]
    for s in singles[:20]:
        ba.sim3_call(s); ba.sim3_reset(s)
    t0 = time.perf_counter()
    for s in singles:
        ba.sim3_call(s)
    t_single = time.perf_counter() - t0
    same = all(b.get(s[1][0]).S12.tobytes() == r.S12.tobytes() for s, r in zip(singles, res) for b in s[2])
    assert same, "single calls and the batched call disagree"
    assert np.median(tb) < t_single, (float(np.median(tb)), t_single)

    h2d, d2h = arena_bytes(len(probs), n_pairs, False)
    out = dict(
        what="vba_sim3_optimize (k_sim3_opt): host clock around calls that end in the library's stream synchronise",
        latency_one_120_pair_candidate_us=dict(calls=int(len(lat)), median=float(np.median(lat) * 1e6), p10=float(np.percentile(lat, 10) * 1e6),
                                               p90=float(np.percentile(lat, 90) * 1e6), min=float(lat.min() * 1e6), max=float(lat.max() * 1e6)),
        batched=dict(candidates=len(probs), pairs=int(n_pairs), calls=int(len(tb)), median_ms=float(np.median(tb) * 1e3),
                     min_ms=float(tb.min() * 1e3), max_ms=float(tb.max() * 1e3), candidates_per_s=float(len(probs) / np.median(tb)),
                     kernel_launches=int(launches), h2d_bytes=int(h2d), d2h_bytes=int(d2h)),
        singles=dict(calls=len(probs), total_ms=float(t_single * 1e3), candidates_per_s=float(len(probs) / t_single)),
        batched_speedup_over_singles=float(t_single / np.median(tb)),
        inliers_mean=float(np.mean([r.n_inliers for r in res])), stage2_its_mean=float(np.mean([r.its_done[1] for r in res])),
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    ba.close()


if __name__ == "__main__":
    main()
