"""Measures vba_search_triangulation on the device and writes profiles/search_tri_bench.json (fails without a device: there is no
CPU path).

  latency      one keyframe pair of 1 000 + 1 000 keypoints per call: median and p10-p90 of >= 200 calls (and >= 0.5 s of timed work)
  keyframe     one keyframe's worth, 20 such pairs: as 20 calls and as one call of 20 pairs
  batched      one call with 1 024 ragged pairs (80-700 keypoints a side)
  singles      the same 1 024 pairs as 1 024 calls, same process, same handle
  bytes        what a call copies each way, from the record sizes
  numpy        the NumPy yardstick (tests/search_tri_ref.py) on a few of the same pairs: a label, not a baseline

Host clock around LocalBA.search_triangulation_call, which returns after the library's stream synchronise and includes the host's
node join and packing; building the ctypes views is outside the timed region.  Every step that uses the GPU runs in a child
process of its own under a time limit; after a step that fails or runs out of time nothing more is started.  Two sanity conditions
are asserted: a call is one kernel launch, and the pairs checked against the yardstick agree with it.  The reference's own
function cannot be built here (it needs OpenCV and DBoW2), so no ratio against it is formed.

usage: python scripts/search_tri_bench.py [--pairs 1024] [--out profiles/search_tri_bench.json]
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

SIZEOF_DESC, SIZEOF_KEY, SIZEOF_QUERY, SIZEOF_OUT = 160, 64, 16, 144      # StDesc / StKey / StQuery / StOut of mc_slam_amd/csrc/vba_layout.h
STEP_SECONDS = dict(latency=180, keyframe=180, batched=300, singles=300)


def _up(b):
    return (b + 255) // 256 * 256


def arena_bytes(probs):
    """bytes of the one H2D and the one D2H copy of a call (the arena layout of vba_search_triangulation)"""
    n, k1, k2 = len(probs), sum(p.n_keys1 for p in probs), sum(p.n_keys2 for p in probs)
    ft, lv = sum(len(p.node_feat2) for p in probs), sum(2 * p.n_levels2 for p in probs)
    h2d = _up(SIZEOF_DESC * n) + _up(SIZEOF_KEY * (k1 + 1)) + _up(SIZEOF_KEY * (k2 + 1)) + _up(SIZEOF_QUERY * (k1 + 1)) + _up(4 * (ft + 1)) + _up(8 * (lv + 1))
    d2h = _up(SIZEOF_OUT * n) + _up(4 * (k1 + 1)) + 2 * _up(k1 + 1)
    return h2d, d2h


def evaluations(p):
    """Hamming distances a pair asks for: candidates of all queries"""
    import search_tri_ref as ref
    return int(sum(e - b for _, b, e in ref.node_join(p)))


def pair(seed):
    return synth.synth_match_pair(seed, n_true=800, n_distract1=200, n_distract2=200, n_nodes=40, flip_bits=14)


def ragged(n_pairs):
    rng = np.random.default_rng(0)
    out = []
    for k in range(n_pairs):
        n = int(rng.integers(60, 501))
        out.append(synth.synth_match_pair(1000 + k, n_true=n, n_distract1=int(rng.integers(20, 201)), n_distract2=int(rng.integers(20, 201)),
                                          n_nodes=max(2, n // 20), flip_bits=14, check_orientation=bool(k % 2)))
    return out


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
    p = pair(12)
    one = ba.search_triangulation_pack([p])
    for _ in range(20):
        ba.search_triangulation_call(one)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    lat = timed(lambda: ba.search_triangulation_call(one), 200, 0.5)
    ba.close()
    h2d, d2h = arena_bytes([p])
    return dict(latency_one_pair_1000_1000_keypoints_us=dict(_stats(lat, 1e6), kernel_launches=int(launches), h2d_bytes=int(h2d), d2h_bytes=int(d2h),
                                                             distance_evaluations=evaluations(p), matches=int(one[2][0].get().n_matches)))


def step_keyframe(a):
    ba = backend.LocalBA(0)
    probs = [pair(200 + k) for k in range(20)]
    singles = [ba.search_triangulation_pack([p]) for p in probs]
    batch = ba.search_triangulation_pack(probs)

    def twenty():
        for s in singles:
            ba.search_triangulation_call(s)
    for _ in range(5):
        twenty(); ba.search_triangulation_call(batch)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    t20 = timed(twenty, 50, 0.5)
    t1 = timed(lambda: ba.search_triangulation_call(batch), 50, 0.5)
    ba.close()
    for s, b in zip(singles, batch[2]):
        assert s[2][0].get().match12.tobytes() == b.get().match12.tobytes()
    h2d, d2h = arena_bytes(probs)
    return dict(keyframe_20_pairs_us=dict(as_20_calls=_stats(t20, 1e6), as_one_call=dict(_stats(t1, 1e6), h2d_bytes=int(h2d), d2h_bytes=int(d2h))))


def step_batched(a):
    import search_tri_ref as ref
    ba = backend.LocalBA(0)
    probs = ragged(a.pairs)
    k1 = sum(p.n_keys1 for p in probs)
    batch = ba.search_triangulation_pack(probs)
    for _ in range(2):
        ba.search_triangulation_call(batch)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    tb = timed(lambda: ba.search_triangulation_call(batch), 5, 0.5)
    res = [b.get() for b in batch[2]]
    ba.close()
    k = min(4, len(probs))
    t0 = time.perf_counter()
    want = [ref.search_tri_ref(p) for p in probs[:k]]
    t_np = (time.perf_counter() - t0) / k
    for w, r in zip(want, res):
        assert np.array_equal(w["match12"], r.match12) and w["n_matches"] == r.n_matches
    h2d, d2h = arena_bytes(probs)
    ev = sum(evaluations(p) for p in probs)
    return dict(batched=dict(pairs=len(probs), keypoints_1=int(k1), distance_evaluations=int(ev), calls=int(len(tb)), median_ms=float(np.median(tb) * 1e3),
                             min_ms=float(tb.min() * 1e3), max_ms=float(tb.max() * 1e3), pairs_per_s=float(len(probs) / np.median(tb)),
                             kernel_launches=int(launches), h2d_bytes=int(h2d), d2h_bytes=int(d2h), matches=int(sum(r.n_matches for r in res))),
                numpy_yardstick=dict(what="tests/search_tri_ref.py in float64 on the host, per pair: NumPy, not a baseline", pairs=k,
                                     keypoints_1=int(sum(p.n_keys1 for p in probs[:k])), ms_per_pair=float(t_np * 1e3)))


def step_singles(a):
    ba = backend.LocalBA(0)
    probs = ragged(a.pairs)
    singles = [ba.search_triangulation_pack([p]) for p in probs]
    for s in singles[:20]:
        ba.search_triangulation_call(s)
    t0 = time.perf_counter()
    for s in singles:
        ba.search_triangulation_call(s)
    t_single = time.perf_counter() - t0
    ba.close()
    return dict(singles=dict(calls=len(probs), total_ms=float(t_single * 1e3), pairs_per_s=float(len(probs) / t_single)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_tri_bench.json"))
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), help="run one step in this process and print its JSON (what the parent starts)")
    a = ap.parse_args()
    steps = dict(latency=step_latency, keyframe=step_keyframe, batched=step_batched, singles=step_singles)
    if a.step:
        print("STEP " + json.dumps(steps[a.step](a)))
        return 0
    out = dict(what="vba_search_triangulation (k_search_tri): host clock around calls that end in the library's stream synchronise")
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
    k = out["keyframe_20_pairs_us"]
    out["keyframe_one_call_speedup_over_20_calls"] = k["as_20_calls"]["median"] / k["as_one_call"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
