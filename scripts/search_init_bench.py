"""Measures vba_search_for_initialization on the device and writes profiles/search_init_bench.json (fails without a device: there is no
CPU path).

Frame pairs of 2 000 x 2 000 keypoints (640 x 480, the 64 x 48 grid), windowSize 100, ORBmatcher(0.9, true) as
Tracking::MonocularInitialization calls it:

  one_pair     ONE pair: median and p10-p90 of >= 50 calls (and >= 0.5 s of timed work).  One pair is one workgroup, and every query
               walks a 200 x 200 pixel window: `rounds` and the candidates per query are recorded so that a later change can judge
               whether the round-0 walk should be spread over tiles
  batch        16 pairs in one call, against the same 16 as 16 calls, same process, same handle.  This feature's own baseline: the
               parent commit has nothing to compare with, and the reference's function cannot be built here (it needs OpenCV)
  numpy        the NumPy yardstick (tests/search_init_ref.py, the sequential loop in Python) on the one pair, once: a NumPy time, NOT
               a baseline
  bytes        what the calls copy each way, from the record sizes

Host clock around LocalBA.search_for_initialization_call, which returns after the library's stream synchronise and includes the host's
checks, packing and the replay of the apply loop; building the ctypes views is outside the timed region.  The GPU work runs in a child
process under a time limit; if it fails or runs out of time nothing more is started.  Two sanity conditions are asserted: a call is
one kernel launch, and the batch returns bit for bit what the single calls return.  There is no pass mark.

usage: python scripts/search_init_bench.py [--out profiles/search_init_bench.json]
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

SIZEOF_DESC, SIZEOF_KEY, SIZEOF_QUERY = 128, 64, 64      # SiDesc / FuKey / SiQuery of mc_slam_amd/csrc/vba_layout.h
STEP_SECONDS = 300
FIELDS = ("match12", "best_idx", "best_dist", "best_dist2", "bin", "state", "prev_matched", "match21", "matched_dist", "hist", "ind")
N_KEYS, N_PAIRS = 2000, 16


def _up(b):
    return (b + 255) // 256 * 256


def arena_bytes(probs):
    """bytes of the one H2D and the one D2H copy of a call (the arena layout of vba_search_for_initialization)"""
    n, nk, nq = len(probs), sum(p.n_keys2 for p in probs), sum(p.n_q for p in probs)
    nc, ft = sum(len(p.cell_begin) for p in probs), sum(len(p.cell_feat) for p in probs)
    h2d = _up(SIZEOF_DESC * n) + _up(SIZEOF_KEY * (nk + 1)) + _up(SIZEOF_QUERY * (nq + 1)) + _up(4 * (nc + 1)) + _up(4 * (ft + 1))
    d2h = _up(4 * (n + 1)) + _up(4 * (nq + 1)) + 2 * _up(2 * (nq + 1)) + _up(nq + 1)
    return h2d, d2h


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
    import search_init_ref
    ba = backend.LocalBA(0)
    pairs = [synth.search_init_scene(9300 + k, n_keys1=N_KEYS, n_keys2=N_KEYS, window_size=100.0) for k in range(N_PAIRS)]
    singles = [ba.search_for_initialization_pack([p]) for p in pairs]
    batch = ba.search_for_initialization_pack(pairs)

    def each():
        for s in singles:
            ba.search_for_initialization_call(s)
    for _ in range(3):
        each(); ba.search_for_initialization_call(batch)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    t_one = timed(lambda: ba.search_for_initialization_call(singles[0]), 50, 0.5)
    t16 = timed(each, 20, 0.5)
    t1 = timed(lambda: ba.search_for_initialization_call(batch), 20, 0.5)
    ba.close()
    rounds, matches, stolen = [], 0, 0
    for s, b in zip(singles, batch[2]):
        x, y = s[2][0].get(), b.get()
        assert (x.n_matches, x.n_before_filter, x.n_stolen, x.rounds) == (y.n_matches, y.n_before_filter, y.n_stolen, y.rounds)
        for k in FIELDS:
            assert getattr(x, k).tobytes() == getattr(y, k).tobytes(), k
        rounds.append(int(y.rounds))
        matches += y.n_matches
        stolen += y.n_stolen
    got = singles[0][2][0].get()
    t0 = time.perf_counter()
    w = search_init_ref.search_init_ref(pairs[0])
    numpy_ms = (time.perf_counter() - t0) * 1e3
    assert w["n_matches"] == got.n_matches and np.array_equal(w["match12"], got.match12) and np.array_equal(w["match21"], got.match21)
    cand = w["n_cand"][pairs[0].oct1 == 0]
    h2d, d2h = arena_bytes(pairs)
    oh2d, od2h = arena_bytes(pairs[:1])
    return dict(kernel_launches=int(launches),
                one_pair=dict(keypoints1=pairs[0].n_keys1, keypoints2=pairs[0].n_keys2, queries=pairs[0].n_q, window_size=pairs[0].window_size,
                              matches=int(got.n_matches), stolen=int(got.n_stolen), rounds=int(got.rounds),
                              candidates_per_query=dict(mean=float(cand.mean()), median=float(np.median(cand)), max=int(cand.max()), total=int(cand.sum())),
                              h2d_bytes=int(oh2d), d2h_bytes=int(od2h), one_call_us=_stats(t_one, 1e6)),
                batch=dict(pairs=len(pairs), matches=int(matches), stolen=int(stolen), h2d_bytes=int(h2d), d2h_bytes=int(d2h), one_call_us=_stats(t1, 1e6),
                           single_calls_us=_stats(t16, 1e6), one_call_speedup_over_single_calls=float(np.median(t16) / np.median(t1)),
                           rounds=dict(per_pair=rounds, min=min(rounds), max=max(rounds), mean=float(np.mean(rounds)))),
                numpy_yardstick_ms=dict(one_pair=numpy_ms), numpy_note="the sequential loop in Python/NumPy, not a baseline")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_init_bench.json"))
    ap.add_argument("--step", action="store_true", help="run the GPU work in this process and print its JSON (what the parent starts)")
    a = ap.parse_args()
    if a.step:
        print("STEP " + json.dumps(step()))
        return 0
    out = dict(what="vba_search_for_initialization (k_search_init): host clock around calls that end in the library's stream synchronise; frame "
                    "pairs of 2 000 x 2 000 keypoints, windowSize 100; no figure of the parent commit or of the reference exists to compare with")
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
