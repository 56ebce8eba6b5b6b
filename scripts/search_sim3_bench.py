"""Measures vba_search_by_sim3 on the device and writes profiles/search_sim3_bench.json (fails without a device: there is no CPU path).

Keyframe pairs of about 1 500 keypoints a side, of which about 400 carry a map point of a shared feature (some already matched,
some without a usable point on one side), as LoopClosing::ComputeSim3 hands them to ORBmatcher::SearchBySim3 after the RANSAC:

  one_pair      one pair per call: median and p10-p90 of >= 50 calls (and >= 0.5 s of timed work)
  five_one_call a ComputeSim3-shaped batch, the 5 candidates of one loop query, in ONE call
  five_calls    the same 5 pairs as 5 calls, same process, same handle, alternating with the one call.  This feature's own baseline:
                the parent commit has nothing to compare with
  ragged        a ragged batch of 3 000 pairs of 0 .. 160 keypoints a side in one call (the threaded packing path)
  numpy_one_pair_s  the NumPy yardstick (tests/search_sim3_ref.py, float64, sequential) on the one pair, LABELLED AS NUMPY: an
                interpreter loop, not the reference's C++; no CPU build of the reference's function exists here (it needs OpenCV),
                so no ratio against the reference is quoted
  bytes         what a call copies each way, from the record sizes

Host clock around LocalBA.search_by_sim3_call, which returns after the library's stream synchronise and includes the host's checks,
the compaction and packing and the agreement loop; building the ctypes views is outside the timed region.  The GPU work runs in a
child process under a time limit; if it fails or runs out of time nothing more is started.  Two sanity conditions are asserted: a
call is one kernel launch, and the one call returns bit for bit what the single calls return.  There is no pass mark.

usage: python scripts/search_sim3_bench.py [--out profiles/search_sim3_bench.json]
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

SIZEOF_DIR, SIZEOF_TILE, SIZEOF_KEY, SIZEOF_QUERY = 360, 16, 64, 96      # SsDir / SsTile / FuKey / SsQuery of mc_slam_amd/csrc/vba_layout.h
STEP_SECONDS = 400
ARRAYS = ("match1", "match2", "best_dist1", "best_dist2", "level1", "level2", "state1", "state2", "match12")


def _up(b):
    return (b + 255) // 256 * 256


def n_queries(kf):
    return int(((kf.has_pt != 0) & (kf.matched == 0)).sum())


def arena_bytes(probs):
    """bytes of the one H2D and the one D2H copy of a call (the arena layout of vba_search_by_sim3), tiles, queries"""
    kfs = [kf for p in probs for kf in (p.kf1, p.kf2)]
    n, nk, nq = len(probs), sum(kf.n_keys for kf in kfs), sum(n_queries(kf) for kf in kfs)
    nc, ft, lv = sum(len(kf.cell_begin) for kf in kfs), sum(len(kf.cell_feat) for kf in kfs), sum(kf.n_levels for kf in kfs)
    tiles = sum((n_queries(kf) + 255) // 256 for kf in kfs)
    h2d = (_up(SIZEOF_DIR * 2 * n) + _up(SIZEOF_TILE * (tiles + 1)) + _up(SIZEOF_KEY * (nk + 1)) + _up(SIZEOF_QUERY * (nq + 1)) + _up(4 * (nc + 1)) +
           _up(4 * (ft + 1)) + _up(8 * (lv + 1)))
    d2h = _up(4 * (nq + 1)) + _up(2 * (nq + 1)) + 2 * _up(nq + 1)
    return h2d, d2h, tiles, nq


def candidates():
    rng = np.random.default_rng(0)
    return [synth.sim3_search_scene(9200 + k, n_keys1=int(rng.integers(1400, 1601)), n_keys2=int(rng.integers(1400, 1601)), n_common=400, extra_points=0.0)
            for k in range(5)]


def ragged():
    rng = np.random.default_rng(1)
    return [synth.sim3_search_scene(9300 + k, n_keys1=int(rng.integers(0, 161)), n_keys2=int(rng.integers(0, 161)), n_common=int(rng.integers(0, 81)),
                                    grid=((16, 12), (16, 12))) for k in range(3000)]


def timed(fn, min_calls, min_seconds):
    ts = []
    while len(ts) < min_calls or sum(ts) < min_seconds:
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return np.array(ts)


def timed_alternating(fa, fb, min_calls, min_seconds):
    """fa and fb in turn, so that whatever else the host does meets both alike"""
    ta, tb = [], []
    while len(ta) < min_calls or sum(ta) + sum(tb) < 2 * min_seconds:
        for f, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
    return np.array(ta), np.array(tb)


def _stats(t, scale):
    return dict(calls=int(len(t)), median=float(np.median(t) * scale), p10=float(np.percentile(t, 10) * scale), p90=float(np.percentile(t, 90) * scale),
                min=float(t.min() * scale), max=float(t.max() * scale))


def _shape(probs):
    h2d, d2h, tiles, nq = arena_bytes(probs)
    return dict(pairs=len(probs), keypoints=int(sum(p.kf1.n_keys + p.kf2.n_keys for p in probs)), queries=int(nq), tiles=int(tiles), h2d_bytes=int(h2d),
                d2h_bytes=int(d2h))


def step():
    import search_sim3_ref
    ba = backend.LocalBA(0)
    five, many = candidates(), ragged()
    singles = [ba.search_by_sim3_pack([p]) for p in five]
    batch = ba.search_by_sim3_pack(five)
    big = ba.search_by_sim3_pack(many)

    def each():
        for s in singles:
            ba.search_by_sim3_call(s)
    for _ in range(5):
        each(); ba.search_by_sim3_call(batch); ba.search_by_sim3_call(big)
        launches = ba.get_profile()["kernel_launches"]
        assert launches == 1, launches
    t_one = timed(lambda: ba.search_by_sim3_call(singles[0]), 50, 0.5)
    t_batch, t_each = timed_alternating(lambda: ba.search_by_sim3_call(batch), each, 50, 0.5)
    t_big = timed(lambda: ba.search_by_sim3_call(big), 20, 0.5)
    ba.close()
    found = 0
    for s, b in zip(singles, batch[2]):
        x, y = s[2][0].get(), b.get()
        assert x.n_found == y.n_found
        for k in ARRAYS:
            assert getattr(x, k).tobytes() == getattr(y, k).tobytes(), k
        found += y.n_found
    t0 = time.perf_counter()
    w = search_sim3_ref.search_sim3_ref(five[0])
    t_numpy = time.perf_counter() - t0
    x = singles[0][2][0].get()
    assert x.n_found == w["n_found"] and all(np.array_equal(getattr(x, k), w[k]) for k in ARRAYS)
    return dict(kernel_launches=int(launches),
                one_pair=dict(_shape(five[:1]), found=int(x.n_found), call_us=_stats(t_one, 1e6)),
                five_candidates=dict(_shape(five), found=int(found), one_call_us=_stats(t_batch, 1e6), five_calls_us=_stats(t_each, 1e6),
                                     one_call_speedup_over_five_calls=float(np.median(t_each) / np.median(t_batch))),
                ragged=dict(_shape(many), found=int(sum(b.get().n_found for b in big[2])), one_call_us=_stats(t_big, 1e6)),
                numpy_one_pair_s=float(t_numpy))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_sim3_bench.json"))
    ap.add_argument("--step", action="store_true", help="run the GPU work in this process and print its JSON (what the parent starts)")
    a = ap.parse_args()
    if a.step:
        print("STEP " + json.dumps(step()))
        return 0
    out = dict(what="vba_search_by_sim3 (k_search_sim3): host clock around calls that end in the library's stream synchronise; ComputeSim3-shaped pairs; "
                    "numpy_one_pair_s is the NumPy yardstick, not the reference's C++")
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
