"""Measures vba_search_by_bow on the device and writes profiles/search_bow_bench.json (fails without a device: there is no CPU path).

Pairs of about 1 500 keypoints a side over about 100 vocabulary nodes, as the callers of ORBmatcher::SearchByBoW hand them over:

  one_pair      one 1 500 x 1 500 pair per call (KF_FRAME mode, the call of TrackReferenceKeyFrame): median and p10-p90 of >= 50
                calls (and >= 0.5 s of timed work)
  five_candidates  the candidates of one LoopClosing::ComputeSim3 round (5 pairs, KF_KF mode) in ONE call, and the same 5 pairs as 5
                calls, same process, same handle, alternating with the one call.  This feature's own baseline: the parent commit has
                nothing to compare with
  relocalisation  10 keyframes against one frame (KF_FRAME mode), as one call and as 10 calls, alternating
  ragged        a ragged batch of 3 000 pairs of 0 .. 160 keypoints a side, both modes mixed, in one call (the threaded packing path)
  rounds        the rounds the conflict pass needed on every realistic pair, next to the largest number of queries in one node
  numpy_one_pair_s  the NumPy yardstick (tests/search_bow_ref.py, sequential) on the one pair, LABELLED AS NUMPY: an interpreter loop,
                not the reference's C++; no CPU build of the reference's function exists here (it needs OpenCV and DBoW2), so no
                ratio against the reference is quoted
  bytes         what a call copies each way, from the record sizes

Host clock around LocalBA.search_by_bow_call, which returns after the library's stream synchronise and includes the host's checks,
the node join, the packing and the write-back with histogram, maxima and drop; building the ctypes views is outside the timed region.
The GPU work runs in a child process under a time limit; if it fails or runs out of time nothing more is started.  Two sanity
conditions are asserted: a call is one kernel launch, and the one call returns bit for bit what the single calls return.  There is no
pass mark.

usage: python scripts/search_bow_bench.py [--out profiles/search_bow_bench.json]
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

from mc_slam_amd import abi, backend, synth  # noqa: E402

SIZEOF_DESC, SIZEOF_KEY, SIZEOF_QUERY = 48, 32, 16      # SbDesc / SbKey / SbQuery of mc_slam_amd/csrc/vba_layout.h
STEP_SECONDS = 400
ARRAYS = ("match12", "best_idx", "best_dist", "best_dist2", "bin", "state", "match21", "hist", "ind")
KF_FRAME, KF_KF = abi.SEARCH_BOW_KF_FRAME, abi.SEARCH_BOW_KF_KF


def _up(b):
    return (b + 255) // 256 * 256


def arena_bytes(probs):
    """bytes of the one H2D and the one D2H copy of a call (the arena layout of vba_search_by_bow)"""
    n, k1, k2 = len(probs), sum(p.n_keys1 for p in probs), sum(p.n_keys2 for p in probs)
    ft = sum(len(p.node_feat2) for p in probs)
    h2d = _up(SIZEOF_DESC * n) + _up(SIZEOF_KEY * (k1 + 1)) + _up(SIZEOF_KEY * (k2 + 1)) + _up(k1 + 1) + _up(k2 + 1) + _up(SIZEOF_QUERY * (k1 + 1)) + _up(4 * (ft + 1))
    d2h = _up(4 * (n + 1)) + _up(4 * (k1 + 1)) + 2 * _up(2 * (k1 + 1)) + _up(k1 + 1)
    return h2d, d2h


def scene(seed, mode, rng):
    return synth.search_bow_scene(seed, mode, n_keys1=int(rng.integers(1400, 1601)), n_keys2=int(rng.integers(1400, 1601)), n_nodes=100)


def loop_candidates():
    rng = np.random.default_rng(0)
    return [scene(9400 + k, KF_KF, rng) for k in range(5)]


def relocalisation():
    """10 keyframes against ONE frame: side 2 of every pair is the frame of the first, so only the first keyframe has twins there"""
    rng = np.random.default_rng(2)
    ps = [scene(9500 + k, KF_FRAME, rng) for k in range(10)]
    f = ps[0]
    return [p.copy(desc2=f.desc2, angle2=f.angle2, node_id2=f.node_id2, node_begin2=f.node_begin2, node_feat2=f.node_feat2) for p in ps]


def ragged():
    rng = np.random.default_rng(1)
    return [synth.search_bow_scene(9600 + k, k % 2, n_keys1=int(rng.integers(0, 161)), n_keys2=int(rng.integers(0, 161)), n_nodes=int(rng.integers(1, 13)))
            for k in range(3000)]


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
    h2d, d2h = arena_bytes(probs)
    return dict(pairs=len(probs), keypoints=int(sum(p.n_keys1 + p.n_keys2 for p in probs)), h2d_bytes=int(h2d), d2h_bytes=int(d2h))


def step():
    import search_bow_ref
    ba = backend.LocalBA(0)
    rng = np.random.default_rng(3)
    one = [scene(9300, KF_FRAME, rng)]
    five, ten, many = loop_candidates(), relocalisation(), ragged()
    out = dict()

    def same(singles, batch):
        n = 0
        for s, b in zip(singles, batch[2]):
            x, y = s[2][0].get(), b.get()
            assert (x.n_matches, x.n_before_filter, x.rounds) == (y.n_matches, y.n_before_filter, y.rounds)
            for k in ARRAYS:
                assert getattr(x, k).tobytes() == getattr(y, k).tobytes(), k
            n += y.n_matches
        return n

    def one_against_many(probs):
        singles = [ba.search_by_bow_pack([p]) for p in probs]
        batch = ba.search_by_bow_pack(probs)

        def each():
            for s in singles:
                ba.search_by_bow_call(s)
        for _ in range(5):
            each(); ba.search_by_bow_call(batch)
            assert ba.get_profile()["kernel_launches"] == 1
        t_batch, t_each = timed_alternating(lambda: ba.search_by_bow_call(batch), each, 50, 0.5)
        matches = same(singles, batch)
        rounds = [[int(b.get().rounds), int(search_bow_ref.queries(p)[1])] for p, b in zip(probs, batch[2])]
        return dict(_shape(probs), matches=int(matches), one_call_us=_stats(t_batch, 1e6), single_calls_us=_stats(t_each, 1e6),
                    one_call_speedup_over_single_calls=float(np.median(t_each) / np.median(t_batch)), rounds_and_largest_node=rounds)

    single = ba.search_by_bow_pack(one)
    for _ in range(5):
        ba.search_by_bow_call(single)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    t_one = timed(lambda: ba.search_by_bow_call(single), 50, 0.5)
    x = single[2][0].get()
    out["one_pair"] = dict(_shape(one), matches=int(x.n_matches), rounds_and_largest_node=[int(x.rounds), int(search_bow_ref.queries(one[0])[1])],
                           call_us=_stats(t_one, 1e6))
    out["five_candidates"] = one_against_many(five)
    out["relocalisation"] = one_against_many(ten)
    big = ba.search_by_bow_pack(many)
    for _ in range(3):
        ba.search_by_bow_call(big)
    assert ba.get_profile()["kernel_launches"] == 1
    t_big = timed(lambda: ba.search_by_bow_call(big), 20, 0.5)
    out["ragged"] = dict(_shape(many), matches=int(sum(b.get().n_matches for b in big[2])), max_rounds=int(max(b.get().rounds for b in big[2])),
                         one_call_us=_stats(t_big, 1e6))
    ba.close()
    t0 = time.perf_counter()
    w = search_bow_ref.search_bow_ref(one[0])
    out["numpy_one_pair_s"] = float(time.perf_counter() - t0)
    assert x.n_matches == w["n_matches"] and all(np.array_equal(getattr(x, k), w[k]) for k in ARRAYS)
    out["kernel_launches"] = int(launches)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_bow_bench.json"))
    ap.add_argument("--step", action="store_true", help="run the GPU work in this process and print its JSON (what the parent starts)")
    a = ap.parse_args()
    if a.step:
        print("STEP " + json.dumps(step()))
        return 0
    out = dict(what="vba_search_by_bow (k_search_bow): host clock around calls that end in the library's stream synchronise; pairs of about 1 500 keypoints "
                    "a side over 100 nodes; numpy_one_pair_s is the NumPy yardstick, not the reference's C++")
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
