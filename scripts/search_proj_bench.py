"""Measures vba_search_by_projection on the device and writes profiles/search_proj_bench.json (fails without a device: there is no CPU
path).

Frames of 1 500 keypoints (640 x 480, the 64 x 48 grid): a last-frame problem has 1 000 queries with th = 15, a local-map problem 1 500
queries with th = 1; a tenth of the keypoints is occupied, a tenth of the queries does not block.

  one_frame    one frame per call, per mode: median and p10-p90 of >= 50 calls (and >= 0.5 s of timed work)
  batch        16 frames (8 per mode) in one call, against the same frames as 16 single calls, same process, same handle.  This
               feature's own baseline: the parent commit has nothing to compare with
  rounds       the rounds of the conflict pass over the 16 frames
  numpy        the NumPy yardstick (tests/search_proj_ref.py, the sequential loop in Python) on one frame per mode, once: a NumPy
               time, NOT a baseline -- no CPU build of the reference's functions exists here
  bytes        what the batch call copies each way, from the record sizes

Host clock around LocalBA.search_by_projection_call, which returns after the library's stream synchronise and includes the host's
checks, packing and the replay of the apply loop; building the ctypes views is outside the timed region.  The GPU work runs in a child
process under a time limit; if it fails or runs out of time nothing more is started.  Two sanity conditions are asserted: a call is
one kernel launch, and the batch returns bit for bit what the single calls return.  There is no pass mark.

usage: python scripts/search_proj_bench.py [--out profiles/search_proj_bench.json]
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

SIZEOF_DESC, SIZEOF_KEY, SIZEOF_QUERY = 304, 64, 112      # SpDesc / FuKey / SpQuery of mc_slam_amd/csrc/vba_layout.h
STEP_SECONDS = 300
FIELDS = ("best_idx", "best_dist", "best_dist2", "level", "view_cos", "uv", "bin", "state", "key_match", "hist", "ind")


def _up(b):
    return (b + 255) // 256 * 256


def arena_bytes(probs):
    """bytes of the one H2D and the one D2H copy of a call (the arena layout of vba_search_by_projection)"""
    n, nk, nq = len(probs), sum(p.n_keys for p in probs), sum(p.n_q for p in probs)
    nc, ft, lv = sum(len(p.cell_begin) for p in probs), sum(len(p.cell_feat) for p in probs), sum(p.n_levels for p in probs)
    h2d = _up(SIZEOF_DESC * n) + _up(SIZEOF_KEY * (nk + 1)) + _up(nk + 1) + _up(SIZEOF_QUERY * (nq + 1)) + _up(4 * (nc + 1)) + _up(4 * (ft + 1)) + _up(8 * (lv + 1))
    d2h = _up(4 * (n + 1)) + _up(4 * (nq + 1)) + 2 * _up(2 * (nq + 1)) + 2 * _up(nq + 1) + _up(8 * (nq + 1)) + _up(16 * (nq + 1))
    return h2d, d2h


def frame(seed, mode):
    return synth.search_proj_scene(seed, mode, n_keys=1500, n_q=1000 if mode == abi.SEARCH_PROJ_LAST_FRAME else 1500)


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
    import search_proj_ref
    ba = backend.LocalBA(0)
    probs = [frame(9000 + k, k % 2) for k in range(16)]
    singles = [ba.search_by_projection_pack([p]) for p in probs]
    batch = ba.search_by_projection_pack(probs)

    def each():
        for s in singles:
            ba.search_by_projection_call(s)
    for _ in range(5):
        each(); ba.search_by_projection_call(batch)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    one = {name: _stats(timed(lambda: ba.search_by_projection_call(singles[k]), 50, 0.5), 1e6) for k, name in ((0, "last_frame"), (1, "local_map"))}
    t16 = timed(each, 50, 0.5)
    t1 = timed(lambda: ba.search_by_projection_call(batch), 50, 0.5)
    ba.close()
    rounds, matches = [], 0
    for s, b in zip(singles, batch[2]):
        x, y = s[2][0].get(), b.get()
        assert (x.n_matches, x.n_before_filter, x.rounds) == (y.n_matches, y.n_before_filter, y.rounds)
        for k in FIELDS:
            assert getattr(x, k).tobytes() == getattr(y, k).tobytes(), k
        rounds.append(int(y.rounds))
        matches += y.n_matches
    numpy_ms = {}
    for k, name in ((0, "last_frame"), (1, "local_map")):
        t0 = time.perf_counter()
        w = search_proj_ref.search_proj_ref(probs[k])
        numpy_ms[name] = (time.perf_counter() - t0) * 1e3
        assert w["n_matches"] == batch[2][k].get().n_matches
    h2d, d2h = arena_bytes(probs)
    return dict(frames=len(probs), keypoints=int(sum(p.n_keys for p in probs)), queries=int(sum(p.n_q for p in probs)), matches=int(matches),
                kernel_launches=int(launches), h2d_bytes=int(h2d), d2h_bytes=int(d2h), one_frame_us=one, batch_one_call_us=_stats(t1, 1e6),
                batch_single_calls_us=_stats(t16, 1e6), one_call_speedup_over_single_calls=float(np.median(t16) / np.median(t1)),
                rounds=dict(per_frame=rounds, min=min(rounds), max=max(rounds), mean=float(np.mean(rounds))),
                numpy_yardstick_ms_one_frame=numpy_ms, numpy_note="the sequential loop in Python/NumPy, not a baseline")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_proj_bench.json"))
    ap.add_argument("--step", action="store_true", help="run the GPU work in this process and print its JSON (what the parent starts)")
    a = ap.parse_args()
    if a.step:
        print("STEP " + json.dumps(step()))
        return 0
    out = dict(what="vba_search_by_projection (k_search_proj): host clock around calls that end in the library's stream synchronise; frames of "
                    "1 500 keypoints, 1 000 (last frame) or 1 500 (local map) queries")
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
