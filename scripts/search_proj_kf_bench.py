"""Measures vba_search_by_projection_kf on the device and writes profiles/search_proj_kf_bench.json (fails without a device: there is no
CPU path).

Targets of 1 500 keypoints (640 x 480, the 64 x 48 grid), a tenth of them occupied:

  loop         ONE loop problem of 8 000 map points with th = 10, th_dist = 50 (the call of LoopClosing::ComputeSim3): median and
               p10-p90 of >= 50 calls (and >= 0.5 s of timed work).  One problem is one workgroup: this figure is recorded so that a
               later change can judge whether the gate phase should be spread over tiles
  reloc        ONE reloc problem of 1 500 queries, 70 % of them with a map point, at (th, ORBdist) = (10, 100)
  candidates   five reloc candidates in one call, against the same five as five calls, same process, same handle.  This feature's
               own baseline: the parent commit has nothing to compare with
  rounds       the rounds of the conflict pass of every problem
  numpy        the NumPy yardstick (tests/search_proj_kf_ref.py, the sequential loop in Python) on the loop and on one reloc problem,
               once: a NumPy time, NOT a baseline -- no CPU build of the reference's functions exists here
  bytes        what the five-candidate call copies each way, from the record sizes

Host clock around LocalBA.search_by_projection_kf_call, which returns after the library's stream synchronise and includes the host's
checks, packing and the replay of the apply loop; building the ctypes views is outside the timed region.  The GPU work runs in a child
process under a time limit; if it fails or runs out of time nothing more is started.  Two sanity conditions are asserted: a call is
one kernel launch, and the batch returns bit for bit what the single calls return.  There is no pass mark.

usage: python scripts/search_proj_kf_bench.py [--out profiles/search_proj_kf_bench.json]
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
FIELDS = ("best_idx", "best_dist", "level", "uv", "bin", "state", "key_match", "hist", "ind")
LOOP, RELOC = abi.SEARCH_PROJ_KF_LOOP, abi.SEARCH_PROJ_KF_RELOC


def _up(b):
    return (b + 255) // 256 * 256


def arena_bytes(probs):
    """bytes of the one H2D and the one D2H copy of a call (the arena layout of vba_search_by_projection_kf)"""
    n, nk, nq = len(probs), sum(p.n_keys for p in probs), sum(p.n_q for p in probs)
    nc, ft, lv = sum(len(p.cell_begin) for p in probs), sum(len(p.cell_feat) for p in probs), sum(p.n_levels for p in probs)
    h2d = _up(SIZEOF_DESC * n) + _up(SIZEOF_KEY * (nk + 1)) + _up(nk + 1) + _up(SIZEOF_QUERY * (nq + 1)) + _up(4 * (nc + 1)) + _up(4 * (ft + 1)) + _up(8 * (lv + 1))
    d2h = _up(4 * (n + 1)) + _up(4 * (nq + 1)) + _up(2 * (nq + 1)) + 2 * _up(nq + 1) + _up(16 * (nq + 1))
    return h2d, d2h


def loop_problem(seed):
    return synth.search_proj_kf_scene(seed, LOOP, n_keys=1500, n_q=8000, th=10.0)


def reloc_problem(seed):
    """70 % of the source keyframe's keypoints hold a map point: the others are skipped"""
    p = synth.search_proj_kf_scene(seed, RELOC, n_keys=1500, n_q=1500, th=10.0, th_dist=100)
    none = np.random.default_rng(seed).random(p.n_q) >= 0.7
    return p.copy(q_skip=(p.q_skip.astype(bool) | none).astype(np.uint8))


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
    import search_proj_kf_ref
    ba = backend.LocalBA(0)
    loop = loop_problem(9100)
    cands = [reloc_problem(9200 + k) for k in range(5)]
    loop_pack = ba.search_by_projection_kf_pack([loop])
    singles = [ba.search_by_projection_kf_pack([p]) for p in cands]
    batch = ba.search_by_projection_kf_pack(cands)

    def each():
        for s in singles:
            ba.search_by_projection_kf_call(s)
    for _ in range(5):
        each(); ba.search_by_projection_kf_call(batch); ba.search_by_projection_kf_call(loop_pack)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    t_loop = timed(lambda: ba.search_by_projection_kf_call(loop_pack), 50, 0.5)
    t_reloc = timed(lambda: ba.search_by_projection_kf_call(singles[0]), 50, 0.5)
    t5 = timed(each, 50, 0.5)
    t1 = timed(lambda: ba.search_by_projection_kf_call(batch), 50, 0.5)
    ba.close()
    rounds, matches = [], 0
    for s, b in zip(singles, batch[2]):
        x, y = s[2][0].get(), b.get()
        assert (x.n_matches, x.n_before_filter, x.rounds) == (y.n_matches, y.n_before_filter, y.rounds)
        for k in FIELDS:
            assert getattr(x, k).tobytes() == getattr(y, k).tobytes(), k
        rounds.append(int(y.rounds))
        matches += y.n_matches
    lr = loop_pack[2][0].get()
    numpy_ms = {}
    for name, p, got in (("loop", loop, lr), ("reloc", cands[0], batch[2][0].get())):
        t0 = time.perf_counter()
        w = search_proj_kf_ref.search_proj_kf_ref(p)
        numpy_ms[name] = (time.perf_counter() - t0) * 1e3
        assert w["n_matches"] == got.n_matches and np.array_equal(w["key_match"], got.key_match)
    h2d, d2h = arena_bytes(cands)
    lh2d, ld2h = arena_bytes([loop])
    return dict(kernel_launches=int(launches),
                loop=dict(keypoints=loop.n_keys, queries=loop.n_q, th=loop.th, th_dist=loop.th_dist, matches=int(lr.n_matches), rounds=int(lr.rounds),
                          h2d_bytes=int(lh2d), d2h_bytes=int(ld2h), one_call_us=_stats(t_loop, 1e6)),
                reloc=dict(keypoints=cands[0].n_keys, queries=cands[0].n_q, with_map_point=int((cands[0].q_skip == 0).sum()), th=cands[0].th,
                           th_dist=cands[0].th_dist, one_call_us=_stats(t_reloc, 1e6)),
                candidates=dict(problems=len(cands), matches=int(matches), h2d_bytes=int(h2d), d2h_bytes=int(d2h), one_call_us=_stats(t1, 1e6),
                                single_calls_us=_stats(t5, 1e6), one_call_speedup_over_single_calls=float(np.median(t5) / np.median(t1)),
                                rounds=dict(per_problem=rounds, min=min(rounds), max=max(rounds), mean=float(np.mean(rounds)))),
                numpy_yardstick_ms=numpy_ms, numpy_note="the sequential loop in Python/NumPy, not a baseline")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_proj_kf_bench.json"))
    ap.add_argument("--step", action="store_true", help="run the GPU work in this process and print its JSON (what the parent starts)")
    a = ap.parse_args()
    if a.step:
        print("STEP " + json.dumps(step()))
        return 0
    out = dict(what="vba_search_by_projection_kf (k_search_proj_kf): host clock around calls that end in the library's stream synchronise; targets "
                    "of 1 500 keypoints; one loop problem of 8 000 points, reloc problems of 1 500 queries")
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
