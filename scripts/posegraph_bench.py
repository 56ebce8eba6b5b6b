"""Measures vba_posegraph_optimize on the device and writes profiles/posegraph_bench.json (fails without a device: there is no CPU
path).

  one_graph    one 500-vertex graph (span 6, one loop of 8 edges, 2 000 map points) per call: median and spread
  batched      one call with 64 ragged graphs of 100-1 000 vertices
  singles      the same 64 graphs as 64 calls, same process, same handle
  numpy        the NumPy yardstick (tests/posegraph_ref.py) on the 500-vertex graph, on this host: NOT a baseline -- a vectorised
               restatement with a dense solve; no compiled CPU implementation of this function exists here to measure against

Host clock around LocalBA.posegraph_call, which returns after the library's stream synchronise; building the ctypes views and
putting the initial estimates back between calls are outside the timed region.

usage: python scripts/posegraph_bench.py [--graphs 64] [--out profiles/posegraph_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mc_slam_amd import backend, synth  # noqa: E402


def timed(setup, fn, min_calls, min_seconds):
    ts = []
    while len(ts) < min_calls or sum(ts) < min_seconds:
        setup()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return np.array(ts)


def spread(ts, unit):
    return dict(calls=int(len(ts)), median=float(np.median(ts) * unit), p10=float(np.percentile(ts, 10) * unit),
                p90=float(np.percentile(ts, 90) * unit), min=float(ts.min() * unit), max=float(ts.max() * unit))


def loop_graph(seed, n, n_pt=0):
    return synth.make_posegraph(seed, n, span=6, loops=[(n - 1 - k, k) for k in range(8)], fixed_at=0, n_pt=n_pt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_bench.json"))
    a = ap.parse_args()
    ba = backend.LocalBA(0)
    rng = np.random.default_rng(0)

    g500 = loop_graph(500, 500, n_pt=2000)
    one = ba.posegraph_pack([g500])
    for _ in range(3):
        ba.posegraph_reset(one); ba.posegraph_call(one)
    assert ba.get_profile()["kernel_launches"] == 2
    r500 = one[2][0]
    one_info = dict(its_done=int(r500.its_done), lm_trials=int(r500.lm_trials), stop=int(r500.stop), chi2_initial=float(r500.chi2_initial),
                    chi2_final=float(r500.chi2_final), edges=int(g500.n_edges))
    lat = timed(lambda: ba.posegraph_reset(one), lambda: ba.posegraph_call(one), 20, 0.5)

    sizes = [int(rng.integers(100, 1001)) for _ in range(a.graphs)]
    graphs = [loop_graph(2000 + k, n) for k, n in enumerate(sizes)]
    batch = ba.posegraph_pack(graphs)
    for _ in range(2):
        ba.posegraph_reset(batch); ba.posegraph_call(batch)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    tb = timed(lambda: ba.posegraph_reset(batch), lambda: ba.posegraph_call(batch), 5, 0.5)
    want = [q.S.tobytes() for q in batch[6]]

    singles = [ba.posegraph_pack([g]) for g in graphs]
    for s in singles[:4]:
        ba.posegraph_call(s); ba.posegraph_reset(s)
    t0 = time.perf_counter()
    for s in singles:
        ba.posegraph_call(s)
    t_single = time.perf_counter() - t0
    assert all(s[6][0].S.tobytes() == w for s, w in zip(singles, want)), "single calls and the batched call disagree"

    import posegraph_ref
    t0 = time.perf_counter()
    rr = posegraph_ref.optimize(g500)
    t_numpy = time.perf_counter() - t0

    out = dict(
        what="vba_posegraph_optimize (k_posegraph_opt, k_posegraph_points): host clock around calls that end in the library's stream synchronise",
        one_graph_500_vertices_ms=dict(spread(lat, 1e3), **one_info),
        batched=dict(graphs=len(graphs), vertices=int(sum(sizes)), edges=int(sum(g.n_edges for g in graphs)), kernel_launches=int(launches),
                     its_done_mean=float(np.mean([r.its_done for r in batch[2]])), lm_trials_mean=float(np.mean([r.lm_trials for r in batch[2]])),
                     **{k + "_ms": v for k, v in spread(tb, 1e3).items() if k != "calls"}, calls=int(len(tb))),
        singles=dict(calls=len(graphs), total_ms=float(t_single * 1e3)),
        batched_speedup_over_singles=float(t_single / np.median(tb)),
        numpy_yardstick_500_vertices_s=dict(seconds=float(t_numpy), its_done=int(rr.its_done), lm_trials=int(rr.lm_trials),
                                            note="NumPy restatement with a dense solve, on the host of this run: not a baseline"),
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    ba.close()


if __name__ == "__main__":
    main()
