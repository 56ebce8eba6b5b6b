"""Measures vba_fuse on the device and writes profiles/fuse_bench.json (fails without a device: there is no CPU path).

A batch shaped like LocalMapping::SearchInNeighbors of one keyframe: 30 problems of about 1 500 keypoints x 300 points (the current
keyframe's points into 30 targets) and one problem of 1 500 keypoints x 6 000 points (the targets' points into the current keyframe).

  one_call     the 31 problems in one vba_fuse call: median and p10-p90 of >= 50 calls (and >= 0.5 s of timed work)
  single_calls the same 31 problems as 31 calls, same process, same handle: what the facade's SearchInNeighbors does, because a
               Fuse call may change what the next one reads.  This feature's own baseline: the parent commit has nothing to compare with
  bytes        what the one call copies each way, from the record sizes

Host clock around LocalBA.fuse_call, which returns after the library's stream synchronise and includes the host's checks and
packing; building the ctypes views is outside the timed region.  The GPU work runs in a child process under a time limit; if it
fails or runs out of time nothing more is started.  Two sanity conditions are asserted: a call is one kernel launch, and the one
call returns bit for bit what the single calls return.  There is no pass mark.

usage: python scripts/fuse_bench.py [--out profiles/fuse_bench.json]
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

from mc_slam_amd import backend, synth  # noqa: E402

SIZEOF_DESC, SIZEOF_TILE, SIZEOF_KEY, SIZEOF_POINT = 304, 8, 64, 128      # FuDesc / FuTile / FuKey / FuPoint of mc_slam_amd/csrc/vba_layout.h
STEP_SECONDS = 300


def _up(b):
    return (b + 255) // 256 * 256


def arena_bytes(probs):
    """bytes of the one H2D and the one D2H copy of a call (the arena layout of vba_fuse)"""
    n, nk, npt = len(probs), sum(p.n_keys for p in probs), sum(p.n_pt for p in probs)
    nc, ft, lv = sum(len(p.cell_begin) for p in probs), sum(len(p.cell_feat) for p in probs), sum(2 * p.n_levels for p in probs)
    tiles = sum((p.n_pt + 255) // 256 for p in probs)
    h2d = (_up(SIZEOF_DESC * n) + _up(SIZEOF_TILE * (tiles + 1)) + _up(SIZEOF_KEY * (nk + 1)) + _up(SIZEOF_POINT * (npt + 1)) + _up(4 * (nc + 1)) +
           _up(4 * (ft + 1)) + _up(8 * (lv + 1)))
    d2h = _up(4 * (npt + 1)) + _up(2 * (npt + 1)) + _up(npt + 1) + _up(16 * (npt + 1)) + _up(npt + 1)
    return h2d, d2h, tiles


def problems():
    rng = np.random.default_rng(0)
    probs = [synth.fuse_scene(9000 + k, n_keys=int(rng.integers(1400, 1601)), n_pt=int(rng.integers(270, 331))) for k in range(30)]
    return probs + [synth.fuse_scene(9100, n_keys=1500, n_pt=6000)]


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
    ba = backend.LocalBA(0)
    probs = problems()
    singles = [ba.fuse_pack([p]) for p in probs]
    batch = ba.fuse_pack(probs)

    def each():
        for s in singles:
            ba.fuse_call(s)
    for _ in range(5):
        each(); ba.fuse_call(batch)
    launches = ba.get_profile()["kernel_launches"]
    assert launches == 1, launches
    t31 = timed(each, 50, 0.5)
    t1 = timed(lambda: ba.fuse_call(batch), 50, 0.5)
    ba.close()
    found = 0
    for s, b in zip(singles, batch[2]):
        x, y = s[2][0].get(), b.get()
        assert x.n_found == y.n_found
        for k in ("best_idx", "best_dist", "level", "uv", "state"):
            assert getattr(x, k).tobytes() == getattr(y, k).tobytes(), k
        found += y.n_found
    h2d, d2h, tiles = arena_bytes(probs)
    return dict(problems=len(probs), keypoints=int(sum(p.n_keys for p in probs)), points=int(sum(p.n_pt for p in probs)), tiles=int(tiles),
                found=int(found), kernel_launches=int(launches), h2d_bytes=int(h2d), d2h_bytes=int(d2h),
                one_call_us=_stats(t1, 1e6), single_calls_us=_stats(t31, 1e6), one_call_speedup_over_single_calls=float(np.median(t31) / np.median(t1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_bench.json"))
    ap.add_argument("--step", action="store_true", help="run the GPU work in this process and print its JSON (what the parent starts)")
    a = ap.parse_args()
    if a.step:
        print("STEP " + json.dumps(step()))
        return 0
    out = dict(what="vba_fuse (k_fuse): host clock around calls that end in the library's stream synchronise; a SearchInNeighbors-shaped batch")
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
