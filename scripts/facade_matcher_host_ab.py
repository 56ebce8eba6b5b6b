#!/usr/bin/env python3
"""The matcher facade on the CPU, an earlier revision against the working tree, through tests/host_facade_matcher_check.cpp (the facade
source with stubs in place of the library; no GPU, no library).

  --record REV    build the harness under ASan + UBSan against mc_slam_amd/host/ORBmatcher.cpp of REV and write both of its modes to
                  tests/golden/facade_matcher_lines.txt (what tests/test_host_facade_matcher.py compares with)
  --ab REV        build the harness with -O2 against REV and against the working tree, run `time` mode (2000 keypoints per target, a
                  64 x 48 grid, 1000 queries; per run the median over --reps fresh scenes of each call's time) ten times each,
                  alternating, and write both tables with the median, p10 and p90 per call to profiles/facade_matcher_host_ab.json.
                  A second binary of REV alternates with them as a control: how often the parent leaves its own band
"""
import argparse
import json
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "host_facade_matcher_check.cpp")


def checkout(rev, tmp):
    """mc_slam_amd/host and include of rev under tmp: the path of its ORBmatcher.cpp"""
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "mc_slam_amd/host", "include"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
    return os.path.join(tmp, "mc_slam_amd", "host", "ORBmatcher.cpp")


def build(exe, flags, source=None):
    define = ['-DFACADE_MATCHER_CPP="%s"' % source] if source else []
    subprocess.check_call(["g++", "-std=c++17"] + flags + define + ["-I", os.path.join(ROOT, "include"), HARNESS, "-o", exe])
    return exe


def times(exe, reps):
    out = subprocess.run([exe, "time", str(reps)], check=True, capture_output=True, text=True).stdout
    return {l.split(None, 2)[2]: int(l.split()[1]) for l in out.splitlines() if l.startswith("time ")}


def table(runs):
    return {call: {"runs_ns": [r[call] for r in runs], "median_ns": float(np.median([r[call] for r in runs])),
                   "p10_ns": float(np.percentile([r[call] for r in runs], 10)), "p90_ns": float(np.percentile([r[call] for r in runs], 90))}
            for call in runs[0]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--record", metavar="REV")
    ap.add_argument("--ab", metavar="REV")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=31)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        if args.record:
            exe = build(os.path.join(tmp, "record"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                      "-fno-omit-frame-pointer"], checkout(args.record, tmp))
            env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
            with open(os.path.join(ROOT, "tests", "golden", "facade_matcher_lines.txt"), "w") as f:
                for title, mode in (("main mode", []), ("refuse mode", ["refuse"])):
                    f.write("# %s\n%s" % (title, subprocess.run([exe] + mode, check=True, capture_output=True, text=True, env=env).stdout))
        if args.ab:
            parent = build(os.path.join(tmp, "parent"), ["-O2"], checkout(args.ab, tmp))
            control = build(os.path.join(tmp, "control"), ["-O2"], checkout(args.ab, tmp))
            new = build(os.path.join(tmp, "new"), ["-O2"])
            runs = {"parent": [], "new": [], "control": []}
            for _ in range(args.runs):
                runs["parent"].append(times(parent, args.reps))
                runs["new"].append(times(new, args.reps))
                runs["control"].append(times(control, args.reps))
            res = {"scene": "2000 keypoints per target, 64 x 48 grid, 1000 queries, stubs in place of the library", "build": "g++ -O2",
                   "per_run": "median over %d fresh scenes of one call's time" % args.reps, "runs": args.runs,
                   "order": "parent, new, control (the parent's source once more) alternating",
                   "parent_rev": subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", args.ab], check=True, capture_output=True, text=True).stdout.strip(),
                   "parent": table(runs["parent"]), "new": table(runs["new"]), "control": table(runs["control"])}
            for arm in ("new", "control"):
                res[arm + "_median_inside_parent_p10_p90"] = {c: res["parent"][c]["p10_ns"] <= res[arm][c]["median_ns"] <= res["parent"][c]["p90_ns"]
                                                              for c in res["parent"]}
            with open(os.path.join(ROOT, "profiles", "facade_matcher_host_ab.json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
            for c in res["parent"]:
                print("%-45s parent %9.0f [%9.0f, %9.0f]  new %9.0f %-7s  control %9.0f %s" % (
                    c, res["parent"][c]["median_ns"], res["parent"][c]["p10_ns"], res["parent"][c]["p90_ns"], res["new"][c]["median_ns"],
                    "inside" if res["new_median_inside_parent_p10_p90"][c] else "OUTSIDE", res["control"][c]["median_ns"],
                    "inside" if res["control_median_inside_parent_p10_p90"][c] else "OUTSIDE"))


if __name__ == "__main__":
    main()
