#!/usr/bin/env python3
"""bench.py -- LocalBA windows/sec on MI355X (BASELINE.json metric).

A "step" is one pass of the hot path (the whole two-stage LocalBAPRVIDP solve, src/Optimizer.cpp:458-517 of the
reference) over one BATCH of synthetic windows per GPU.  Workload at every N: BASELINE.json configs[2] (LocalBAPRVIDP
window: 50 KF / 5 000 inverse-depth landmarks / 30 000 EdgePRIDP + PRV + bias edges, Gauss-Newton 5+10), `--batch` windows
per GPU built from `--distinct` seeded windows whose sizes are drawn AROUND that configuration (40..60 keyframes, mean 50;
`--uniform` = every window exactly 50 / 5 000 / 30 000).

A plain run measures the headline figure only: it sets up, warms up, times `--steps` steps and prints the line.
  value             windows/s with the inputs already resident in HBM when the clock starts (vba_batch_upload before,
                    K x vba_batch_run timed) -- the bench contract's `value`; `ms_per_step` = one timed step.
`--full` adds, on the same batch, everything else the benchmark measures and checks:
  verified          replicas agree bit for bit, the distinct windows match the CPU oracle;
  value_end_to_end  windows/s of FRESH windows: host arrays in, solved host arrays out (vba_batch_solve = H2D + structure
                    build + solve + D2H, chunks of the batch in flight concurrently) -- SURVEY 8(d) "copies included";
  single_window_ms  median latency of one vba_solve (upload + solve + download of ONE window, the way LocalMapping calls
                    the reference) beside the 1-core CPU oracle on the same window;
  roofline          dominant kernel class, HIP events on the backend's own stream, in a profiled run of its own;
  cpu_baseline      the CPU oracle = restatement of the reference's g2o path, 1 core, bounded sample; PCG (c4 / gba).
`--dump-outputs DIR` writes what the last timed step handed back to its caller as DIR/<name>.npy (dump_outputs below).
Weak scaling: every rank solves its own batch, no data-path collective (windows are independent);
torch.distributed (RCCL) only carries the barrier and the max-over-ranks time.  `--gpus N` without torchrun starts the N
ranks itself (mc_slam_amd/launch.py); under torchrun every process is a rank already.  One JSON line on rank 0.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def csrc_sha():
    """hash of the kernel sources: a PMC traffic profile only describes the kernels it was taken from"""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "mc_slam_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".h", ".hip")):
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def _gen_window(spec):
    """(workload, seed, uniform, landmark order) -> Problem; runs in forked worker processes (numpy only, no GPU, no torch)"""
    from mc_slam_amd import synth
    wl, seed, uniform, order = spec[:4]
    mix = spec[4] if len(spec) > 4 else "r3"
    if wl == "c3":
        return synth.config_c3(seed=seed, landmark_order=order) if uniform else synth.config_c3_ragged(seed=seed, landmark_order=order, kinds=(mix != "r2"))
    if wl in ("c4", "c3s", "c2", "c2s"):   # local windows: the order the caller hands landmarks over in matters to the record layout
        return {"c4": synth.config_c4, "c3s": synth.config_c3s, "c2": synth.config_c2, "c2s": synth.config_c2s}[wl](seed=seed, landmark_order=order)
    return synth.config_gba(seed=seed)   # (the global BA walks pMap->GetAllMapPoints(): no keyframe grouping)


def make_windows(specs, n_proc):
    if n_proc <= 1 or len(specs) < 4:
        return [_gen_window(s) for s in specs]
    import multiprocessing as mp
    with mp.get_context("fork").Pool(min(n_proc, len(specs))) as pool:   # forked BEFORE anything touches the GPU
        return pool.map(_gen_window, specs, chunksize=1)


def dump_outputs(out_dir, items, cap=56 << 20):
    """items: one {name: array} per window (or frame) of the batch, what the timed call handed back for it.  Writes
    out_dir/<name>.npy, every name concatenated over a fixed sample of the items -- all of them when they fit in `cap` bytes,
    else items drawn in a seeded random order while they fit, kept in batch order -- and out_dir/sample.npy, the indices of
    the items written.  Flags are written as float32, everything else as float64."""
    import numpy as np
    conv = [{k: np.asarray(v, dtype=np.float32 if np.asarray(v).dtype in (np.uint8, np.bool_) else np.float64).ravel()
             for k, v in it.items() if v is not None} for it in items]
    pick, size = [], 0
    for i in np.random.default_rng(0).permutation(len(conv)):
        b = sum(a.nbytes for a in conv[i].values())
        if size + b > cap:
            break
        pick.append(int(i))
        size += b
    pick.sort()
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "sample.npy"), np.array(pick, dtype=np.float64))
    for k in conv[0]:
        np.save(os.path.join(out_dir, k + ".npy"), np.concatenate([conv[i][k] for i in pick]))


def finish(dist, rank, out):
    """end of a run: the ranks leave together, rank 0 prints the line"""
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out))


def bench_pose(args, rank, local_rank, world, dist, torch):
    """Extra measurement: frames/s of vba_pose_optimize on a batch of tracked frames (300 correspondences, last
    keyframe and last-frame variants alternating), end to end per call (host gather + H2D + the one kernel + D2H); the CPU
    oracle's PoseOptimization restatement on the same frames beside it."""
    import numpy as np
    from mc_slam_amd import synth, backend, shard
    nb = args.batch
    distinct = [synth.make_frame(seed=shard.window_seed(g), n_obs=300, last_is_frame=bool(i % 2))
                for i, g in enumerate(shard.window_ids(16 * world, rank, world))]
    frames = [distinct[i % len(distinct)] for i in range(nb)]
    ba = backend.LocalBA(local_rank)
    packed = ba.pose_pack(frames)
    meter = shard.ThroughputMeter(dist, torch.cuda.synchronize)
    for _ in range(args.warmup):
        ba.pose_run(packed)
    # the call updates the frames in place: the (Python-side) reset of the inputs between steps stays outside the clock
    total, dt = 0, 0.0
    for _ in range(args.steps):
        ba.pose_reset(packed)
        meter.start()
        ba.pose_call(packed)
        n_step, t_step = meter.stop(nb, device="cuda")
        total += n_step
        dt += t_step
    res = [b.get(s_) for b, s_ in zip(packed[2], packed[1])]
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, [{"nav": r.nav, "its_done": r.its_done, "status": r.status, "n_inliers": r.n_inliers,
                                          "outlier": r.outlier, "outlier_last": r.outlier_last, "chi2_round": r.chi2_round,
                                          "marg_cov_inv": r.marg_cov_inv} for r in res])
    out = None
    if rank == 0:
        out = {"metric": "IMU-aided PoseOptimization frames/sec (300 correspondences) [extra measurement]", "value": total / dt, "unit": "frames/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
               "config": {"workload": "Optimizer::PoseOptimization(Frame*, KeyFrame*|Frame*, IMUPreintegrator, gw, bComputeMarg): 4 x optimize(10) LM + "
                                      "reclassification + marginals per frame", "frames_per_gpu_per_step": nb, "distinct_frames": len(distinct)}}
    if rank == 0 and args.full:
        cpu, verified = None, "batch self-consistent"
        for i, r in enumerate(res):
            j = i % len(distinct)
            if r.its_done != res[j].its_done or (r.nav != res[j].nav).any():
                raise SystemExit("bench: frame %d did not solve like its twin %d" % (i, j))
        if not args.no_cpu_baseline:
            import oracle_lib
            t0 = time.perf_counter()
            ros = [oracle_lib.pose_optimize(f) for f in distinct]
            tc = time.perf_counter() - t0
            for r, ro in zip(res, ros):
                if r.its_done != ro.its_done or (r.outlier != ro.outlier).any() or np.abs(r.nav[:3] - ro.nav[:3]).max() > 1e-6:
                    raise SystemExit("bench: a frame does not match the CPU oracle")
            verified += "; %d distinct frames == oracle (LM iterations, outlier bitmap, P 1e-6 m)" % len(distinct)
            cpu = {"value": len(distinct) / tc, "unit": "frames/s", "cores": 1, "kind": "port",
                   "sample": "%d frames, single thread, oracle/libvba_oracle.so" % len(distinct)}
        out.update({"roofline": None, "cpu_baseline": cpu, "verified": verified})
    finish(dist, rank, out)


def matches_oracle(np, sol, res, qo, ro):
    """BASELINE.json bars: same iteration counts and outlier bitmap, final chi2 <= 1e-4 rel, keyframe translations <= 1e-6 m"""
    return (ro.its_done == res.its_done and ro.status == res.status and abs(ro.chi2_vis - res.chi2_vis) <= 1e-4 * max(ro.chi2_vis, 1e-300)
            and (ro.obs_outlier == res.obs_outlier).all() and np.abs(qo.kf_pose[:, :3] - sol.kf_pose[:, :3]).max() <= 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=None, help="windows per GPU per step (default: 4096 for c3, 2048 for c2, 256 for c4, 4 for gba, 4096 frames for pose)")
    ap.add_argument("--distinct", type=int, default=None, help="distinct seeded windows generated per rank and replicated to fill the batch (default: 256 for c3, 16 for c2, 2 for c4 / gba)")
    ap.add_argument("--landmark-order", default="caller", choices=["caller", "random"],
                    help="local-window workloads (c3, c3s, c4, c2, c2s): 'caller' = landmarks in the order the reference's caller builds lLocalMapPoints in -- keyframe by "
                         "keyframe over lLocalKeyFrames, every keyframe appending the map points no earlier one has listed (src/Optimizer.cpp:59-78, 3877-3894), i.e. grouped by "
                         "the first local keyframe that observes them; 'random' = the generator's order (uncorrelated with the keyframes; the workload of rounds 1-3a)")
    ap.add_argument("--iteration-mix", default="r3", choices=["r3", "r2"],
                    help="c3: 'r3' = three kinds of window (5+3 / 4..5+2 / 3..4+1 Gauss-Newton iterations: 60 / 20 / 20 %%, the workload since round 3); 'r2' = every "
                         "window of the first kind (all 5+3): the iteration mix of rounds 1-2, same sizes -- with --landmark-order random the round-2 workload exactly")
    ap.add_argument("--uniform", action="store_true", help="c3: every window exactly 50 KF / 5 000 landmarks / 30 000 edges instead of sizes drawn around it")
    ap.add_argument("--workload", default="c3", choices=["c2", "c3", "c4", "gba", "pose", "c3s", "c2s"],
                    help="c3 = BASELINE configs[2] (the headline metric); c2 / c4 = configs[1] / configs[3], gba = map-scale global BA, pose = IMU-aided per-frame pose "
                         "optimisation, c3s / c2s = configs[2] / configs[1] with scattered co-visibility (tracks with gaps, fixed co-observers): extra measurements")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pcg", action="store_true", help="c4 / gba: skip the second run of the batch with the PCG solver")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--e2e-chi2", action="store_true", help="end to end: also bring the per-edge chi2 back (an optional output of the C-ABI, 8 B per edge; the reference's "
                    "caller reads the erase list only)")
    ap.add_argument("--e2e-steps", type=int, default=4, help="timed vba_batch_solve calls over fresh copies of the batch (0: skip)")
    ap.add_argument("--gen-procs", type=int, default=None, help="worker processes that generate the synthetic windows (default: up to 16; 1 under a profiler)")
    ap.add_argument("--single-reps", type=int, default=21, help="vba_solve repetitions behind single_window_ms (0: skip)")
    ap.add_argument("--full", action="store_true", help="beyond the headline figure: the checks against replicas and the CPU oracle, end to end, "
                    "single window, roofline, CPU baselines, PCG and tile products (the options above that select among them apply here only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one handed back as DIR/<name>.npy")
    args = ap.parse_args()
    if args.batch is None:
        args.batch = {"c2": 2048, "c3": 4096, "c4": 256, "gba": 4, "pose": 4096, "c3s": 4096, "c2s": 2048}[args.workload]
    if args.distinct is None:
        args.distinct = {"c2": 64, "c3": 256, "c4": 2, "gba": 2, "pose": 16, "c3s": 64, "c2s": 64}[args.workload]

    # `python bench.py --gpus N` (no torchrun): start the N ranks ourselves, before this process touches torch or the GPU
    from mc_slam_amd import launch
    if launch.needs_self_launch(args.gpus, os.environ):
        sys.exit(launch.spawn_ranks(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    # one process per GPU: bind this rank to its share of the host cores (and size the backend's host pool to it) before
    # anything starts a thread or touches the GPU; a single rank keeps the whole machine
    my_cpus = launch.pin_rank(os.environ)

    # synthetic windows; window w of the job belongs to rank w % world, seed 100 + w.  Generated by forked
    # worker processes before torch / HIP are initialised in this one.
    from mc_slam_amd import shard
    specs = []
    if args.workload != "pose":
        n_distinct = max(1, min(args.distinct, args.batch))
        specs = [(args.workload, shard.window_seed(g), args.uniform, args.landmark_order, args.iteration_mix) for g in shard.window_ids(n_distinct * world, rank, world)]
    # under rocprofv3 the profiler's preloaded library has initialised the GPU runtime before main(): forking such a process is
    # what this pool forbids (children inherit the runtime's locks; an intermittent hang of a PMC pass was traced to it) -> serial
    profiled = any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", "")
    n_proc = max(1, min(16, len(my_cpus)))
    if args.gen_procs is not None:
        n_proc = max(1, args.gen_procs)
    elif profiled:
        n_proc = 1
    wins = make_windows(specs, n_proc)

    import numpy as np
    import torch

    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if os.environ.get("BENCH_TEST_ONE_GPU"):   # rehearsal of the N>1 path on a one-GPU box: every rank on cuda:0, gloo
            local_rank = 0
            torch.cuda.set_device(0)
            dist.init_process_group("gloo", rank=rank, world_size=world)
            args.batch = max(256, args.batch // world)   # the ranks share one card's HBM here: the rehearsal checks the launcher, not the rate
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP backend has no CPU path")
    torch.cuda.set_device(local_rank)

    from mc_slam_amd import backend

    if args.workload == "pose":
        return bench_pose(args, rank, local_rank, world, dist, torch)

    batch = [wins[i % len(wins)] for i in range(args.batch)]
    ba = backend.LocalBA(local_rank)
    ba.upload(batch)

    # ---- (1) resident: inputs in HBM, K x vba_batch_run ----
    meter = shard.ThroughputMeter(dist, torch.cuda.synchronize)
    for _ in range(args.warmup):
        ba.run()
    meter.start()
    for _ in range(args.steps):
        ba.run()          # vba_batch_run returns after the stream has drained
    total_windows, dt = meter.stop(args.batch * args.steps, device="cuda")
    value = total_windows / dt

    sol = res = None
    if args.full or args.dump_outputs:
        sol, res = ba.download()   # what the last timed run handed back: states, erase list and per-edge chi2 of every window
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, [{"kf_pose": s_.kf_pose, "kf_vel": s_.kf_vel, "kf_bias": s_.kf_bias, "pt": s_.pt,
                                          "status": r.status, "its_done": r.its_done, "chi2_vis": r.chi2_vis, "chi2_prv": r.chi2_prv,
                                          "chi2_bias": r.chi2_bias, "n_outliers": r.n_outliers, "lambda_final": r.lambda_final,
                                          "lin_iterations": r.lin_iterations, "chi2_trace": r.chi2_trace, "obs_outlier": r.obs_outlier,
                                          "obs_chi2": r.obs_chi2} for s_, r in zip(sol, res)])
    rng = lambda f: [int(min(f(w) for w in wins)), int(max(f(w) for w in wins))]
    out = None
    if rank == 0:
        out = {
            "metric": {"c3": "LocalBA windows/sec (50 KF, 5k pts, 30k obs, IMU edges)",
                       "c3s": "LocalBA windows/sec, scattered co-visibility (50 free + 8 fixed KF, 5k pts, 30k obs, IMU edges) [extra measurement]",
                       "c2s": "vision-only LocalBundleAdjustment windows/sec, scattered co-visibility (20 KF, 2k pts, 12k obs) [extra measurement]",
                       "c2": "vision-only LocalBundleAdjustment windows/sec (20 KF, 2k pts, 12k obs) [extra measurement]",
                       "c4": "synthetic VI graph solves/sec (200 KF, 50k pts, 500k obs) [extra measurement]",
                       "gba": "global BA solves/sec (300 KF, 30k pts, 180k obs, IMU chain) [extra measurement]"}[args.workload],
            "value": value, "unit": "windows/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            # `value` = kernel-only rate: inputs resident in HBM when the clock starts (the bench contract's definition);
            # `value_end_to_end` (--full) = the same windows handed over as fresh host arrays, PCIe both ways included
            "value_kernel_only": value,
            "config": {"workload": {"c3": "BASELINE configs[2]: LocalBAPRVIDP windows, 50 KF (49 free + fixed predecessor) / 5000 IDP landmarks / "
                                          "30000 EdgePRIDP + 49 PRV + 49 bias edges, GN 5+10" + ("" if args.uniform else
                                          "; sizes drawn per seed around it: 40..60 KF (mean 50), 100 landmarks per KF, 6 edges per landmark"),
                                    "c2": "BASELINE configs[1]: vision-only LocalBundleAdjustment, 20 KF (18 free) / 2000 XYZ landmarks / "
                                          "12000 EdgeSE3ProjectXYZ, LM 5+10",
                                    "c3s": "BASELINE configs[2] with scattered co-visibility: 50 free + 8 fixed co-observer KF / 5000 IDP landmarks / 30000 "
                                           "EdgePRIDP whose tracks are random subsets of the keyframes in view (gaps), ~20 % of the landmarks with a fixed "
                                           "reference keyframe, GN 5+10",
                                    "c2s": "BASELINE configs[1] with scattered co-visibility (tracks = random subsets of the keyframes in view), LM 5+10",
                                    "c4": "BASELINE configs[3]: synthetic VI graph, 200 KF / 50000 IDP landmarks / 500000 EdgePRIDP + IMU "
                                          "chain, GN 5+10",
                                    "gba": "GlobalBundleAdjustmentNavStatePRV, 300 KF / 30000 XYZ landmarks / 180000 EdgeNavStatePRPointXYZ "
                                           "+ IMU chain, LM optimize(10)"}[args.workload],
                       "landmark_order": (args.landmark_order + (" (grouped by first local keyframe, as src/Optimizer.cpp:59-78 builds lLocalMapPoints)" if args.landmark_order == "caller" else
                                                                 " (uncorrelated with the keyframes)")) if args.workload in ("c3", "c3s", "c4", "c2", "c2s") else None,
                       "windows_per_gpu_per_step": args.batch, "distinct_windows": len(wins),
                       "n_kf_range": rng(lambda w: w.n_kf), "n_pt_range": rng(lambda w: w.n_pt), "n_obs_range": rng(lambda w: w.n_obs),
                       "mean_n_kf": float(np.mean([w.n_kf for w in batch])), "mean_n_obs": float(np.mean([w.n_obs for w in batch])),
                       "parallelism": "independent windows sharded %d per GPU, no data-path collective" % args.batch,
                       "value_is": "kernel-only (windows resident in HBM, no PCIe in the timed region)" + ("; value_end_to_end includes H2D + D2H" if args.full else ""),
                       "host_threads": int(ba.lib.vba_host_threads()), "cpu_affinity": {"cores": len(my_cpus), "first": my_cpus[0], "last": my_cpus[-1]},
                       "iteration_mix": args.iteration_mix if args.workload == "c3" and not args.uniform else None},
        }
    if not args.full:
        return finish(dist, rank, out)

    # the timed work must be the real work: every window of the last timed run finished both stages, windows built from the
    # same seed agree bit for bit, and (rank 0) EVERY distinct window matches the CPU oracle
    def check_twins(sol, res, what):
        for i, r in enumerate(res):
            j = i % len(wins)
            if r.status != 0 or r.its_done[0] < 1 or (min(r.its_done) < 1 and batch[0].protocol == 0) or r.its_done != res[j].its_done \
                    or r.chi2_vis != res[j].chi2_vis or (sol[i].kf_pose != sol[j].kf_pose).any():
                raise SystemExit("bench (%s): window %d did not solve like its twin %d: %s vs %s" % (what, i, j, (r.status, r.its_done), res[j].its_done))
    check_twins(sol, res, "resident")
    verified = "every window finished both stages; replicas agree bit for bit"
    oracle_res, oracle_ms = None, None
    full_oracle = args.workload in ("c2", "c3", "c3s", "c2s")   # every distinct window; C4 / GBA (5-10 s per oracle solve): the first window, below
    big_oracle = None
    if rank == 0 and not args.no_cpu_baseline and not full_oracle:
        import oracle_lib
        mode = 1 if args.workload == "c4" else 0   # the faster elimination order of the oracle at this shape (measured)
        t_big, qo, ro = oracle_lib.solve_timed(wins[0], solver_mode=mode)
        if not matches_oracle(np, sol[0], res[0], qo, ro):
            raise SystemExit("bench: window 0 does not match the CPU oracle: its %s vs %s, chi2 %r vs %r" % (res[0].its_done, ro.its_done, res[0].chi2_vis, ro.chi2_vis))
        big_oracle = (t_big, mode)
        verified += "; window 0 == oracle (iterations, outlier bitmap, chi2 1e-4 rel, t 1e-6 m)"
    if rank == 0 and not args.no_cpu_baseline and full_oracle:
        import oracle_lib
        from concurrent.futures import ThreadPoolExecutor
        oracle_lib.lib()
        nthr = max(1, min(len(my_cpus), 64))

        def one(w):
            t1 = time.perf_counter()
            r = oracle_lib.solve(w)
            return r, time.perf_counter() - t1
        with ThreadPoolExecutor(max_workers=nthr) as ex:   # ctypes releases the GIL
            oracle_res = list(ex.map(one, wins))
        for i, ((qo, ro), _t) in enumerate(oracle_res):
            if not matches_oracle(np, sol[i], res[i], qo, ro):
                raise SystemExit("bench: distinct window %d (seed %d) does not match the CPU oracle: its %s vs %s, chi2 %r vs %r" % (
                    i, specs[i][1], res[i].its_done, ro.its_done, res[i].chi2_vis, ro.chi2_vis))
        verified += "; all %d distinct windows == oracle (iterations, outlier bitmap, chi2 1e-4 rel, t 1e-6 m)" % len(wins)
    its_hist = {}
    for r in res[:len(wins)]:
        k = "%d+%d" % tuple(r.its_done)
        its_hist[k] = its_hist.get(k, 0) + 1

    # ---- (2) end to end: fresh host arrays in, solved host arrays out ----
    e2e = None
    if args.e2e_steps > 0:
        packed = ba.pack(batch, want_chi2=args.e2e_chi2)
        ba.solve_packed(packed)                      # warm-up: lanes, pinned staging and device buffers get allocated
        tot_e, dt_e = 0, 0.0
        for _ in range(args.e2e_steps):
            ba.pack_reset(packed)                    # the solve writes the states in place: the reset stays outside the clock
            meter.start()
            ba.solve_packed(packed)
            n_step, t_step = meter.stop(args.batch, device="cuda")
            tot_e += n_step
            dt_e += t_step
        sol_e, res_e = ba.pack_results(packed)
        check_twins(sol_e, res_e, "end to end")
        for i in range(len(wins)):                   # the streamed call must give what upload + run + download gave
            if res_e[i].its_done != res[i].its_done or res_e[i].chi2_vis != res[i].chi2_vis or (sol_e[i].kf_pose != sol[i].kf_pose).any() \
                    or (sol_e[i].pt != sol[i].pt).any() or (res_e[i].obs_outlier != res[i].obs_outlier).any():
                raise SystemExit("bench: vba_batch_solve and upload+run+download disagree on window %d" % i)
        e2e = {"value": tot_e / dt_e, "unit": "windows/s", "steps": args.e2e_steps, "ms_per_step": dt_e / args.e2e_steps * 1e3,
               "frac_of_resident": (tot_e / dt_e) / value,
               "what": "vba_batch_solve on fresh copies of the batch: host packing + H2D + structure build + solve + D2H + scatter, chunks in flight concurrently; "
                       "back come states, landmarks and the erase list" + (" and the per-edge chi2" if args.e2e_chi2 else " (the optional per-edge chi2 is not requested: --e2e-chi2)")}
        del packed, sol_e, res_e

    if rank == 0:
        # ---- (3) one window at a time, the way LocalMapping calls the reference (src/LocalMapping.cpp:1026-1037) ----
        single = None
        oracle_mode = 1 if args.workload == "c4" else 0
        if args.single_reps > 0 and args.workload in ("c2", "c3", "c3s", "c2s"):
            import ctypes as C
            from mc_slam_amd import abi, synth
            w1 = synth.config_c3(seed=3, landmark_order=args.landmark_order) if args.workload == "c3" else wins[0]
            ba1 = backend.LocalBA(local_rank)
            ts = []
            for k in range(args.single_reps + 3):
                q = w1.copy()
                s = q.as_struct()
                rb = abi.ResultBuf(q.n_obs)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if ba1.lib.vba_solve(ba1.h, C.byref(s), C.byref(rb.s), None) != 0:
                    raise SystemExit("bench: vba_solve failed")
                ts.append(time.perf_counter() - t1)
            ts = sorted(ts[3:])
            single = {"ms": ts[len(ts) // 2] * 1e3, "min_ms": ts[0] * 1e3, "reps": len(ts),
                      "what": "median wall time of vba_solve (H2D + structure + two-stage solve + D2H) on one fresh window, BASELINE configs[%d] seed %s" % (
                          2 if args.workload in ("c3", "c3s") else 1, "3" if args.workload == "c3" else str(specs[0][1]))}
            single["kernel_launches"] = ba1.get_profile()["kernel_launches"]   # launches one vba_solve enqueued (vba_profile)
            if args.workload == "c3":
                # The reference's actual call: LocalMapping::Run -> Optimizer::LocalBAPRVIDP(pKF, lLocalKeyFrames, &mbAbortBA, ...) once per
                # keyframe (src/LocalMapping.cpp:1035).  The C++ facade with that signature on a mock KeyFrame / MapPoint map holding this
                # window: graph extraction (src/Optimizer.cpp:49-451), vba_solve_b behind it, erase + write-back under the map lock
                # (:496-623) -- a fresh map per repetition (the call changes the map).
                try:
                    import facade_lib
                    facade_lib.lib().fc_set_device(local_rank)
                    fts = []
                    for k in range(max(3, min(args.single_reps, 7)) + 2):
                        fm = facade_lib.FacadeMap(w1)
                        flag = C.c_bool(False)
                        fm.local_ba_prvidp_flag(flag)
                        fts.append(fm.last_timing())
                        r_f = facade_lib.lib().fc_last_result().contents
                        if r_f.status != 0:
                            raise SystemExit("bench: the facade call did not finish (status %d)" % r_f.status)
                        fm.close()
                    fts = fts[2:]
                    med = lambda key: float(sorted(t[key] for t in fts)[len(fts) // 2])
                    single["facade"] = {"total_ms": med("total_ms"), "extract_ms": med("extract_ms"), "solve_ms": med("solve_ms"),
                                        "writeback_ms": med("writeback_ms"), "overhead_us": (med("total_ms") - med("solve_ms")) * 1e3,
                                        "reps": len(fts),
                                        "what": "median wall time of Optimizer::LocalBAPRVIDP (mc_slam_amd/host) on a mock map holding the same window: "
                                                "extraction + vba_solve_b + erase / write-back; the map's float32 storage makes its window "
                                                "differ from `ms`'s in rounding only"}
                except OSError as ex:
                    single["facade"] = {"error": "libvba_facade.so not built: %s" % ex}
            if not args.no_cpu_baseline:
                import oracle_lib
                # ONE baseline for the whole line: both elimination orders of the oracle are timed on this window (best of 3
                # each, -O3 -march=native build), the faster one is the CPU side of `single_window` AND of `cpu_baseline`
                best = {}
                for mode in (0, 1):
                    for _ in range(3):
                        t_o, qo, ro = oracle_lib.solve_timed(w1, solver_mode=mode)
                        best[mode] = min(best.get(mode, 1e30), t_o)
                    if not matches_oracle(np, q, rb.get(), qo, ro):
                        raise SystemExit("bench: the single window does not match the CPU oracle (mode %d)" % mode)
                oracle_mode = 0 if best[0] <= best[1] else 1
                single["cpu_oracle_1core_ms"] = best[oracle_mode] * 1e3
                single["cpu_oracle_mode"] = ["natural (g2o vertex-id) order", "V/Bias-first order"][oracle_mode]
                single["cpu_oracle_ms_by_mode"] = {"natural": best[0] * 1e3, "vbias_first": best[1] * 1e3}
                single["cpu_oracle_build"] = oracle_lib.timing_lib()[1]
                single["speedup_vs_cpu_1core"] = single["cpu_oracle_1core_ms"] / single["ms"]
            ba1.close()

        # ---- roofline of the dominant kernel class: a separate profiled run (HIP events around every launch of the
        # class, on the backend's stream), never mixed into `value`
        ba.set_profile(True)
        ba.run()
        pf = ba.get_profile()
        ba.set_profile(False)
        classes = {k: v for k, v in pf.items() if isinstance(v, dict)}
        dom = max(classes, key=lambda k: classes[k]["ms"])
        its = [sum(r.its_done) for r in res]
        alg_bytes = classes[dom]["bytes"]   # algorithmic bytes of the class over the whole run (vba_profile)
        dur_s = classes[dom]["ms"] * 1e-3
        launches = max(1, classes[dom]["launches"])
        achieved = alg_bytes / dur_s / 1e9 if dur_s > 0 else 0.0
        roofline = {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": 8000.0, "unit": "GB/s",
                    "frac": achieved / 8000.0, "traffic": None,
                    "avg_launch_ms": classes[dom]["ms"] / launches, "launches": launches,
                    "class_ms": {k: round(v["ms"], 4) for k, v in classes.items() if v["launches"]},
                    "class_frac": {k: round(v["bytes"] / (v["ms"] * 1e-3) / 8e12, 5) for k, v in classes.items()
                                   if k in ("linearize", "schur", "factor", "update") and v["launches"] and v["ms"] > 0 and v["bytes"] > 0},
                    "profiled_total_ms": pf["total_ms"]}
        # HBM traffic of the dominant class from the committed rocprofv3 PMC passes (FETCH_SIZE corrected x2 per the MI355X
        # guide, + WRITE_SIZE), per class launch -- only when that profile was taken from THESE kernel sources and batch size
        try:
            import glob
            # the profile taken from THESE kernel sources (a fresh checkout gives every file the same mtime: match by content, newest name last)
            cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_traffic.json")))
            match = [f for f in cands if json.load(open(f)).get("csrc_sha") == csrc_sha() and json.load(open(f)).get("batch") == args.batch]
            tj = (match or cands)[-1]
            tr = json.load(open(tj))
            if tr.get("batch") == args.batch and tr.get("csrc_sha") == csrc_sha() and tr.get("workload", "c3") == args.workload:
                kmap = {"schur": ["k_schur_all", "k_schur_all_w", "k_schur_diag", "k_schur_off", "k_schur_ref"], "linearize": ["k_lin2", "k_lin2_imu", "k_lin_imu"],
                        "factor": ["k_chol_step", "k_chol_step3", "k_chol_step4", "k_chol_panel", "k_chol_update", "k_chol_diag_ll", "k_chol_diag_ll2", "k_chol_panel_ll"],
                        "trsv": ["k_trsv", "k_trsv_w", "k_trsv_p"], "update": ["k_update"]}
                ks = [tr["kernels"][k] for k in kmap.get(dom, []) if k in tr["kernels"]]
                n_cls = max(k["active_launches"] for k in ks)
                roofline["traffic"] = sum((k["fetch_corrected"] + k["write"]) * k["active_launches"] for k in ks) / n_cls
                roofline["traffic_source"] = os.path.basename(tj)
                # algorithmic bytes of ONE launch that covers every window of the batch (the PMC figures are per such launch; the
                # class average above also counts the launches in which part of the windows have already converged)
                npw = lambda w_: (6 if w_.variant == 0 else 15) * w_.n_kf_free
                full = {"schur": sum(8.0 * npw(w_) ** 2 for w_ in batch), "factor": sum(16.0 * npw(w_) ** 2 for w_ in batch),
                        "trsv": sum(8.0 * npw(w_) ** 2 for w_ in batch),
                        "linearize": sum(32.0 * w_.n_obs + 36.0 * w_.n_pt + 432.0 * w_.n_kf_free for w_ in batch),
                        "update": sum(36.0 * w_.n_pt + 432.0 * w_.n_kf_free for w_ in batch)}.get(dom)
                roofline["algorithmic_bytes_full_launch"] = full
                roofline["traffic_over_algorithmic"] = roofline["traffic"] / full if full else None
                # what the class really writes (the Schur kernels are credited with n_p^2 * 8 per solve but write only the blocks of
                # S that are ever read -- 15 % of it): the same fraction against the bytes written
                wr = sum(k["write"] * k["active_launches"] for k in ks) / n_cls
                roofline["written_bytes_per_launch"] = wr
                roofline["frac_by_written_bytes"] = wr / (classes[dom]["ms"] / launches * 1e-3) / 8e12
                roofline["fetch_correction"] = ("x2 (FETCH_SIZE = TCC_EA0_RDREQ x 64 B; every fabric read request of these kernels is a 128-B "
                                                "request: TCC_EA0_RDREQ_128B == TCC_EA0_RDREQ, profiles/round3_tcc_request_sizes.txt)")
            else:
                roofline["traffic_note"] = "no PMC profile of these kernel sources (csrc %s) at this batch size is committed" % csrc_sha()
        except Exception:
            pass
        # the dense solve (north_star: "MFMA utilisation reported against gfx950 peak"): FP64 flop the factorisation class
        # executed with v_mfma_f64_16x16x4 (tile products of the symbolic lists x 2*32^3) over its HIP-event time, against
        # the 78.6 TFLOP/s FP64 matrix peak of the MI355X
        if classes["factor"]["ms"] > 0:
            tf = classes["factor"]["flops"] / (classes["factor"]["ms"] * 1e-3) / 1e12
            roofline["mfma_factor"] = {"achieved": tf, "peak": 78.6, "unit": "TFLOP/s", "frac": tf / 78.6, "dtype": "f64"}

        # what the Schur walk is actually bound by: scattered 64-byte record fetches.  Records a window's
        # walk fetches per launch: two per item of its off-diagonal pairs (sum over landmarks of m (m + 1) / 2 for m observations + the
        # reference record) and a slot + an edge record per observation in the diagonal pass; over the launches each window was active in.
        if dom == "schur" and batch[0].variant == 2 and classes[dom]["ms"] > 0:
            recs = 0.0
            for wdw, it_w in zip(batch, its):
                m = np.diff(wdw.pt_obs_begin).astype(np.float64)
                recs += (2.0 * float((m * (m + 1) / 2).sum()) + 2.0 * wdw.n_obs + wdw.n_pt) * it_w
            roofline["record_fetch"] = {"achieved": recs / (classes[dom]["ms"] * 1e-3) / 1e9, "unit": "G records/s",
                                        "ceiling_l2_resident": 174.0, "ceiling_past_l2": 78.0,
                                        "what": "scattered 64-byte record fetches of the Schur class per second; ceilings: scripts/gather_rate_probe.hip on MI355X "
                                                "(profiles/round4_gather_rate_probe.txt): a lane reading a random record in three 16-byte pieces, table inside / past the XCD's L2; "
                                                "the class time is measured with the other window groups' kernels sharing the chip (the plain gather alone on one stream: "
                                                "184 G records/s, profiles/round4_schur_split_probe.txt)"}

        cpu = None
        if not args.no_cpu_baseline:
            import oracle_lib
            oracle_lib.lib()
            if oracle_res is not None:
                # every distinct window was solved by the oracle above (one window per thread); its 1-core rate is measured
                # on a bounded sample, one solve at a time, nothing else running
                n_done, t_cpu = 0, 0.0
                while t_cpu < args.cpu_seconds and n_done < len(wins):
                    t_cpu += oracle_lib.solve_timed(wins[n_done], solver_mode=oracle_mode)[0]
                    n_done += 1
            else:
                n_done, t_cpu = 0, 0.0
                if big_oracle is not None:
                    t_cpu, n_done, oracle_mode = big_oracle[0], 1, big_oracle[1]
            if n_done:
                cpu = {"value": n_done / t_cpu, "unit": "windows/s", "cores": 1, "kind": "port",
                       "sample": "%d solves of the first distinct windows of the batch, single thread, oracle/vba_oracle.c built -O3 -march=%s, "
                                 "LDL^T in %s (the faster of its two orders on this box; same mode as single_window.cpu_oracle_1core_ms) -- a "
                                 "restatement of the reference's g2o path, NOT g2o itself (no Eigen3 in the image)" % (
                                     n_done, oracle_lib.timing_lib()[1], ["natural order", "V/Bias-first order"][oracle_mode])}
            if cpu is not None and oracle_res is not None:
                # the same oracle on every host core at once, one window per thread (the reference itself
                # solves on one thread, src/System.cpp:198; this is the generous reading)
                from concurrent.futures import ThreadPoolExecutor
                ncores = max(1, min(len(my_cpus), 64))
                per = 2
                t1 = time.perf_counter()
                with ThreadPoolExecutor(max_workers=ncores) as ex:
                    list(ex.map(lambda k: oracle_lib.solve_timed(wins[k % len(wins)], solver_mode=oracle_mode), range(per * ncores)))
                t_all = time.perf_counter() - t1
                cpu["all_cores"] = {"value": per * ncores / t_all, "unit": "windows/s", "cores": ncores,
                                    "sample": "%d solves, %d threads, one window per thread" % (per * ncores, ncores)}
        # BASELINE configs[3] says "Schur + PCG": the same batch with vba_problem.solver = VBA_SOLVER_PCG beside the LDL^T figure
        pcg = None
        if args.workload in ("c4", "gba") and not args.no_pcg:
            from mc_slam_amd import abi
            pw = []
            for w_ in wins:
                q_ = w_.copy(); q_.solver = abi.SOLVER_PCG; pw.append(q_)
            bp = backend.LocalBA(local_rank)
            n_pcg = min(args.batch, 16)              # (CG runs ~1 400 iterations per solve: a smaller batch keeps the leg at a few seconds)
            bp.upload([pw[i % len(pw)] for i in range(n_pcg)])
            bp.run()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            for _ in range(2):
                bp.run()
            torch.cuda.synchronize(); tp = (time.perf_counter() - t1) / 2
            solp, resp = bp.download()
            for i in range(len(wins)):
                if resp[i].its_done != res[i].its_done or abs(resp[i].chi2_vis - res[i].chi2_vis) > 1e-4 * res[i].chi2_vis \
                        or np.abs(solp[i].kf_pose[:, :3] - sol[i].kf_pose[:, :3]).max() > 1e-6:
                    raise SystemExit("bench: the PCG path does not land where the LDL^T path lands (window %d)" % i)
            n_p = (6 if batch[0].variant == 0 else 15) * batch[0].n_kf_free
            pcg = {"value": n_pcg / tp, "unit": "windows/s", "ms_per_step": tp * 1e3, "windows": n_pcg, "vs_ldlt": (n_pcg / tp) / value,
                   "cg_iterations_per_solve": float(np.mean([r.lin_iterations / max(1, sum(r.its_done)) for r in resp])), "n_p": n_p,
                   "what": "same batch, vba_problem.solver = VBA_SOLVER_PCG (block-Jacobi PCG on the reduced system, tolerance 1e-10); "
                           "iteration counts, chi2 (1e-4) and translations (1e-6 m) equal to the LDL^T run"}
            bp.close()
        tile_products = None
        if batch[0].variant != 0:   # visual-inertial windows: tile products of the symbolic factorisation under both elimination orders
            import ctypes as C
            tp = np.zeros((len(wins), 5), dtype=np.int64)
            bh = backend.LocalBA(local_rank, hooks=True)   # (a diagnostic of the symbolic factorisation: the hooks flavour of the library)
            bh.upload(wins)
            for i in range(len(wins)):
                bh.lib.vba_debug_tile_products(bh.h, i, tp[i].ctypes.data_as(C.c_void_p))
            bh.close()
            if (tp[:, 0] >= 0).all():
                tile_products = {"vbias_first_mean": float(tp[:, 0].mean()), "keyframe_order_mean": float(tp[:, 1].mean()),
                                 "two_sided_mean": float(tp[:, 4].mean()) if (tp[:, 4] >= 0).all() else None,
                                 "windows_in_keyframe_order": int((tp[:, 2] == 1).sum()), "windows_two_sided": int((tp[:, 2] == 2).sum()),
                                 "chosen_mean": float(tp[:, 3].mean())}
        out["value_end_to_end"] = None if e2e is None else e2e["value"]
        out["single_window_ms"] = None if single is None else single["ms"]
        out["config"].update({"its_done_histogram": its_hist, "tile_products_per_factorisation": tile_products,
                              "mean_outer_iterations": float(np.mean(its))})
        out.update({
            # work-normalised: outer (Gauss-Newton / LM) iterations of all windows per second -- comparable across iteration mixes
            "window_iterations_per_s": value * float(np.mean(its)),
            "end_to_end": e2e, "single_window": single, "pcg": pcg,
            "roofline": roofline, "cpu_baseline": cpu, "verified": verified,
        })
    finish(dist, rank, out)


if __name__ == "__main__":
    main()
