"""How often the chi2-only probe of a linearisation pass (LIN_AUTO / LIN_REDO, mc_slam_amd/csrc/vba_batch.h) is right, on the 256
distinct windows of bench.py's C3 workload (synth.config_c3_ragged, seeds 100..355, caller landmark order, three kinds).

CPU only by default: every window is solved by the oracle, and the rule of k_ctrl_gn -- pass p of a stage is a probe when p >= 2, it
is not the stage's scheduled final evaluation and the chi2 decrease of pass p - 1 was below T -- is replayed on its chi2 trace, for
T in {1, 10, 30, 100}.  Per T: the passes that are probes (n_probe), the probes behind which the window went on (n_redo = wrong
predictions: the full pass is run after all) and the stops by convergence a probe caught, of all such stops.  Writes
profiles/lin_probe_predictor.json.

--device: also solves the same 256 windows as one batch on the GPU (hooks flavour of the library) with the rule (T = 10) and with
every pass probed, sums WinCtrl::n_probe / n_redo over the windows and adds them to the file beside the replayed numbers; iteration
counts match the oracle, so the sums must be equal.

    python scripts/lin_probe_predictor.py [--device] [--distinct 256] [--procs 8]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LIMITS = (5, 10)
THRESHOLDS = (1.0, 10.0, 30.0, 100.0)


def _window(seed):
    from mc_slam_amd import synth
    return synth.config_c3_ragged(seed=seed, landmark_order="caller", kinds=True)


def _oracle(seed):
    import oracle_lib
    r = oracle_lib.solve(_window(seed))[1]
    return seed, r.status, tuple(r.its_done), [float(x) for x in r.chi2_trace]


def stages(its_done, trace):
    m0, m1 = its_done
    assert len(trace) == m0 + 1 + m1 + 1, (its_done, len(trace))
    return (trace[:m0 + 1], m0, LIMITS[0]), (trace[m0 + 1:], m1, LIMITS[1])


def replay(its_done, trace, T):
    """(n_probe, n_redo, stops caught) of one window under threshold T (T = None: every pass that may be a probe)"""
    n_probe = n_redo = caught = 0
    for c, m, L in stages(its_done, trace):
        for p in range(2, min(m, L - 1) + 1):
            if T is None or abs(c[p - 2] - c[p - 1]) < T:
                n_probe += 1
                n_redo += p < m
                caught += p == m
    return n_probe, n_redo, caught


def device_counters(seeds, mode):
    """sum of (n_probe, n_redo) over the windows of one batch run with vba_debug_set_path(h, "lin_probe", mode), and their its_done"""
    from mc_slam_amd import backend
    ba = backend.LocalBA(0, hooks=True)
    try:
        lib = ba.lib
        lib.vba_debug_set_path.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
        lib.vba_debug_copy.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_uint64]
        lib.vba_debug_window_layout.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64]
        assert lib.vba_debug_set_path(ba.h, b"lin_probe", mode) == 0
        ba.upload([_window(s) for s in seeds]); ba.run()
        _, rs = ba.download()
        lay = np.zeros(4096, np.int64)
        assert lib.vba_debug_window_layout(ba.h, 0, lay.ctypes.data_as(C.POINTER(C.c_int64)), len(lay)) == 0
        size = int(lay[13])
        raw = np.zeros(len(seeds) * size, np.uint8)
        assert lib.vba_debug_copy(ba.h, lib.vba_debug_buf_id(b"CTRL"), 0, raw.ctypes.data, raw.nbytes) == 0
        cnt = raw.reshape(len(seeds), size)[:, size - 8:].copy().view(np.int32)
        return [int(x) for x in cnt.sum(axis=0)], [tuple(r.its_done) for r in rs]
    finally:
        ba.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lin_probe_predictor.json"))
    args = ap.parse_args()
    seeds = [100 + i for i in range(args.distinct)]
    import multiprocessing as mp
    with mp.get_context("fork").Pool(max(1, args.procs)) as pool:   # (forked before anything touches the GPU)
        sols = pool.map(_oracle, seeds, chunksize=1)
    assert all(st == 0 for _, st, _, _ in sols)
    hist = {}
    for _, _, its, _ in sols:
        hist["%d+%d" % its] = hist.get("%d+%d" % its, 0) + 1
    full = sum(min(m, L - 1) + 1 for _, _, its, _ in sols for m, L in zip(its, LIMITS) if m > 0)
    stops = sum(1 <= m < L for _, _, its, _ in sols for m, L in zip(its, LIMITS))
    final = sum(m == L for _, _, its, _ in sols for m, L in zip(its, LIMITS))
    out = {"windows": len(seeds), "seeds": [seeds[0], seeds[-1]], "its_done": dict(sorted(hist.items(), key=lambda kv: -kv[1])),
           "lin_full_passes": full, "lin_full_needed": full - stops, "stops_by_convergence": stops, "scheduled_lin_err_passes": final,
           "stops_in_pass_1": sum(m == 1 and L > 1 for _, _, its, _ in sols for m, L in zip(its, LIMITS)), "thresholds": {}}
    for T in THRESHOLDS + (None,):
        tot = np.sum([replay(its, tr, T) for _, _, its, tr in sols], axis=0)
        out["thresholds"]["every_pass" if T is None else "%g" % T] = {"n_probe": int(tot[0]), "n_redo_wrong_predictions": int(tot[1]), "stops_caught": int(tot[2])}
    if args.device:
        out["device"] = {}
        for name, mode in (("10", 1), ("every_pass", 2)):
            cnt, its = device_counters(seeds, mode)
            out["device"][name] = {"n_probe": cnt[0], "n_redo_wrong_predictions": cnt[1], "its_done_equal_oracle": its == [s[2] for s in sols]}
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
