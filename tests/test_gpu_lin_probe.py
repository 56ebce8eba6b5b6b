"""The chi2-only probe of a linearisation pass (LIN_AUTO / LIN_REDO, mc_slam_amd/csrc/vba_batch.h; plan_lin_probe): a Gauss-Newton
window whose last chi2 decrease was below 10 evaluates chi2 only in its next pass, and gets the full pass behind the control launch
if it goes on all the same.  The chi2 of a probe comes from the instructions of the full pass and the redone pass rewrites the same
partial sums, so every output is BIT FOR BIT what it is without the probe: that is what these tests assert, for the three settings
of vba_debug_set_path(h, "lin_probe", v) -- 0 off, 1 by the rule, 2 wherever a probe may run -- and for the default (no hook).

Windows: 7..9 keyframes, 20 landmarks per keyframe, 6 edges per landmark, the three kinds of bench.py's C3 windows (one pixel of
noise with 5 % gross outliers; 0.3 px; 0.1 px, both without outliers).  The oracle's iteration counts of the six seeds (asserted
below, no GPU): 5+2, 5+3, 5+3 (stage 1 to its limit, stage 2 of three iterations), 4+1, 3+1, 3+1 (both stages stop by |dchi2| <
1e-3); under the rule 705, 708, 709 and 704 have a stop caught, 702 and 705 are probed in vain once (a redo), and 701 and the
second stage of 702 stop without a probe.

Counters (WinCtrl::n_probe, n_redo: the last two ints of the control block), derived per stage from the oracle's trace c[0..m]
(m = its_done of the stage, L its limit).  k_ctrl_gn arms a probe in its call of pass p - 1 only if that call has it = p - 1 >= 1
(the stage then has a decrease to judge by) and leaves the window active, and pass L is the scheduled chi2-only evaluation that
every window gets.  So pass p is a probe iff 2 <= p <= min(m, L - 1), under the rule also |c[p-2] - c[p-1]| < 10; it is redone iff
the window goes on behind it, p < m.  Forced, n_redo = n_probe - (stages that stopped by convergence in a pass p >= 2); a stage that
stops in its pass 1 (its_done 1: every stage 2 of the 0.1-px windows) has no decrease before that pass and is never probed."""
import ctypes as C
import functools

import numpy as np
import pytest

from mc_slam_amd import abi, synth, backend
from test_gpu_parity import _check
from test_gpu_protocol_edges import _zero_pivot_window

gpu = pytest.mark.gpu

KINDS = ((1.0, 0.05), (0.3, 0.0), (0.1, 0.0))     # (pix_noise, outlier_frac) by seed % 3
SEEDS = (702, 705, 708, 709, 704, 701)
ITS = {702: (5, 2), 705: (5, 3), 708: (5, 3), 709: (4, 1), 704: (3, 1), 701: (3, 1)}
LIMITS = (5, 10)
T_PROBE = 10.0                                     # LIN_PROBE_DCHI2
N_BATCH = 66                                       # >= 64: probing is on by default


@functools.lru_cache(maxsize=None)
def window(seed):
    n_kf = 7 + (seed // 3) % 3
    pix, of = KINDS[seed % 3]
    return synth.make_window(abi.VARIANT_PRV_IDP, n_kf=n_kf, n_fixed=1, n_pt=20 * n_kf, n_obs=120 * n_kf, seed=seed, pix_noise=pix, outlier_frac=of)


@functools.lru_cache(maxsize=None)
def oracle_solution(seed):
    import oracle_lib
    return oracle_lib.solve(window(seed))


def batch(n):
    """n windows drawn from the seeds in turn: ragged (7, 8 and 9 keyframes side by side)"""
    return [SEEDS[i % len(SEEDS)] for i in range(n)]


def stage_traces(r):
    tr, m0, m1 = np.asarray(r.chi2_trace), r.its_done[0], r.its_done[1]
    assert len(tr) == m0 + 1 + m1 + 1
    return tr[:m0 + 1], tr[m0 + 1:]


def expected_counters(r, mode):
    """(n_probe, n_redo) of a window that ran to its end, from its trace (module docstring)"""
    n_probe = n_redo = 0
    for c, m, L in zip(stage_traces(r), r.its_done, LIMITS):
        for p in range(2, min(m, L - 1) + 1):
            if mode == 2 or (mode == 1 and abs(c[p - 2] - c[p - 1]) < T_PROBE):
                n_probe += 1
                n_redo += p < m
    return n_probe, n_redo


def test_the_seeds_cover_the_cases():
    """(no GPU) iteration counts, the three cases, no decrease near a threshold, and what the rule does with each window"""
    for s in SEEDS:
        p, (qo, ro) = window(s), oracle_solution(s)
        assert 7 <= p.n_kf <= 9 and p.n_pt == 20 * p.n_kf and p.n_obs == 6 * p.n_pt
        assert ro.status == 0 and ro.its_done == ITS[s], (s, ro.its_done)
        for c in stage_traces(ro):
            d = np.abs(np.diff(c))
            assert not ((d > 0.8 * T_PROBE) & (d < 1.25 * T_PROBE)).any() and not ((d > 0.8e-3) & (d < 1.25e-3)).any(), (s, d)
    its = [ITS[s] for s in SEEDS]
    assert any(a < 5 and 1 <= b < 10 for a, b in its)          # stops by convergence in each stage
    assert any(a == 5 for a, b in its) and any(b >= 3 for a, b in its)
    # (n_probe, n_redo) forced / by the rule, worked out by hand from the decreases: e.g. 705 has 1.3e5, 141, 2.7, 0.068, 0.0024 in
    # stage 1 (limit 5: passes 2..4 can be probes; the rule probes pass 4 behind the 2.7 and redoes it) and 58, 0.015, 6.6e-7 in
    # stage 2 (passes 2, 3; the rule probes pass 3 behind the 0.015, which stops the window)
    want = {702: ((4, 3), (1, 1)), 705: ((5, 4), (2, 1)), 708: ((5, 4), (1, 0)), 709: ((3, 2), (1, 0)), 704: ((2, 1), (1, 0)), 701: ((2, 1), (0, 0))}
    for s in SEEDS:
        ro = oracle_solution(s)[1]
        assert (expected_counters(ro, 2), expected_counters(ro, 1)) == want[s], s
        assert expected_counters(ro, 0) == (0, 0)
        stops = sum(2 <= m < L for m, L in zip(ro.its_done, LIMITS))
        assert expected_counters(ro, 2)[1] == expected_counters(ro, 2)[0] - stops


# ---- runs --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ba():
    b = backend.LocalBA(0, hooks=True)
    lib = b.lib
    lib.vba_debug_set_path.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    lib.vba_debug_set_streams.argtypes = [C.c_void_p, C.c_int32]
    lib.vba_debug_set_stop_after.argtypes = [C.c_void_p, C.c_int32]
    lib.vba_debug_copy.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.vba_debug_window_layout.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64]
    assert lib.vba_debug_set_path(b.h, b"lin_probe", 3) != 0 and lib.vba_debug_set_path(b.h, b"lin_probe", -2) != 0
    yield b
    b.close()


def _counters(ba, n):
    """[n, 2] n_probe, n_redo of the windows of the last run"""
    lay = np.zeros(2048, np.int64)
    assert ba.lib.vba_debug_window_layout(ba.h, 0, lay.ctypes.data_as(C.POINTER(C.c_int64)), len(lay)) == 0
    size = int(lay[13])
    raw = np.zeros(n * size, np.uint8)
    bid = ba.lib.vba_debug_buf_id(b"CTRL")
    assert bid >= 0 and ba.lib.vba_debug_copy(ba.h, bid, 0, raw.ctypes.data, raw.nbytes) == 0
    tail = raw.reshape(n, size)[:, size - 16:].copy().view(np.int32)    # lin_probe, lin_redo, n_probe, n_redo
    assert (tail[:, :2] == 0).all()                                     # no flag is left standing behind a run
    return tail[:, 2:]


def _solve(ba, seeds, mode, streams=0, stop_after=-1, probs=None):
    """upload + run + download with the hooks set for this run: [(problem, result)], counters"""
    lib = ba.lib
    probs = [window(s) for s in seeds] if probs is None else probs
    assert lib.vba_debug_set_path(ba.h, b"lin_probe", mode) == 0 and lib.vba_debug_set_streams(ba.h, streams) == 0
    assert lib.vba_debug_set_stop_after(ba.h, stop_after) == 0
    try:
        ba.upload(probs); ba.run()
        qs, rs = ba.download()
        return [(q.copy(), r) for q, r in zip(qs, rs)], _counters(ba, len(probs))
    finally:
        lib.vba_debug_set_path(ba.h, b"lin_probe", -1); lib.vba_debug_set_streams(ba.h, 0); lib.vba_debug_set_stop_after(ba.h, -1)


def _same_bits(a, b):
    (qa, ra), (qb, rb) = a, b
    assert ra.status == rb.status and ra.its_done == rb.its_done and ra.lambda_final == rb.lambda_final and ra.n_outliers == rb.n_outliers
    assert np.asarray(ra.chi2_trace).tobytes() == np.asarray(rb.chi2_trace).tobytes()
    assert (ra.chi2_vis, ra.chi2_prv, ra.chi2_bias) == (rb.chi2_vis, rb.chi2_prv, rb.chi2_bias)
    assert np.array_equal(ra.obs_outlier, rb.obs_outlier) and np.asarray(ra.obs_chi2).tobytes() == np.asarray(rb.obs_chi2).tobytes()
    for f in ("kf_pose", "kf_vel", "kf_bias", "pt"):
        assert getattr(qa, f).tobytes() == getattr(qb, f).tobytes(), f


def _check_counters(seeds, cnt, mode):
    for i, s in enumerate(seeds):
        assert tuple(cnt[i]) == expected_counters(oracle_solution(s)[1], mode), (i, s, mode, cnt[i])


_BATCH_RUNS = {}


def batch_runs(ba, streams=0):
    """the 66 windows with the probe off, by the rule, forced, and with no hook at all (-1): computed once per stream setting"""
    if streams not in _BATCH_RUNS:
        _BATCH_RUNS[streams] = {mode: _solve(ba, batch(N_BATCH), mode, streams) for mode in (0, 1, 2, -1)}
    return _BATCH_RUNS[streams]


@gpu
@pytest.mark.parametrize("streams", [0, 1], ids=["default_groups", "one_stream"])
def test_batch_of_66_is_bit_identical_in_every_mode_and_counts_as_derived(ba, streams):
    R, seeds = batch_runs(ba, streams), batch(N_BATCH)
    for mode in (1, 2, -1):
        for w in range(N_BATCH):
            _same_bits(R[0][0][w], R[mode][0][w])
    for mode in (0, 1, 2):
        _check_counters(seeds, R[mode][1], mode)
    _check_counters(seeds, R[-1][1], 1)                      # 66 windows: the rule is on without the hook
    assert R[1][1].sum() > 0 and R[2][1][:, 1].sum() > R[1][1][:, 1].sum()


@gpu
def test_probe_off_matches_the_oracle(ba):
    R, seeds = batch_runs(ba), batch(N_BATCH)
    for w in range(N_BATCH):
        q, r = R[0][0][w]
        _check(window(seeds[w]), q, r, *oracle_solution(seeds[w]))


@gpu
@pytest.mark.parametrize("n", [1, 5, 9])
def test_few_windows_through_the_fused_kernel(ba, n):
    """below 64 windows the probe is off by default; forced on it runs through k_lin2_imu (edges and IMU factors in one launch)"""
    seeds = batch(n)
    off, c0 = _solve(ba, seeds, 0)
    dflt, cd = _solve(ba, seeds, -1)
    assert (c0 == 0).all() and (cd == 0).all()
    for mode in (1, 2):
        on, cnt = _solve(ba, seeds, mode)
        for w in range(n):
            _same_bits(off[w], on[w])
            _same_bits(off[w], dflt[w])
        _check_counters(seeds, cnt, mode)
    for w in range(n):
        _check(window(seeds[w]), off[w][0], off[w][1], *oracle_solution(seeds[w]))


@gpu
def test_vba_batch_solve_is_bit_identical_in_every_mode(ba):
    probs = [window(s) for s in batch(N_BATCH)]
    out = {}
    for mode in (0, 1, 2, -1):
        assert ba.lib.vba_debug_set_path(ba.h, b"lin_probe", mode) == 0
        try:
            qs, rs = ba.solve_batch(probs)
        finally:
            ba.lib.vba_debug_set_path(ba.h, b"lin_probe", -1)
        out[mode] = list(zip(qs, rs))
    for mode in (1, 2, -1):
        for w in range(N_BATCH):
            _same_bits(out[0][w], out[mode][w])


@gpu
@pytest.mark.parametrize("n", [9, N_BATCH])
@pytest.mark.parametrize("poll", [2, 3, 4, 6, 8])
def test_abort_at_a_poll_is_the_same_with_every_pass_probed(ba, n, poll):
    """polls 2..4 cut stage 1 (behind a probe, a redo, or in between), 6 and 8 cut stage 2; the control launches and hence the polls
    of a window are the same with and without the probe"""
    seeds = batch(n)
    off, c0 = _solve(ba, seeds, 0, stop_after=poll)
    on, c2 = _solve(ba, seeds, 2, stop_after=poll)
    for w in range(n):
        _same_bits(off[w], on[w])
    assert (c0 == 0).all()
    assert any(r.status == 1 for _, r in off) == (poll <= 4) and any(sum(r.its_done) < sum(ITS[s]) for s, (_, r) in zip(seeds, off))


@gpu
def test_failed_factorisation_is_the_same_with_every_pass_probed(ba):
    bad = _zero_pivot_window(synth.make_window(abi.VARIANT_PRV_IDP, n_kf=8, n_fixed=1, n_pt=200, n_obs=900, seed=40), 6)
    for n in (9, N_BATCH):
        probs = [window(s) for s in batch(n)]
        probs[4] = bad
        off, _ = _solve(ba, None, 0, probs=probs)
        on, _ = _solve(ba, None, 2, probs=probs)
        assert off[4][1].status == -2 and off[4][1].its_done == (1, 1)
        for w in range(n):
            _same_bits(off[w], on[w])
