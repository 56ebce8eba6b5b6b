"""Asynchronous batches (vba_batch_submit / poll / wait) on the GPU: every ticket gives bit for bit what upload + run + download
(or vba_batch_solve / _b with the same stop flag) of its batch gives, whatever the depth and the order of the waits; pending
tickets are observable (test hook), a rejected window fails its ticket only, misuse fails with a message, and closing a handle
finishes its pending tickets."""
import ctypes as C

import numpy as np
import pytest

from mc_slam_amd import abi, backend, synth

pytestmark = pytest.mark.gpu

STATES = ("kf_pose", "kf_vel", "kf_bias", "pt")
VBA_ABORTED_BEFORE = 2   # include/vislam_ba.h: stop flag set on entry, nothing touched
SCALARS = ("chi2_vis", "chi2_prv", "chi2_bias", "its_done", "status", "n_outliers", "lambda_final", "lin_iterations")


def _small(variant, i, seed0=300):
    kw = dict(n_fixed=1) if variant == abi.VARIANT_PRV_IDP else dict(n_fixed=2)
    return synth.make_window(variant, n_kf=7 + (i % 4), n_pt=120 + 15 * (i % 6), n_obs=600 + 70 * (i % 6), seed=seed0 + i % 6, **kw)


@pytest.fixture(scope="module")
def W():
    """every window of the module, built before the first GPU call"""
    idp = [_small(abi.VARIANT_PRV_IDP, i) for i in range(29)]
    gba = []
    for s in (6, 7):
        g = synth.config_gba(seed=s, n_kf=12, n_pt=300, n_obs=1800, its=5)
        assert g.protocol == abi.PROTO_SINGLE and g.kf_fix is not None
        gba.append(g)
    bad = idp[4].copy()
    bad.obs_kf = bad.obs_kf.copy()
    bad.obs_kf[5] = 99
    return dict(
        idp=idp,
        se3=[_small(abi.VARIANT_SE3_XYZ, i, 310) for i in range(8)],
        prv=[_small(abi.VARIANT_PRV_XYZ, i, 320) for i in range(3)],
        one=[idp[2]],
        gba=gba,
        many=[idp[i % 6] for i in range(260)],   # >= 256 windows: the left-looking regime
        bad=bad,
    )


@pytest.fixture(scope="module")
def ba(W):
    b = backend.LocalBA(0, hooks=True)
    yield b
    b.close()


@pytest.fixture(scope="module")
def ref(W):
    b = backend.LocalBA(0, hooks=True)
    yield b
    b.close()


def _urd(ref, probs, cache={}):
    """upload + run + download of the batch on the second handle: (solved copies, Results)"""
    key = tuple(id(p) for p in probs)
    if key not in cache:
        ref.upload(probs)
        ref.run()
        q, r = ref.download()
        cache[key] = ([x.copy() for x in q], r)
    return cache[key]


def _same(a, b):
    (qa, ra), (qb, rb) = a, b
    assert len(qa) == len(qb) == len(ra) == len(rb)
    for w, (x, y, s, t) in enumerate(zip(qa, qb, ra, rb)):
        for k in STATES:
            u, v = getattr(x, k), getattr(y, k)
            assert (u is None and v is None) or np.array_equal(u, v), (w, k)
        for k in SCALARS:
            assert getattr(s, k) == getattr(t, k), (w, k, getattr(s, k), getattr(t, k))
        assert np.array_equal(s.obs_outlier, t.obs_outlier), w
        assert (s.obs_chi2 is None and t.obs_chi2 is None) or np.array_equal(s.obs_chi2, t.obs_chi2), w
        assert np.array_equal(s.chi2_trace, t.chi2_trace), w


def test_tickets_equal_upload_run_download_across_shapes(ba, ref, W):
    batches = [W["idp"], W["se3"], W["prv"], W["one"], W["gba"], W["many"]]
    tickets = [ba.submit(b) for b in batches]
    assert tickets == sorted(tickets) and len(set(tickets)) == len(tickets)
    got = {t: ba.wait(t) for t in reversed(tickets)}
    for t, b in zip(tickets, batches):
        _same(got[t], _urd(ref, b))
    assert all(r.status == 0 for r in got[tickets[0]][1])


def test_depth_does_not_change_results(ref, W):
    batches = [W["idp"], W["se3"], W["idp"][:9]]
    want = [_urd(ref, b) for b in batches]
    for depth in (1, 2, 3):
        b = backend.LocalBA(0, hooks=True)
        try:
            b.set_depth(depth)
            ts = [b.submit(x) for x in batches]
            for t, w in zip(ts, want):
                _same(b.wait(t), w)
        finally:
            b.close()
    b = backend.LocalBA(0, hooks=True)
    try:
        for bad in (0, 5):
            with pytest.raises(RuntimeError, match="depth must be 1..4"):
                b.set_depth(bad)
    finally:
        b.close()


def test_pending_is_observable_with_the_hold_hook(ba, ref, W):
    batches = [W["idp"][:5], W["se3"][:4], W["idp"][5:13]]
    packs = [ba.pack(b) for b in batches]
    assert ba.lib.vba_debug_async_hold(ba.h, 1) == 0
    try:
        ts = [ba.submit_packed(p) for p in packs]
        for t in ts:
            assert ba.poll(t) is False
        for p, b in zip(packs, batches):   # no upload has started: the packed copies still hold the inputs
            for q, src in zip(p["own"], b):
                for k in STATES:
                    assert np.array_equal(getattr(q, k), getattr(src, k))
    finally:
        assert ba.lib.vba_debug_async_hold(ba.h, 0) == 0
    for t, b in zip(ts, batches):
        _same(ba.wait(t), _urd(ref, b))


def test_rejected_window_fails_its_ticket_only(ba, ref, W):
    good1, good3 = W["idp"][:6], W["se3"]
    mid = W["idp"][:1] + [W["bad"]] + W["idp"][6:13]
    t1, t2, t3 = ba.submit(good1), ba.submit(mid), ba.submit(good3)
    _same(ba.wait(t1), _urd(ref, good1))
    with pytest.raises(RuntimeError, match=r"vba_batch_submit, ticket %d, windows 0\.\.%d: " % (t2, len(mid) - 1)):
        ba.wait(t2)
    _same(ba.wait(t3), _urd(ref, good3))


def test_stop_flag_per_ticket(ba, ref, W):
    batch = W["idp"][:10]
    flag = C.c_uint8(1)
    t_stop = ba.submit(batch, stop=flag)
    t_free = ba.submit(batch)
    got_stop, got_free = ba.wait(t_stop), ba.wait(t_free)
    for stop, got in ((C.c_uint8(1), got_stop), (None, got_free)):
        packed = ref.pack(batch)
        ptr = C.cast(C.pointer(stop), C.c_void_p) if stop is not None else None
        assert ref.lib.vba_batch_solve_b(ref.h, packed["n"], packed["parr"], packed["rarr"], ptr) == 0
        _same(got, ref.pack_results(packed))
    assert all(r.status == VBA_ABORTED_BEFORE for r in got_stop[1])
    for q, src in zip(got_stop[0], batch):   # nothing was touched
        for k in STATES:
            assert np.array_equal(getattr(q, k), getattr(src, k))
    assert all(r.status == 0 for r in got_free[1])


def test_misuse_fails_with_a_message(ba, ref, W):
    with pytest.raises(RuntimeError, match="unknown or retired ticket"):
        ba.wait(10 ** 9)
    batch = W["idp"][:7]
    assert ba.lib.vba_debug_async_hold(ba.h, 1) == 0
    try:
        t = ba.submit(batch)
        for call in (lambda: ba.solve(W["idp"][0]), lambda: ba.upload(W["idp"][:2]), lambda: ba.solve_batch(W["idp"][:2]),
                     lambda: ba.set_depth(3)):
            with pytest.raises(RuntimeError, match="asynchronous batches pending"):
                call()
        assert ba.poll(t) is False
    finally:
        assert ba.lib.vba_debug_async_hold(ba.h, 0) == 0
    _same(ba.wait(t), _urd(ref, batch))
    with pytest.raises(RuntimeError, match="unknown or retired ticket"):
        ba.wait(t)
    with pytest.raises(RuntimeError, match="unknown or retired ticket"):
        ba.poll(t)
    q, r = ba.solve(W["idp"][0])   # everything retired: the handle works synchronously again
    q0, r0 = ref.solve(W["idp"][0])
    _same(([q], [r]), ([q0], [r0]))


def test_close_finishes_pending_tickets(ref, W):
    batch = W["idp"][:9]
    want = _urd(ref, batch)
    b = backend.LocalBA(0, hooks=True)
    packed = b.pack(batch)
    b.submit_packed(packed)
    b.close()                                   # the binding waits, then vba_destroy
    _same(b.pack_results(packed), want)
    b = backend.LocalBA(0, hooks=True)
    packed = b.pack(batch)
    b.submit_packed(packed)
    assert b.lib.vba_destroy(b.h) == 0          # the library itself finishes the pending ticket before it frees
    b.h = C.c_void_p()
    b._tickets = {}
    _same(b.pack_results(packed), want)
