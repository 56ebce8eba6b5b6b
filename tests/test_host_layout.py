"""The description half of an upload (mc_slam_amd/csrc/vba_host_layout.h: check_window, describe_window, BatchCursor, LaunchGeom)
under AddressSanitizer + UBSan (CPU only).  Every expectation below is derived from the sizes of the problems -- the offsets as
prefix sums, the rows of the reduced system from the layout rules of the three elimination orders restated here -- and the two
encodings of a dof's position (the descriptor fields the kernels read, and vpos_host) are compared entry by entry."""
import os

import pytest

from mc_slam_amd import abi, synth
import host_check_lib as hc

NB = 32
ORDERS = [None, 0, 1, 2]      # VBA_ORDER unset (the library's choice) and the three orders forced


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return hc.build(tmp_path_factory, "host_layout_check")


@pytest.fixture(scope="module")
def windows(tmp_path_factory):
    """name -> (problem, file): the small shapes of test_host_structure.py"""
    d = tmp_path_factory.mktemp("hlw")
    ps = {"idp12": synth.make_window(abi.VARIANT_PRV_IDP, n_kf=12, n_fixed=1, n_pt=400, n_obs=2400, seed=41),
          "idp9": synth.make_window(abi.VARIANT_PRV_IDP, n_kf=9, n_fixed=3, n_pt=150, n_obs=700, seed=42),
          "idp70": synth.make_window(abi.VARIANT_PRV_IDP, n_kf=70, n_fixed=1, n_pt=900, n_obs=5400, seed=44),     # two-word landmark masks
          "idp4": synth.make_window(abi.VARIANT_PRV_IDP, n_kf=4, n_fixed=1, n_pt=60, n_obs=150, seed=47),          # n_free = 3: order 2 does not apply
          "se3": synth.make_window(abi.VARIANT_SE3_XYZ, algo=abi.ALGO_LM, n_kf=10, n_fixed=2, n_pt=300, n_obs=1800, seed=43),
          "prv": synth.make_window(abi.VARIANT_PRV_XYZ, algo=abi.ALGO_LM, n_kf=10, n_fixed=1, n_pt=300, n_obs=1800, seed=45),
          "c3": synth.config_c3(seed=3)}
    out = {}
    for k, p in ps.items():
        f = str(d / (k + ".vbap"))
        abi.save_problem(f, p)
        out[k] = (p, f)
    return out


# the batches of one harness run: a large inverse-depth batch, then a small one (the geometry must not remember the first), then the XYZ variants
BATCHES = [["idp12", "idp9", "idp70", "c3", "idp4"], ["idp9", "idp4"], ["se3", "se3"], ["prv"]]


def _run(checker, args, order=None):
    env = dict(os.environ)
    env.pop("VBA_ORDER", None)
    if order is not None:
        env["VBA_ORDER"] = str(order)
    return hc.run(checker, args, env=env, timeout=600)


def _fields(line):
    t = line.split()
    if t[0] == "end":
        t = t[1:]
    f = {}
    for k, v in zip(t[0::2], t[1::2]):
        f[k] = ([] if v == "-" else [int(x) for x in v.split(",")]) if k in ("vpos", "vpos_host", "pad0", "padn") else int(v)
    return f


@pytest.fixture(scope="module")
def described(checker, windows):
    """order -> per batch (window lines, end line), one harness run per order"""
    args = []
    for b in BATCHES:
        args += ["--"] + [windows[k][1] for k in b]
    out = {}
    for order in ORDERS:
        lines = _run(checker, args[1:], order)
        assert not [l for l in lines if not l.startswith(("win ", "end "))], lines
        batches, cur = [], []
        for l in lines:
            if l.startswith("end "):
                batches.append((cur, _fields(l)))
                cur = []
            else:
                cur.append(_fields(l))
        assert [len(b[0]) for b in batches] == [len(b) for b in BATCHES]
        out[order] = batches
    return out


def _cdiv(a, b):
    return (a + b - 1) // b


def _two_sided(nf):
    """keyframes in the first chain, first row of the second chain, first row of the PR blocks (order 2: both chains and the PR
    part start at a tile boundary; the split near the middle with the fewest tile rows)"""
    best = None
    for c in range(max(1, nf // 2 - 3), min(nf - 1, nf // 2 + 3) + 1):
        ta, tb = _cdiv(9 * c, NB), _cdiv(9 * (nf - c), NB)
        cost = 64 * max(ta, tb - 1) + (ta + tb)
        if best is None or cost < best[0]:
            best = (cost, c, NB * ta, NB * (ta + tb))
    return best[1:]


def _expected_nS(order, pdim, nf):
    rows = pdim * nf
    if pdim == 15 and order == 2:
        rows = _two_sided(nf)[2] + 6 * nf
    return _cdiv(rows, NB) * NB


def _sizes(p):
    se3 = p.variant == abi.VARIANT_SE3_XYZ
    return dict(n_kf=p.n_kf, n_free=p.n_kf_free, n_pt=p.n_pt, n_obs=p.n_obs, n_imu=0 if se3 else p.n_imu, pdim=6 if se3 else 15)


@pytest.mark.parametrize("order", ORDERS)
def test_offsets_are_prefix_sums_of_the_sizes(described, windows, order):
    for names, (wins, end) in zip(BATCHES, described[order]):
        acc = dict(kf0=0, pt0=0, obs0=0, imu0=0, pair0=0, vec0=0, S0=0, mask0=0)
        for i, (k, f) in enumerate(zip(names, wins)):
            z = _sizes(windows[k][0])
            for key, v in z.items():
                assert f[key] == v, (k, key)
            if order is not None:
                assert f["order"] == (0 if z["pdim"] == 6 or (order == 2 and z["n_free"] < 4) else order), k
            assert f["order"] in ((0, 1, 2) if z["pdim"] == 15 else (0,))
            nS = _expected_nS(f["order"], z["pdim"], z["n_free"])
            assert f["win"] == i and f["nS"] == nS and nS % NB == 0 and f["nb"] == nS // NB and f["np"] == z["pdim"] * z["n_free"]
            assert f["n_pairs"] == z["n_free"] * (z["n_free"] + 1) // 2 and f["mwords"] == _cdiv(z["n_kf"], 64)
            for key, v in acc.items():
                assert f[key] == v, (k, key, f[key], v)
            acc["kf0"] += z["n_kf"]; acc["pt0"] += z["n_pt"]; acc["obs0"] += z["n_obs"]; acc["imu0"] += z["n_imu"]
            acc["pair0"] += f["n_pairs"]; acc["vec0"] += nS; acc["S0"] += nS * nS; acc["mask0"] += z["n_pt"] * _cdiv(z["n_kf"], 64)
        assert end["windows"] == len(names) and end["S_tot"] == acc["S0"]
        for key in ("kf0", "pt0", "obs0", "imu0", "pair0", "vec0", "mask0"):
            assert end[key] == acc[key], key


@pytest.mark.parametrize("order", ORDERS)
def test_both_encodings_of_a_dof_position_agree(described, order):
    two_sided_seen = False
    for wins, _ in described[order]:
        for f in wins:
            nS, n = f["nS"], f["pdim"] * f["n_free"]
            assert f["vpos"] == f["vpos_host"] and len(f["vpos"]) == n
            assert len(set(f["vpos"])) == n and min(f["vpos"]) >= 0 and max(f["vpos"]) < nS       # injective into [0, nS)
            pads = [r for p0, pn in zip(f["pad0"], f["padn"]) for r in range(p0, p0 + pn)]
            assert all(pn >= 0 for pn in f["padn"]) and len(set(pads)) == len(pads)                 # the pad ranges are disjoint
            assert set(pads) == set(range(nS)) - set(f["vpos"])                                     # ... and exactly the rows of no variable
            two_sided_seen = two_sided_seen or (f["order"] == 2 and f["padn"][1] + f["padn"][2] > 0)
    if order == 2:
        assert two_sided_seen      # the pads on both sides of the second chain were exercised


@pytest.mark.parametrize("order", ORDERS)
def test_geometry_is_the_maximum_over_the_batch(described, windows, order):
    ends = []
    for names, (wins, end) in zip(BATCHES, described[order]):
        z = [_sizes(windows[k][0]) for k in names]
        ps = [windows[k][0] for k in names]
        npairs = [s["n_free"] * (s["n_free"] + 1) // 2 for s in z]
        nS = [_expected_nS(f["order"], s["pdim"], s["n_free"]) for f, s in zip(wins, z)]
        want = dict(max_pt_blk=max(_cdiv(s["n_pt"], 64) for s in z), max_imu=max(s["n_imu"] for s in z), max_pairs=max(npairs),
                    max_nb=max(nS) // NB, max_obs_blk=max(_cdiv(s["n_obs"], 64) for s in z), max_kf_blk=max(_cdiv(s["n_kf"], 64) for s in z),
                    max_ns_blk=max(_cdiv(v, 64) for v in nS), max_nS=max(nS), max_its0=max(p.its_stage1 for p in ps), max_its1=max(p.its_stage2 for p in ps),
                    max_free=max(s["n_free"] for s in z), max_quads=max([1] + [(q - s["n_free"] + 3) // 4 for q, s in zip(npairs, z)]),
                    max_offp=max([1] + [q - s["n_free"] for q, s in zip(npairs, z)]), max_kf=max(s["n_kf"] for s in z),
                    max_mwords=max(_cdiv(s["n_kf"], 64) for s in z),
                    # quantities of the structure, as each window reports them
                    max_lin_blk=max(f["n_part_lin"] for f in wins), max_pan=max(f["pan"] for f in wins), min_nc=min(f["nc"] for f in wins),
                    max_nc=max(f["nc"] for f in wins), max_cu=max(f["n_cu"] for f in wins), max_split=max(f["nc_split"] for f in wins),
                    max_chain_rows=max(f["nb"] - f["nc"] if f["nc"] > 0 else 0 for f in wins),
                    chain_lds=max((f["nc"] * (f["nb"] - f["nc"]) + 2 * f["nc"] + 8) * 2 for f in wins),
                    tile_updates=sum(f["tiles"] for f in wins), step_grid=max(nS) // NB, pan_grid=max(nS) // NB,
                    any_lin_fallback=int(any(f["lin_runs"] == 0 for f in wins)))
        for key, v in want.items():
            assert end[key] == v, (names, key, end[key], v)
        for f, s in zip(wins, z):
            assert f["n_part_pt"] == _cdiv(s["n_pt"], 64) and f["its0"] >= 0
        ends.append(end)
    # the second batch is a subset of the first and smaller in every respect: its geometry is its own, not the first batch's
    for key in ("max_pt_blk", "max_pairs", "max_nb", "max_obs_blk", "max_kf_blk", "max_nS", "max_free", "max_quads", "max_offp", "max_pan", "max_kf",
                "max_mwords", "max_lin_blk", "tile_updates", "step_grid"):
        assert ends[1][key] < ends[0][key], key


def test_every_refusal_names_its_cause(checker, windows):
    idp, se3, c3 = windows["idp12"][1], windows["se3"][1], windows["idp9"][1]
    p = windows["idp12"][0]
    gn_only = "inverse-depth landmarks are solved with Gauss-Newton only (as the reference does, src/Optimizer.cpp:136)"
    lm_only = "XYZ landmarks are solved with Levenberg-Marquardt only (as the reference does, src/Optimizer.cpp:1028,3928)"
    nothing = "a window without landmarks or observations has nothing to optimise"
    cases = [(["@variant=3", idp], 0, "bad variant / algo"), (["@variant=-1", idp], 0, "bad variant / algo"), (["@algo=7", idp], 0, "bad variant / algo"),
             (["@algo=%d" % abi.ALGO_LM, idp], 0, gn_only), (["@algo=%d" % abi.ALGO_GN, se3], 0, lm_only),
             (["@n_kf_free=0", idp], 0, "bad sizes"), (["@n_kf_free=%d" % (p.n_kf + 1), idp], 0, "bad sizes"), (["@n_imu=-1", idp], 0, "bad sizes"),
             (["@n_pt=-1", idp], 0, "bad sizes"), (["@n_obs=-2", idp], 0, "bad sizes"),
             (["@imu_null=1", idp], 0, "n_imu > 0 but an IMU array is NULL"),
             (["@n_pt=0", idp], 0, nothing), (["@n_obs=0", idp], 0, nothing),
             ([idp, se3], 1, "mixed batch"), ([idp, "@solver=%d" % abi.SOLVER_PCG, c3], 1, "mixed batch"),
             (["@solver=7", idp], 0, "unknown solver"),
             (["@its_stage1=31", idp], 0, "its out of range"), (["@its_stage2=-1", idp], 0, "its out of range"),
             (["@protocol=9", idp], 0, "unknown protocol"),
             # the first cause in the order of the checks wins
             (["@protocol=9", "@its_stage1=31", "@n_kf_free=0", idp], 0, "bad sizes")]
    assert p.n_imu > 0
    args = []
    for a, _, _ in cases:
        args += ["--"] + a
    lines = _run(checker, args[1:])
    got = [l for l in lines if l.startswith("refused ")]
    assert len(got) == len(cases) and not [l for l in lines if l.startswith("end ")], lines
    for (a, w, msg), line in zip(cases, got):
        assert line == "refused %d %s" % (w, msg), (a, line)
