"""The fixed-vertex patterns (vba_problem.kf_fix inside the free range) that tests/test_gpu_kf_fix.py runs on the GPU and
tests/test_stage_ref.py holds the reference to.  TEST INFRASTRUCTURE ONLY.

kf_fix bits: 1 PR, 2 V, 4 Bias.  The window has 12 keyframes, 10 of them listed as free (nS = 160)."""
import numpy as np

from mc_slam_amd import abi, synth

PATTERNS = {
    "pr_mid": {4: 1},              # PR fixed on a keyframe that is observer and reference
    "v_mid": {7: 2},               # identity rows inside the V/Bias columns the chain kernels own
    "b_mid": {5: 4},               # bias fixed: the bias-edge rule of imu_act
    "pr+v": {4: 1, 7: 2},          # the recorded finding
    "prod": {0: 5},                # the pattern production sends
    "all_mid": {4: 7},             # a wholly fixed keyframe listed as free
    "adj_all": {4: 7, 5: 7},       # an IMU edge with every vertex fixed (dropped)
    "first_last": {0: 1, 9: 7},    # both ends of the two-sided order
    "pr_v_same": {4: 3},           # two parts of one keyframe
    "vb_adj": {3: 6, 4: 6},        # neighbouring chain columns inactive
}
VARIANTS = {"idp": (abi.VARIANT_PRV_IDP, abi.ALGO_GN), "xyz": (abi.VARIANT_PRV_XYZ, abi.ALGO_LM)}


def window(variant, pattern, **kw):
    """the window of the recorded finding with the pattern's flags set"""
    var, algo = VARIANTS[variant]
    base = dict(n_kf=12, n_fixed=2, n_pt=400, n_obs=2000, seed=93, landmark_order="caller")
    base.update(kw)
    p = synth.make_window(var, algo=algo, **base)
    fix = np.zeros(p.n_kf, np.uint8)
    for kf, bits in PATTERNS[pattern].items():
        fix[kf] = bits
    p.kf_fix = fix
    return p
