"""What a batch of n windows is expected to take (mc_slam_amd/csrc/vba_host_plan.h), restated from the documented thresholds
(DESIGN.md "regime") and shared by tests/test_host_plan.py (CPU harness) and tests/test_gpu_plan.py
(vba_debug_plan).  The field order is the documented order of vba_host::plan_ints."""
FIELDS = ("n_win left_looking chain_on two_sided arena_on inc_copy results_block dev_stop hist_block row_lds zero_s pcg "
          "schur factor trsv step_form imu_lin poll pace_depth pcg_tri dbg_stop_after ngroups word_report").split()
N_UPLOAD = 12                     # the first twelve are the UploadPlan
SE3_XYZ, PRV_XYZ, PRV_IDP = 0, 1, 2
GN, LM = 0, 1
SCHUR_ALL_W, SCHUR_ALL, SCHUR_SPLIT_W, SCHUR_SPLIT, SCHUR3_W, SCHUR3 = range(6)
FACTOR_STEP1, FACTOR_STEP4, FACTOR_STEP4_ONE, FACTOR_LL, FACTOR_PCG = 1, 4, 5, 6, 7
TRSV_P, TRSV = 0, 1
IMU_FUSED, IMU_PAIR, IMU_RES_HESS = 0, 1, 2


def expected(n, variant=PRV_IDP, algo=GN, pcg=0, ll_min=256):
    """the plan under an empty environment (ll_min: vba_debug_set_ll_min)"""
    ll = n >= ll_min
    e = dict(n_win=n,
             left_looking=int(ll),
             chain_on=int(ll or n <= 64),                 # right-looking: up to VBA_CHAIN_RL_MAX = 64 windows
             two_sided=1,
             arena_on=int(n <= 8),                        # VBA_ARENA_MAX
             inc_copy=int(n > 8),
             results_block=int(n < 4),
             dev_stop=int(n >= 64),
             hist_block=1024 if n <= 64 else 256,
             row_lds=0,
             zero_s=int(ll or pcg),
             pcg=pcg,
             schur=((SCHUR_ALL if n >= 8 else SCHUR_ALL_W) if variant == PRV_IDP else (SCHUR3 if n >= 8 else SCHUR3_W)),
             factor=FACTOR_PCG if pcg else FACTOR_LL if ll else FACTOR_STEP4_ONE if n == 1 else FACTOR_STEP4,
             trsv=-1 if pcg else TRSV if ll else TRSV_P,
             step_form=4,
             imu_lin=IMU_RES_HESS if n >= 64 else IMU_FUSED if variant == PRV_IDP else IMU_PAIR,
             poll=int(n >= 64),
             pace_depth=1 if n < 8 else 2,
             pcg_tri=1,
             dbg_stop_after=-1,
             ngroups=4 if n >= 64 else 2 if n >= 16 else 1,
             word_report=int(n == 1 and algo == GN))
    return [e[k] for k in FIELDS]
