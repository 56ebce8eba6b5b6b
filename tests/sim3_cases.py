"""The seeded loop candidates of the Sim3 tests, in one place: tests/test_gpu_sim3.py compares the GPU with tests/sim3_ref.py on
them, tests/test_sim3_ref.py asserts (on the CPU) the two conditions that comparison rests on for every seed and budget listed."""
from mc_slam_amd import synth

SHORT = dict(its_stage1=3, its_stage2_bad=2, its_stage2_clean=2)     # every lambda, rho and nu of the schedule shows in the estimate
FULL = dict(its_stage1=5, its_stage2_bad=10, its_stage2_clean=5)     # the reference's budgets (src/Optimizer.cpp:4724, :4749-4752)

# (seed, n_pairs, fix_scale, outlier_frac, same_K)
SCHEDULE = [
    (101, 25, False, 0.0, False),
    (101, 120, False, 0.1, True),
    (101, 400, False, 0.3, False),
    (101, 120, True, 0.1, False),
    (105, 25, True, 0.0, True),
    (101, 400, True, 0.3, True),
    (101, 120, False, 0.0, False),
]
# result parity at the reference's budgets: the same problems and three more
RESULT = SCHEDULE + [
    (102, 25, False, 0.0, False),
    (102, 200, False, 0.1, True),
    (101, 60, True, 0.1, False),
]


def make(case, budgets):
    seed, n, fix, frac, same_k = case
    p = synth.make_sim3_pair(seed, n, fix_scale=fix, outlier_frac=frac, same_K=same_k)
    for k, v in budgets.items():
        setattr(p, k, v)
    return p


def case_id(case):
    return "seed%d-n%d-%s-o%g-%s" % (case[0], case[1], "fixed" if case[2] else "free", case[3], "sameK" if case[4] else "K1K2")
