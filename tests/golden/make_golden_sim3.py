"""Writes tests/golden/sim3_pairs.npz: inputs and the `analytic` outputs of tests/sim3_ref.py for four seeded loop candidates
(run from the repository root: python tests/golden/make_golden_sim3.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import sim3_cases  # noqa: E402
import sim3_ref    # noqa: E402

CASES = [(201, 25, False, 0.0, False), (202, 120, False, 0.1, True), (203, 120, True, 0.1, False), (204, 400, False, 0.3, False)]

if __name__ == "__main__":
    out = dict(n_problems=np.int64(len(CASES)))
    for k, c in enumerate(CASES):
        p = sim3_cases.make(c, sim3_cases.FULL)
        r = sim3_ref.optimize(p)
        out["case_%d" % k] = np.array([c[0], c[1], int(c[2]), int(c[4])], dtype=np.int64)
        out["frac_%d" % k] = np.float64(c[3])
        for name in ("S12", "p1c", "p2c", "uv1", "uv2", "w1", "w2", "K1", "K2"):
            out["%s_%d" % (name, k)] = getattr(p, name)
        out["n_inliers_%d" % k] = np.int64(r.n_inliers)
        out["n_bad_%d" % k] = np.int64(r.n_bad_stage1)
        out["its_%d" % k] = np.array(r.its_done, dtype=np.int64)
        out["outlier_%d" % k] = r.outlier
        out["S12_out_%d" % k] = r.S12
        out["chi2_stage_%d" % k] = r.chi2_stage
    np.savez_compressed(os.path.join(HERE, "sim3_pairs.npz"), **out)
    print("wrote sim3_pairs.npz:", os.path.getsize(os.path.join(HERE, "sim3_pairs.npz")), "bytes")
